"""GPU: the live-sample compaction of the decoder's backward (mipsf_decoder_live_compact, the list modes of
mipsf_decoder_bwd_chain16 / mipsf_decoder_wgrad16 / mipsf_hashgrid_dx_from_jac_list, ops.COMPACT_LIVE) against the same calls on
the live-tile lists: same record, same incoming gradient."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops, synth
from mipsfusion_amd.model import JointEncoding, MLP_reg

pytestmark = pytest.mark.gpu
PLS = float(2.0 ** (math.log2(256 / 16) / 15))
SHAPES = [1, 33, 64, 4096 + 17, 70000]          # 70000: more compact tiles than workgroups, the persistent kernels
PATTERNS = ("prefix", "every32", "scattered", "all", "none", "count32k", "count32k1", "few", "edges")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_dout(M, pattern, dev, seed):
    """-> (dout [M,10], live mask by construction or None).  Magnitudes as the losses give them (a mean over the batch)."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    dout = (torch.randn(M, 10, generator=gen) * torch.exp(torch.empty(M, 1).uniform_(-16.0, -6.0, generator=gen)))
    dout[dout == 0] = 1e-9
    idx = torch.arange(M)
    if pattern == "prefix":                      # a live prefix of 0..64 samples per 64-sample ray, 0 and 64 among them
        n_rays = (M + 63) // 64
        length = torch.randint(0, 65, (n_rays,), generator=gen)
        length[::7] = 0
        length[3::7] = 64
        keep = (idx % 64) < length.repeat_interleave(64)[:M]
    elif pattern == "every32":                   # a compact tile gathers from 32 source tiles
        keep = idx % 32 == 0
    elif pattern == "scattered":
        keep = torch.rand(M, generator=gen) < 0.01
        keep[M // 2] = True
    elif pattern == "all":
        keep = torch.ones(M, dtype=torch.bool)
    elif pattern == "none":
        keep = torch.zeros(M, dtype=torch.bool)
    elif pattern in ("count32k", "count32k1"):   # exactly 32 k live samples, and 32 k + 1 (31 pad lanes)
        n = 32 * max(1, (M // 2) // 32) + (1 if pattern == "count32k1" else 0)
        if n > M:
            return None, None
        keep = torch.zeros(M, dtype=torch.bool)
        keep[torch.randperm(M, generator=gen)[:n]] = True
    elif pattern == "few":                       # fewer than 32 live samples in the whole batch
        keep = torch.zeros(M, dtype=torch.bool)
        keep[torch.randperm(M, generator=gen)[:min(M, 7)]] = True
    elif pattern == "edges":                     # a subnormal-only sample is live, a sample of -0.0 only is dead
        keep = torch.zeros(M, dtype=torch.bool)
        keep[torch.randperm(M, generator=gen)[:min(M, 40)]] = True
        dout[~keep] = 0.0
        a, b = M // 3, (2 * M) // 3
        dout[a] = 0.0
        dout[a, 4] = 1e-42                       # subnormal: != 0.0f
        keep[a] = True
        if b != a:
            dout[b] = -0.0
            keep[b] = False
        return dout.to(dev).contiguous(), keep.numpy()
    dout[~keep] = 0.0
    return dout.to(dev).contiguous(), keep.numpy()


class Record:
    """One decoder, batch and forward record (lean: the record the exchange form reads), shared by the patterns of a case."""

    def __init__(self, dev, M, layout, prec):
        torch.manual_seed(11 + M)
        self.M, self.prec = M, prec
        dec = MLP_reg({}, input_ch=32, input_ch_pos=48).to(dev)
        self.ws = dec.ordered_parameters()
        self.packed16 = ops.decoder_pack16(self.ws, precision=prec)
        self.x = torch.rand(M, 3, device=dev)
        feat_aos = (torch.randn(M, 32, device=dev) * 0.3).contiguous()
        self.lay = _lib.FEAT_AOS if layout == "aos" else _lib.FEAT_LEVEL_MAJOR
        self.feat = feat_aos if layout == "aos" else feat_aos.view(M, 16, 2).permute(1, 0, 2).contiguous()
        self.out, self.saved = ops.decoder_fwd(None, self.feat, self.lay, self.x, None, M, save="lean", precision=prec,
                                               packed16=self.packed16)
        self.out_m, self.saved_m = ops.decoder_fwd(None, self.feat, self.lay, self.x, None, M, save="masks", precision=prec,
                                                   packed16=self.packed16)

    def bwd(self, dout, compact, grads, frozen_record=False, deterministic=False):
        keep = ops.COMPACT_LIVE
        ops.COMPACT_LIVE = compact
        try:
            out, saved = (self.out_m, self.saved_m) if frozen_record else (self.out, self.saved)
            return ops.decoder_bwd(None, self.feat, self.lay, self.x, None, out, dout, saved, grads, self.M, precision=self.prec,
                                   packed16=self.packed16, return_tiles=True, deterministic=deterministic)
        finally:
            ops.COMPACT_LIVE = keep

    def chain_dsmall(self, dout, compact):
        """The chain through the C API on a zeroed gradient record -> its small rows [M, 8] (d logits, d rgb)."""
        M, dev = self.M, dout.device
        dact = torch.zeros(_lib.buffer_size(_lib.SIZE_DECODER_DACT, M), dtype=torch.float32, device=dev)
        tile_live = torch.zeros(_lib.buffer_size(_lib.SIZE_DECODER_TILE_WORDS, M), dtype=torch.int32, device=dev)
        dfeat, dx = torch.empty_like(self.feat), torch.empty(M, 3, device=dev)
        ll = None
        if compact:
            ll = torch.empty(_lib.buffer_size(_lib.SIZE_DECODER_LIVE_LIST, M), dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().mipsf_decoder_live_compact(ops.dptr(dout), M, ops.dptr(ll, torch.int32), ops.dptr(dfeat),
                                                             ops.dptr(dx), self.lay, ops.stream_ptr()), "live_compact")
        a = _lib.DecoderChain16Args.new(M=M, packed16=ops.dptr(self.packed16), x=ops.dptr(self.x), out=ops.dptr(self.out),
                                        dout=ops.dptr(dout), saved=ops.dptr(self.saved), dfeat=ops.dptr(dfeat), dx=ops.dptr(dx),
                                        dact=ops.dptr(dact), tile_live=ops.dptr(tile_live, torch.int32), feat_layout=self.lay,
                                        flags=(4 if self.prec == "bf16x6" else 0) | 2, packed16_floats=self.packed16.numel(),
                                        live_list=ops.dptr(ll, torch.int32))
        _lib.check(_lib.lib().mipsf_decoder_bwd_chain16(C.byref(a), ops.stream_ptr()), "chain16")
        n_bt = (M + 127) // 128
        rec = _lib.buffer_size(_lib.SIZE_DECODER_DACT, M) - n_bt * 128 * 8
        return dact[rec:rec + M * 8].view(M, 8).clone(), dfeat, dx


def check_list(rec, dout, keep):
    """The pre-pass alone: list, padding, header, and the zeros of the dead samples (and nothing else written)."""
    M, dev = rec.M, dout.device
    ll = torch.full((_lib.buffer_size(_lib.SIZE_DECODER_LIVE_LIST, M),), 12345, dtype=torch.int32, device=dev)
    dfeat = torch.full_like(rec.feat, float("nan"))
    dx = torch.full((M, 3), float("nan"), device=dev)
    _lib.check(_lib.lib().mipsf_decoder_live_compact(ops.dptr(dout), M, ops.dptr(ll, torch.int32), ops.dptr(dfeat), ops.dptr(dx),
                                                     rec.lay, ops.stream_ptr()), "live_compact")
    words = ll.cpu().numpy().view(np.uint32)
    crit = (dout.cpu().numpy() != np.float32(0.0)).any(axis=1)
    assert np.array_equal(crit, keep), "the pattern is what it says"
    want = np.nonzero(crit)[0].astype(np.uint32)
    n, H = want.size, _lib.LIVE_HEADER
    assert words[0] == n and words[1] == (n + 31) // 32
    assert np.array_equal(words[H:H + n], want), "the live samples, ascending"
    assert np.all(words[H + n:H + 32 * ((n + 31) // 32)] == _lib.LIVE_PAD)
    df = dfeat if rec.lay == _lib.FEAT_AOS else dfeat.permute(1, 0, 2).reshape(M, 32)
    dead = torch.from_numpy(~crit).to(dev)
    assert not df[dead].any() and not dx[dead].any(), "zeros for the dead samples"
    assert bool(torch.isnan(df[~dead]).all()) and bool(torch.isnan(dx[~dead]).all()), "the live samples are left to the chain"
    return n


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("layout", ["aos", "level_major"])
@pytest.mark.parametrize("M", SHAPES)
def test_compacted_backward_equals_the_tile_list_path(dev, M, layout, prec):
    """Every liveness pattern on one record: the list is numpy's nonzero of the criterion; d(features), d(x) and the small
    rows of the gradient record are EQUAL to the uncompacted path's (a sample is one column of every product of the chain,
    wherever it sits); the ten parameter gradients agree at the gate of the zero-tile test, 1e-6 of the largest entry (the
    fp32 sums over the samples are grouped by other tiles: 24 mantissa bits, sums of at most 70000 terms accumulated per
    32-sample tile); a frozen decoder on the masks-only record gives the same d(features) and d(x); dx from the Jacobian in
    list mode equals the tiles= mode."""
    rec = Record(dev, M, layout, prec)
    meta = _lib.make_grid_meta(16, 2, 10, 16, PLS)
    params = torch.randn(meta.n_params, device=dev) * 0.1
    _, jac = ops.hashgrid_fwd(rec.x, params, meta, rec.lay, with_jac=True)
    ran = 0
    for k, pattern in enumerate(PATTERNS):
        dout, keep = make_dout(M, pattern, dev, 100 * k + M)
        if dout is None:
            continue
        ran += 1
        n_live = check_list(rec, dout, keep)
        g_c, g_u = [torch.zeros_like(w) for w in rec.ws], [torch.zeros_like(w) for w in rec.ws]
        df_u, dx_u, _, tiles_u = rec.bwd(dout, False, g_u)
        df_c, dx_c, _, tiles_c = rec.bwd(dout, True, g_c)
        assert isinstance(tiles_c, ops.LiveList) and torch.is_tensor(tiles_u)
        assert ops.last_live_tile_share() == ((n_live + 31) // 32) / ((M + 31) // 32)
        assert torch.equal(df_c, df_u) and torch.equal(dx_c, dx_u), pattern
        for name, a, b in zip(ops.DECODER_PARAM_ORDER, g_c, g_u):
            e = rel_err(a, b)
            assert e <= 1e-6, f"{pattern}: grad {name}: max error relative to max magnitude {e:.3e}"
        if pattern == "none":
            assert n_live == 0 and not df_c.any() and not dx_c.any() and all(not g.any() for g in g_c)
        # frozen decoder, masks-only record
        df_f, dx_f, _, _ = rec.bwd(dout, True, None, frozen_record=True)
        assert torch.equal(df_f, df_u) and torch.equal(dx_f, dx_u), pattern
        # the small rows of the gradient record
        ds_u, df2_u, dx2_u = rec.chain_dsmall(dout, False)
        ds_c, df2_c, dx2_c = rec.chain_dsmall(dout, True)
        assert torch.equal(ds_c, ds_u), pattern
        assert torch.equal(df2_c, df_u) and torch.equal(dx2_c, dx_u) and torch.equal(df2_u, df_u)
        # dx += J . dfeat: one thread per listed sample against the tile lists
        dxj_u, dxj_c = dx_u.clone(), dx_c.clone()
        ops.hashgrid_dx_from_jac(jac, df_u, dxj_u, meta, rec.lay, tiles=tiles_u)
        ops.hashgrid_dx_from_jac(jac, df_c, dxj_c, meta, rec.lay, tiles=tiles_c)
        assert torch.equal(dxj_c, dxj_u), pattern
    assert ran >= (7 if M < 32 else 9)


def test_weight_gradients_refuse_a_list_outside_the_exchange_form(dev):
    """mipsf_decoder_wgrad16 takes a live-sample list in the transpose-read exchange form only (packed16 given, f16x3 /
    bf16x6), and not when the forward's record does not fit one buffer resource; the chain needs tile_live beside the
    list.  Every refusal comes before anything is launched."""
    M = 64
    rec = Record(dev, M, "aos", "f16x3")
    lib = _lib.lib()
    buf = torch.zeros(1024, device=dev)
    ll = torch.zeros(_lib.buffer_size(_lib.SIZE_DECODER_LIVE_LIST, M), dtype=torch.int32, device=dev)
    grads = [torch.zeros_like(w) for w in rec.ws]
    st = ops._decoder_struct(grads, _lib.DecoderGrads)

    def wgrad(**kw):
        args = dict(M=M, packed16=ops.dptr(rec.packed16), feat=ops.dptr(rec.feat), x=ops.dptr(rec.x), saved=ops.dptr(rec.saved),
                    dact=ops.dptr(buf), tile_live=None, grads=C.pointer(st), partial=ops.dptr(buf), feat_layout=rec.lay,
                    arithmetic=_lib.PREC["f16x3"], flags=0, packed16_floats=rec.packed16.numel(),
                    live_list=ops.dptr(ll, torch.int32))
        args.update(kw)
        return lib.mipsf_decoder_wgrad16(C.byref(_lib.DecoderWgrad16Args.new(**args)), ops.stream_ptr())

    for kw, msg in ((dict(packed16=None, packed16_floats=0), b"exchange form only"),
                    (dict(packed16=None, packed16_floats=0, arithmetic=_lib.PREC["bf16x3"]), b"exchange form only"),
                    (dict(M=3_000_000), b"less than 4 GiB")):      # 1536 B of record per sample: 4.6 GB
        assert wgrad(**kw) != 0 and msg in lib.mipsf_last_error(), (kw, lib.mipsf_last_error())
    with pytest.raises(RuntimeError, match="exchange form only"):
        _lib.check(wgrad(packed16=None, packed16_floats=0), "wgrad16")
    a = _lib.DecoderChain16Args.new(M=M, packed16=ops.dptr(rec.packed16), x=ops.dptr(rec.x), out=ops.dptr(rec.out),
                                    dout=ops.dptr(buf), saved=ops.dptr(rec.saved), dfeat=ops.dptr(buf), dx=ops.dptr(buf),
                                    dact=None, tile_live=None, feat_layout=rec.lay, flags=0,
                                    packed16_floats=rec.packed16.numel(), live_list=ops.dptr(ll, torch.int32))
    assert lib.mipsf_decoder_bwd_chain16(C.byref(a), ops.stream_ptr()) != 0 and b"tile_live" in lib.mipsf_last_error()
    # the plumbing keeps the tile lists where the list is not taken: the forms that read H1 from a full record, the fp32 kernel
    dout, _ = make_dout(M, "prefix", dev, 5)
    for kw in (dict(), dict(deterministic=True), dict(wgrad_precision="f32")):
        full = ops.decoder_fwd(None, rec.feat, rec.lay, rec.x, None, M, save=True, precision="f16x3", packed16=rec.packed16)
        tiles = ops.decoder_bwd(None, rec.feat, rec.lay, rec.x, None, full[0], dout, full[1], [torch.zeros_like(w) for w in rec.ws],
                                M, precision="f16x3", packed16=rec.packed16, return_tiles=True, **kw)[3]
        assert not isinstance(tiles, ops.LiveList)


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
def test_compacted_deterministic_gradients_do_not_depend_on_the_schedule(dev, prec):
    """Deterministic mode on the compact path: the list is ascending whatever order the pre-pass's blocks ran in, the chain writes a
    compact tile's record wherever it is processed, the weight-gradient kernel visits compact tiles in a fixed order and its
    records are summed in block order -- the same inputs must give the same bits: repeated, and beside a decoder forward that
    competes for the CUs on a second stream (the chain's tiles are then dealt to other waves)."""
    M = 70000
    rec = Record(dev, M, "level_major", prec)
    dout, _ = make_dout(M, "prefix", dev, 9)

    def run():
        grads = [torch.zeros_like(w) for w in rec.ws]
        df, dx, _, tiles = rec.bwd(dout, True, grads, deterministic=True)
        assert isinstance(tiles, ops.LiveList)
        return [df, dx] + grads

    ref = run()
    assert all(float(g.abs().max()) > 0 for g in ref)
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(run(), ref))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(3):
            ops.decoder_fwd(None, rec.feat, rec.lay, rec.x, None, M, False, precision=prec, packed16=rec.packed16)
    busy = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(busy, ref))


def test_captured_step_reads_the_compact_bounds_on_the_device(dev):
    """A JointEncoding training step captured once and replayed with two ray batches whose samples are live in different
    numbers: every replay must give the gradients of its own eager run -- the number of compact tiles is read by the kernels,
    not baked into the launches.  (Grid gradient: the scatter's atomics move the last bit run to run.)"""
    from oracle import path_cpu
    assert ops.COMPACT_LIVE and ops.SKIP_ZERO_TILES
    cfg = synth.config_plumbing()
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    torch.manual_seed(0)
    model = JointEncoding(cfg, bb, nf).to(dev).train()
    with torch.no_grad():
        model.embed_fn.params.copy_((torch.randn(model.embed_fn.params.shape) * 0.2).to(dev))
    model.accumulate_param_grads_in_place = True
    frame = synth.make_frame(cfg, seed=1)
    H, W = frame["depth"].shape
    batches = []
    for seed, scale in ((3, 1.0), (4, 0.6)):          # (nearer targets: the truncation band cuts the rays elsewhere)
        gen = torch.Generator().manual_seed(seed)
        idx = torch.randperm(H * W, generator=gen)[:256]
        ro, rd, rgb, d = synth.ray_batch(frame, idx, frame["c2w"])
        batches.append([t.to(dev).contiguous() for t in (ro, rd, rgb, d * scale, torch.rand(256, 16, generator=gen))])
    static = [t.clone() for t in batches[0]]
    params = [p for p in model.parameters() if p.numel()]

    def step():
        ret = model.forward(*static[:4], noise=static[4])
        path_cpu.total_loss(ret, cfg["training"]).backward()

    def zero():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()

    eager, live = [], []
    for b in batches:
        for s, t in zip(static, b):
            s.copy_(t)
        zero()
        step()
        torch.cuda.synchronize()
        assert ops._LAST_TILE_LIVE[2], "the step compacts"
        live.append(int(ops._LAST_TILE_LIVE[0][0].item()))
        eager.append([p.grad.clone() for p in params])
    assert live[0] != live[1] and min(live) > 0, live
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for s, t in zip(static, batches[0]):
            s.copy_(t)
        step()                                         # allocator warm-up on this stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            step()
        for k in (1, 0, 1):
            for s, t in zip(static, batches[k]):
                s.copy_(t)
            zero()
            graph.replay()
            torch.cuda.synchronize()
            assert int(ops._LAST_TILE_LIVE[0][0].item()) == live[k]
            for p, ref in zip(params, eager[k]):
                a, b = p.grad.double().cpu().numpy().ravel(), ref.double().cpu().numpy().ravel()
                bad = np.abs(a - b) > 1e-6 * (np.abs(b).max() + 1e-30)
                l2 = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
                assert bad.mean() <= 1e-4 and l2 <= 4e-6, f"replay of batch {k}: {bad.sum()} of {bad.size} off, L2 {l2:.2e}"
