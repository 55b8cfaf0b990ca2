"""GPU: the deterministic training mode (include/mipsf.h MIPSF_HG_DETERMINISTIC, MIPSF_WGRAD_DETERMINISTIC,
JointEncoding.deterministic).  The scatter equals the NumPy replay of its contract bit for bit (tests/det_replay.py) and does
not depend on the schedule; ordered live-tile lists make the decoder's weight gradients independent of the chain's list
order; mapping iterations and the two-room walk repeat bit for bit."""
import random

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops, synth
from oracle import tcnn_cpu

from . import det_replay

pytestmark = pytest.mark.gpu

FEAT_AOS, FEAT_LEVEL_MAJOR = _lib.FEAT_AOS, _lib.FEAT_LEVEL_MAJOR


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _metas(n_levels, log2_size, base_res, pls):
    meta = _lib.make_grid_meta(n_levels=n_levels, n_features=2, log2_hashmap_size=log2_size, base_resolution=base_res,
                               per_level_scale=pls)
    meta_o = tcnn_cpu.make_grid_meta(n_levels=n_levels, n_features=2, log2_hashmap_size=log2_size,
                                     base_resolution=base_res, per_level_scale=pls)
    assert list(meta.offsets[:n_levels + 1]) == meta_o.offsets
    assert [float(s) for s in meta.scales[:n_levels]] == meta_o.scales
    return meta, meta_o


def _points(rng, M, kind, meta_o):
    if kind == "inside":
        x = rng.uniform(0.0, 1.0, (M, 3))
    elif kind == "outside":
        x = rng.uniform(-2.0, 3.0, (M, 3))
    elif kind == "boundary":               # on cell faces / corners of random levels (the fma lands on an integer or next to it)
        lvl = rng.integers(0, meta_o.n_levels, M)
        s = np.array(meta_o.scales)[lvl]
        k = rng.integers(1, 12, (M, 3))
        x = (k - 0.5) / s[:, None]
        half = rng.random(M) < 0.3
        x[half, 1:] = rng.uniform(0.0, 1.0, (int(half.sum()), 2))
    elif kind == "crowded":                # one cell of the finest level
        x = rng.uniform(0.2, 0.8, 3)[None, :] + rng.uniform(0.0, 1e-4, (M, 3))
    else:                                  # "dup": a few points many times over
        base = rng.uniform(0.0, 1.0, (max(1, M // 16), 3))
        x = base[rng.integers(0, base.shape[0], M)]
    return det_replay.move_tiny(x.astype(np.float32), meta_o)


def _grads(rng, M, L, bad_row):
    g = (rng.standard_normal((M, L, 2)) * np.exp2(rng.uniform(-20.0, 20.0, (M, L, 2)))).astype(np.float32)
    g[rng.random((M, L)) < 0.2] = 0.0                         # dead pairs
    g[rng.random((M, L)) < 0.05, 1] = 0.0                     # one feature exactly zero
    g[int(M * 0.8):] = 0.0                                    # a dead tail
    if bad_row and M > 2:
        r = M // 3
        g[r, :, 0], g[r, :, 1] = np.inf, np.nan
    return g


SIZES = (10, 14, 16, 19, 21)
KINDS = ("inside", "outside", "boundary", "crowded", "dup")


def _cases():
    rng = np.random.default_rng(2024)
    out = []
    for k in range(26):
        M = 70000 if k == 25 else int(rng.integers(1, 5001))
        out.append(dict(seed=k, M=M, log2=SIZES[k % 5], kind=KINDS[(k // 5) % 5], layout=(FEAT_AOS, FEAT_LEVEL_MAJOR)[k % 2],
                        zero=(k // 2) % 2 == 0, bad=k % 7 == 3))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c['seed']}-M{c['M']}-T{c['log2']}-{c['kind']}")
def test_scatter_equals_the_replay_bit_for_bit(dev, case):
    rng = np.random.default_rng(case["seed"])
    L = 16 if case["log2"] >= 16 else 8
    meta, meta_o = _metas(L, case["log2"], 16, 1.38 if L == 16 else 1.6)
    M = case["M"]
    x = _points(rng, M, case["kind"], meta_o)
    g = _grads(rng, M, L, case["bad"])
    n_params = meta_o.n_params
    base = None if case["zero"] else rng.standard_normal(n_params).astype(np.float32)
    want = det_replay.det_backward(x, g, meta_o, dparams_in=base, zero=case["zero"])
    dout = g.reshape(M, L * 2) if case["layout"] == FEAT_AOS else np.ascontiguousarray(g.transpose(1, 0, 2))
    xd, dd = torch.from_numpy(x).to(dev), torch.from_numpy(dout).to(dev)
    params = torch.zeros(n_params, device=dev)
    dp = torch.zeros(n_params, device=dev) if case["zero"] else torch.from_numpy(base).to(dev)
    ops.hashgrid_bwd(xd, params, dd, dp, meta, case["layout"], None, dparams_zero=case["zero"], deterministic=True)
    got = dp.cpu().numpy()
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w)
    ok = ~nan_w
    bad = np.nonzero(got[ok].view(np.uint32) != want[ok].view(np.uint32))[0]
    assert bad.size == 0, (bad.size, got[ok][bad[:5]], want[ok][bad[:5]])
    assert np.array_equal(got == 0, want == 0)
    if not case["bad"] and case["zero"]:
        fast = torch.zeros(n_params, device=dev)
        ops.hashgrid_bwd(xd, params, dd, fast, meta, case["layout"], None, dparams_zero=True)
        f = fast.cpu().numpy()
        scale = max(float(np.abs(f).max()), 1e-30)
        assert float(np.abs(got - f).max()) <= 2e-5 * scale


def test_scatter_dx_is_the_fast_paths(dev):
    rng = np.random.default_rng(11)
    meta, meta_o = _metas(16, 16, 16, 1.38)
    M = 3000
    x = torch.from_numpy(_points(rng, M, "inside", meta_o)).to(dev)
    g = torch.from_numpy(_grads(rng, M, 16, False).reshape(M, 32)).to(dev)
    params = (torch.randn(meta_o.n_params) * 0.1).to(dev)
    outs = []
    for det in (False, True):
        dp, dx = torch.zeros_like(params), torch.zeros(M, 3, device=dev)
        ops.hashgrid_bwd(x, params, g, dp, meta, FEAT_AOS, dx, dparams_zero=True, deterministic=det)
        outs.append(dx)
    assert torch.equal(outs[0], outs[1])


def test_refusals(dev):
    meta, _ = _metas(16, 19, 16, 1.38)
    x = torch.rand(8, 3, device=dev)
    dout = torch.randn(8, 32, device=dev)
    dp = torch.zeros(meta.n_params, device=dev)
    scratch = torch.empty(_lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, 8, 0, 0, meta), device=dev)
    a = _lib.HashgridBwdArgs.new(M=8, x=ops.dptr(x), params=ops.dptr(dp), dout=ops.dptr(dout), dparams=ops.dptr(dp),
                                 meta=_lib.C.pointer(meta), feat_layout=FEAT_AOS, scratch=ops.dptr(scratch),
                                 flags=_lib.HG_DETERMINISTIC | _lib.HG_ROUTED)
    with pytest.raises(RuntimeError, match="ROUTED"):
        _lib.check(_lib.lib().mipsf_hashgrid_bwd(_lib.C.byref(a), ops.stream_ptr()), "hashgrid_bwd")
    a.flags, a.M = _lib.HG_DETERMINISTIC, (1 << 24) + 1          # above the limit: refused before anything is read
    with pytest.raises(RuntimeError, match="limit"):
        _lib.check(_lib.lib().mipsf_hashgrid_bwd(_lib.C.byref(a), ops.stream_ptr()), "hashgrid_bwd")


# ------------------------------------------------------------------ headline batch
def _headline(dev, hash_size=19):
    from mipsfusion_amd.model import JointEncoding
    cfg = synth.config_headline()
    cfg["grid"]["hash_size"] = hash_size
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    torch.manual_seed(0)
    m = JointEncoding(cfg, bb, nf).to(dev).train()
    with torch.no_grad():
        m.embed_fn.params.copy_((torch.randn(m.embed_fn.params.shape) * 0.2).to(dev))
    frame = synth.make_frame(cfg, seed=0)
    H, W = frame["depth"].shape
    random.seed(0)
    idx = torch.tensor(random.sample(range(H * W), 4096))
    batch = [t.to(dev) for t in synth.ray_batch(frame, idx, frame["c2w"])]
    return cfg, m, batch


def _headline_samples(dev):
    """The points and the feature gradient of one mapping iteration at config 2 (4096 rays x 64 samples, 2^19 table)."""
    cfg, m, (ro, rd, rgb, d) = _headline(dev)
    noise = torch.rand(4096, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    keep = {}
    orig = ops.hashgrid_bwd

    def spy(x, params, dout, dparams, meta, layout=FEAT_AOS, dx=None, routed=None, dparams_zero=False, deterministic=False):
        keep.update(x=x.clone(), dout=dout.clone(), layout=layout)
        return orig(x, params, dout, dparams, meta, layout, dx, routed=routed, dparams_zero=dparams_zero,
                    deterministic=deterministic)
    ops.hashgrid_bwd = spy
    try:
        ret = m.forward(ro, rd, rgb, d, noise=noise)
        from oracle import path_cpu
        path_cpu.total_loss(ret, cfg["training"]).backward()
    finally:
        ops.hashgrid_bwd = orig
    torch.cuda.synchronize()
    return m, keep


def test_scatter_does_not_depend_on_the_schedule(dev):
    m, k = _headline_samples(dev)
    x, dout, layout, meta = k["x"], k["dout"], k["layout"], m.embed_fn.meta
    assert x.shape[0] == 262144 and meta.log2_hashmap_size == 19
    params = m.embed_fn.params.detach()

    def run(**kw):
        dp = torch.zeros_like(params)
        ops.hashgrid_bwd(x, params, dout, dp, meta, layout, None, dparams_zero=True, deterministic=True, **kw)
        return dp

    ref = run()
    assert float(ref.abs().max()) > 0
    for _ in range(2):
        assert torch.equal(run(), ref)
    # a kept counter block (the fast path's) is ignored by this path: hand one in through the argument block
    dp = torch.zeros_like(params)
    n = _lib.buffer_size(_lib.SIZE_HASHGRID_DET_SCRATCH, x.shape[0], 0, 0, meta)
    scratch = torch.empty(n, device=dev)
    counters = torch.full((_lib.buffer_size(_lib.SIZE_HASHGRID_COUNTER_WORDS, meta=meta),), 7, dtype=torch.int32, device=dev)
    a = _lib.HashgridBwdArgs.new(M=x.shape[0], x=ops.dptr(x), params=ops.dptr(params), dout=ops.dptr(dout), dparams=ops.dptr(dp),
                                 meta=_lib.C.pointer(meta), feat_layout=layout, scratch=ops.dptr(scratch),
                                 counters=ops.dptr(counters, torch.int32), flags=_lib.HG_DETERMINISTIC | _lib.HG_DPARAMS_ZERO)
    _lib.check(_lib.lib().mipsf_hashgrid_bwd(_lib.C.byref(a), ops.stream_ptr()), "hashgrid_bwd")
    assert torch.equal(dp, ref)
    # next to a decoder kernel on a second stream
    side = torch.cuda.Stream()
    feat = ops.hashgrid_fwd(x, params, meta, FEAT_LEVEL_MAJOR)
    w = m.decoder.ordered_parameters()
    p16 = ops.decoder_pack16(w, precision="bf16x6")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(3):
            ops.decoder_fwd(None, feat, FEAT_LEVEL_MAJOR, x, None, x.shape[0], False, precision="bf16x6", packed16=p16)
    busy = run()
    torch.cuda.synchronize()
    assert torch.equal(busy, ref)
    # replayed from a captured graph
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = torch.zeros_like(params)
        ops.hashgrid_bwd(x, params, dout, out, meta, layout, None, dparams_zero=True, deterministic=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out.zero_()
            ops.hashgrid_bwd(x, params, dout, out, meta, layout, None, dparams_zero=True, deterministic=True)
        out.fill_(1.0)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    # `routed=` given: waited for, its scratch unused
    routed = ops.hashgrid_route_ahead(x, meta)
    assert torch.equal(run(routed=routed), ref)


# ------------------------------------------------------------------ ordered tile lists
TL_HEADER = 512


def _tl_cap(n_tiles):
    return ((n_tiles + 63) // 64) * 8 + 8


def _lists(tl, M):
    n_tiles = (M + 31) // 32
    cap = _tl_cap(n_tiles)
    t = tl.cpu().numpy().view(np.uint32)
    return [t[TL_HEADER + q * cap: TL_HEADER + q * cap + t[64 * q + 32]].copy() for q in range(8)], t[:TL_HEADER].copy()


def test_ordered_tile_lists_fix_the_weight_gradients(dev):
    cfg, m, _ = _headline(dev)
    M = 262144
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(M, 3, generator=gen).to(dev)
    meta = m.embed_fn.meta
    params = m.embed_fn.params.detach()
    feat = ops.hashgrid_fwd(x, params, meta, FEAT_LEVEL_MAJOR)
    weights = m.decoder.ordered_parameters()
    p16 = ops.decoder_pack16(weights, precision="bf16x6")
    out, saved = ops.decoder_fwd(None, feat, FEAT_LEVEL_MAJOR, x, None, M, True, precision="bf16x6", packed16=p16)
    dout = torch.randn(M // 64, 64, 10, generator=gen)
    dout[:, 32:] = 0.0                                         # dead ray tails: every second 32-sample tile
    dout[::5, :32] = 0.0                                       # and some whole rays
    dout = dout.reshape(M, 10).to(dev)
    dact = torch.empty(_lib.buffer_size(_lib.SIZE_DECODER_DACT, M), device=dev)
    dfeat, dxx = torch.empty_like(feat), torch.empty(M, 3, device=dev)
    tl = torch.empty(_lib.buffer_size(_lib.SIZE_DECODER_TILE_WORDS, M), dtype=torch.int32, device=dev)
    a = _lib.DecoderChain16Args.new(M=M, packed16=ops.dptr(p16), x=ops.dptr(x), out=ops.dptr(out), dout=ops.dptr(dout),
                                    saved=ops.dptr(saved), dfeat=ops.dptr(dfeat), dx=ops.dptr(dxx), dact=ops.dptr(dact),
                                    tile_live=ops.dptr(tl, torch.int32), feat_layout=FEAT_LEVEL_MAJOR, flags=4,
                                    packed16_floats=p16.numel())
    _lib.check(_lib.lib().mipsf_decoder_bwd_chain16(_lib.C.byref(a), ops.stream_ptr()), "chain16")

    def wgrad(tiles, order):
        grads = [torch.zeros_like(w) for w in weights]
        st = ops._decoder_struct(grads, _lib.DecoderGrads)
        partial = torch.zeros(_lib.buffer_size(_lib.SIZE_DECODER_WGRAD_PARTIAL), device=dev)     # (records not written stay 0)
        b = _lib.DecoderWgrad16Args.new(M=M, packed16=None, feat=ops.dptr(feat), x=ops.dptr(x), saved=ops.dptr(saved),
                                        dact=ops.dptr(dact), tile_live=ops.dptr(tiles, torch.int32), grads=_lib.C.pointer(st),
                                        partial=ops.dptr(partial), feat_layout=FEAT_LEVEL_MAJOR, arithmetic=_lib.PREC["bf16x6"],
                                        flags=_lib.WGRAD_DETERMINISTIC if order else 0, packed16_floats=0)
        _lib.check(_lib.lib().mipsf_decoder_wgrad16(_lib.C.byref(b), ops.stream_ptr()), "wgrad16")
        return grads, partial

    raw_lists, hdr = _lists(tl, M)
    assert sum(len(li) for li in raw_lists) > 0
    ordered = tl.clone()
    g_ref, p_ref = wgrad(ordered, True)
    o_lists, o_hdr = _lists(ordered, M)
    assert np.array_equal(o_hdr[32::64], hdr[32::64])                 # counts unchanged
    for q in range(8):
        assert np.array_equal(o_lists[q], np.sort(raw_lists[q])), q  # the same members, ascending
        assert np.all((o_lists[q] >> 3) % 8 == q)
    # shuffle every list's used prefix in place
    shuf = tl.clone()
    cap = _tl_cap((M + 31) // 32)
    rng = np.random.default_rng(5)
    host = shuf.cpu().numpy().view(np.uint32)
    for q in range(8):
        lo = TL_HEADER + q * cap
        host[lo:lo + len(raw_lists[q])] = rng.permutation(raw_lists[q])
    shuf = torch.from_numpy(host.view(np.int32).copy()).to(dev)
    g_unordered, p_unordered = wgrad(shuf.clone(), False)
    g_again, p_again = wgrad(shuf, True)
    s_lists, s_hdr = _lists(shuf, M)
    assert np.array_equal(s_hdr[32::64], hdr[32::64]) and all(np.array_equal(a_, b_) for a_, b_ in zip(s_lists, o_lists))
    assert torch.equal(p_again, p_ref)                                   # the per-workgroup records
    for a_, b_ in zip(g_again, g_ref):
        assert torch.equal(a_, b_)
    # Is the ordering needed?  The kernel deals list positions round-robin to its workgroups: the per-workgroup records of
    # shuffled lists (before any reduce) show whether another list order gives another association of the sums.
    p_diff = int((p_unordered != p_ref).sum())
    g_diff = sum(int(not torch.equal(a_, b_)) for a_, b_ in zip(g_unordered, g_ref))
    print(f"shuffled lists, no ordering: {p_diff} differing words in the per-workgroup records, "
          f"{g_diff} of {len(g_ref)} gradient tensors differ")


# ------------------------------------------------------------------ mapping end to end
def _mapping_run(dev, graphed, flag=True, iters=20, use_torch_flag=False):
    from mipsfusion_amd.graph import GraphedSteps
    from mipsfusion_amd.helper_functions.geometry_helper import quaternion_to_matrix
    from mipsfusion_amd.optim import FusedAdam
    from oracle import path_cpu
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        if use_torch_flag:
            torch.use_deterministic_algorithms(True)
        with torch.cuda.stream(side):
            cfg, m, (ro, rd, rgb, d) = _headline(dev, hash_size=19)
            m.deterministic = None if use_torch_flag else flag
            m.accumulate_param_grads_in_place = True
            rot = torch.nn.Parameter(torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev))
            trans = torch.nn.Parameter(torch.zeros(1, 3, device=dev))
            opt = FusedAdam([{"params": m.decoder.parameters(), "weight_decay": 1e-6, "lr": 0.01},
                             {"params": m.embed_fn.parameters(), "eps": 1e-15, "lr": 0.01}], betas=(0.9, 0.99), capturable=True)
            pose_opt = FusedAdam([{"params": [rot, trans], "lr": 1e-3}], betas=(0.9, 0.99), capturable=True)
            noise = torch.rand(4096, 64, generator=torch.Generator().manual_seed(2)).to(dev)
            losses = torch.zeros(iters, device=dev)

            def step():
                R = quaternion_to_matrix(rot)[0]               # (capturable: no host tensors)
                rays_d = (rd[:, None, :] * R[None]).sum(-1)
                rays_o = ro + trans
                ret = m.forward(rays_o, rays_d, rgb, d, noise=noise)
                loss = path_cpu.total_loss(ret, cfg["training"])
                loss.backward()
                opt.step(zero_grad=True)
                pose_opt.step(zero_grad=True)
                return loss

            slot = torch.zeros((), device=dev)

            def graph_step(_k=0):
                slot.copy_(step())

            for i in range(2):                           # the eager warm-up of the allocator / lazy initialisation
                graph_step()
                losses[i].copy_(slot)
            if graphed:
                gs = GraphedSteps(graph_step, 1, warmup=0, stream=side)
                for i in range(2, iters):
                    gs.replay()
                    losses[i].copy_(slot)
            else:
                for i in range(2, iters):
                    graph_step()
                    losses[i].copy_(slot)
            torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(prev)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    moments = [t.clone() for g in opt.state.values() for t in g.values() if torch.is_tensor(t)]
    return state, moments, rot.detach().clone(), trans.detach().clone(), losses.clone()


def _same_run(a, b):
    sa, ma, ra, ta, la = a
    sb, mb, rb, tb, lb = b
    assert torch.equal(la, lb), (la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert len(ma) == len(mb) and all(torch.equal(x, y) for x, y in zip(ma, mb))
    assert torch.equal(ra, rb) and torch.equal(ta, tb)


def test_mapping_iterations_repeat_bit_for_bit(dev):
    """config 2 (4096 x 64, 2^19 table), 20 iterations of map + pose with FusedAdam: two eager runs, a graphed run, and
    torch.use_deterministic_algorithms(True) with deterministic = None give the same bits."""
    eager = _mapping_run(dev, graphed=False)
    assert bool(torch.isfinite(eager[4]).all()) and float(eager[4][-1]) < float(eager[4][0])
    _same_run(eager, _mapping_run(dev, graphed=False))
    _same_run(eager, _mapping_run(dev, graphed=True))
    _same_run(eager, _mapping_run(dev, graphed=False, use_torch_flag=True))


def test_one_iteration_stage_by_stage(dev):
    """Every intermediate of one deterministic iteration, twice: samples, features, decoder outputs, loss terms, the
    feature and pre-activation gradients (through the ops the backward calls), weight / grid / pose gradients."""
    from oracle import path_cpu
    cfg, m, (ro, rd, rgb, d) = _headline(dev)
    m.deterministic = True
    noise = torch.rand(4096, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    runs = []
    for _ in range(2):
        seen = {}
        orig_bwd, orig_dec = ops.hashgrid_bwd, ops.decoder_bwd

        def spy_bwd(x, params, dout, dparams, *a, **kw):
            seen["xn"], seen["dfeat"] = x.clone(), dout.clone()
            orig_bwd(x, params, dout, dparams, *a, **kw)
            seen["dgrid"] = dparams.clone()

        def spy_dec(packed, feat, layout, x, embed_pos, out, dout, saved, grads, M, **kw):
            seen["feat"], seen["raw"], seen["draw"] = feat.clone(), out.clone(), dout.clone()
            r = orig_dec(packed, feat, layout, x, embed_pos, out, dout, saved, grads, M, **kw)
            seen["dfeat_chain"] = r[0].clone()
            seen["wgrads"] = [g.clone() for g in grads]
            return r
        ops.hashgrid_bwd, ops.decoder_bwd = spy_bwd, spy_dec
        try:
            rot = torch.nn.Parameter(torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev))
            trans = torch.nn.Parameter(torch.zeros(1, 3, device=dev))
            from mipsfusion_amd.helper_functions.geometry_helper import qt_to_transform_matrix
            T = qt_to_transform_matrix(rot, trans)[0]
            ret = m.forward(ro, (rd[:, None, :] * T[None, :3, :3]).sum(-1), rgb, d, noise=noise)
            loss = path_cpu.total_loss(ret, cfg["training"])
            loss.backward()
        finally:
            ops.hashgrid_bwd, ops.decoder_bwd = orig_bwd, orig_dec
        seen.update({k: ret[k].detach().clone() for k in ("z_vals", "depth", "rgb", "sdf_loss", "fs_loss", "rgb_loss",
                                                          "depth_loss") if k in ret})
        seen["grads"] = [p.grad.clone() for p in m.parameters() if p.grad is not None]
        seen["pose"] = [rot.grad.clone(), trans.grad.clone()]
        m.zero_grad(set_to_none=True)
        runs.append(seen)
    a, b = runs
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, list):
            assert len(va) == len(vb) and all(torch.equal(x, y) for x, y in zip(va, vb)), k
        else:
            assert torch.equal(va, vb), k


def test_two_room_walk_repeats_pose_for_pose(dev):
    """The sequence of test_graphed_two_room_sequence_tracks_through_both_switches with deterministic=True, twice: the
    same trajectory pose for pose, inside the existing gates."""
    from mipsfusion_amd import sequence
    from mipsfusion_amd.graph import work_stream
    from .test_gpu_sequence import _small_two_room_cfg
    runs = []
    for _ in range(2):
        cfg = _small_two_room_cfg(quick=False)
        random.seed(0), np.random.seed(0), torch.manual_seed(0)
        gt, frames, schedule = synth.two_room_sequence(cfg, 300, kf_every=15)
        prev = torch.cuda.current_stream(dev)
        try:
            seq = sequence.GraphedSequence(cfg, dev, frames, kf_every=15, sampler="device", stream=work_stream(dev),
                                           schedule=schedule, deterministic=True)
            res = seq.run(gt)
        finally:
            torch.cuda.set_stream(prev)
        out = sequence.summarise(res, gt, cfg, "graphs")
        print({k: out[k] for k in ("ms_per_frame_mean", "ms_per_frame_median", "ate_rmse_m", "ate_max_m", "switch_frames")})
        assert sorted(out["switch_frames"]) == sorted(schedule)
        assert out["ate_rmse_m"] < 0.05 and out["ate_max_m"] < 0.30
        runs.append([e.cpu().clone() for e in res["est"]])
    assert len(runs[0]) == len(runs[1])
    for k, (p, q) in enumerate(zip(*runs)):
        assert torch.equal(p, q), k
