"""GPU (-m gpu): the ray mask of the grid's d x path (include/mipsf_compact.h, RAY MASK).

A ray of a pose that is not optimised needs no gradient of its points: `forward_from_table` hands the per-ray mask of
gather_pose_place_kernel to the grid forward (no Jacobian stored for a masked ray) and to hashgrid_dx_jac_kernel (d x = +0 for
its samples, nothing loaded).  Held here, bit for bit:

  kernels   features and the Jacobian of unmasked rays as without a mask; the Jacobian words of masked rays stay unwritten (a
            NaN poison survives there and reaches no output); d x rows of masked rays exactly +0.0f whatever the decoder's
            backward left there, rows of the others as without a mask; no mask = the unmasked entry points; S = 64 (a wave is
            a ray) and S = 33 (the test per lane); the whole batch, the live-tile lists and the live-sample list
  model     `forward_from_table` + backward with and without the mask, in deterministic mode (fixed-order sums: equal inputs
            give equal bits): d feat, the table gradient, the ten weight gradients, rot.grad and trans.grad identical; d x of
            masked rays +0.0f, of the others identical; with the live-sample list and with MIPSF_NO_COMPACT's live-tile lists

Owners: all fixed, none fixed, alternating, only the last ray fixed."""
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops, synth
from mipsfusion_amd._lib import FEAT_AOS, FEAT_LEVEL_MAJOR, dptr, stream_ptr
from mipsfusion_amd.model import JointEncoding

pytestmark = pytest.mark.gpu
PLS = float(2.0 ** (math.log2(256 / 16) / 15))
SHAPES = [(8, 64), (5, 33)]
OWNERS = ["all_fixed", "none_fixed", "alternating", "last_fixed"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def fixed_rays(pattern, N):
    """bool [N]: the ray belongs to a fixed pose"""
    f = np.zeros(N, bool)
    if pattern == "all_fixed":
        f[:] = True
    elif pattern == "alternating":
        f[::2] = True
    elif pattern == "last_fixed":
        f[-1] = True
    else:
        assert pattern == "none_fixed"
    return f


def plus_zero(t):
    """every word is +0.0f (not -0.0f)"""
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ----------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("lname,layout", [("aos", FEAT_AOS), ("level_major", FEAT_LEVEL_MAJOR)])
@pytest.mark.parametrize("pattern", OWNERS)
@pytest.mark.parametrize("N,S", SHAPES)
def test_masked_kernels(dev, N, S, pattern, lname, layout):
    torch.manual_seed(N * 100 + S)
    M = N * S
    meta = _lib.make_grid_meta(16, 2, 14, 16, PLS)
    x = torch.rand(M, 3, device=dev)
    params = torch.randn(meta.n_params, device=dev) * 0.1
    fixed = torch.from_numpy(fixed_rays(pattern, N)).to(dev)
    mask = (~fixed).to(torch.int32)
    masked_s = fixed.repeat_interleave(S)                                  # [M] samples of masked rays
    lib = _lib.lib()

    feat0, jac0 = ops.hashgrid_fwd(x, params, meta, layout, with_jac=True)
    feat1 = torch.empty_like(feat0)
    jac1 = torch.full_like(jac0, float("nan"))                             # poison: a masked ray's words must stay unwritten
    _lib.check(lib.mipsf_hashgrid_fwd_masked(dptr(x), dptr(params), dptr(feat1), dptr(jac1), dptr(mask, torch.int32), S, M,
                                             _lib.C.byref(meta), layout, stream_ptr()), "hashgrid_fwd_masked")
    assert torch.equal(feat1, feat0), "features changed under the mask"
    assert torch.equal(jac1[:, :, ~masked_s], jac0[:, :, ~masked_s]), "Jacobian of unmasked rays"
    assert bool(torch.isnan(jac1[:, :, masked_s]).all()), "the Jacobian of a masked ray was written"
    feat2, jac2 = ops.hashgrid_fwd(x, params, meta, layout, with_jac=True, ray_mask=None)
    assert torch.equal(feat2, feat0) and torch.equal(jac2, jac0)
    feat3 = torch.empty_like(feat0)
    jac3 = torch.empty_like(jac0)
    _lib.check(lib.mipsf_hashgrid_fwd_masked(dptr(x), dptr(params), dptr(feat3), dptr(jac3), None, 0, M, _lib.C.byref(meta),
                                             layout, stream_ptr()), "hashgrid_fwd_masked (no mask)")
    assert torch.equal(feat3, feat0) and torch.equal(jac3, jac0), "no mask = the unmasked forward"

    dfeat = torch.randn_like(feat0)
    live = torch.rand(M, device=dev) < 0.6
    live[0] = True
    if layout == FEAT_AOS:
        dfeat[~live] = 0
    else:
        dfeat[:, ~live] = 0
    chain = torch.randn(M, 3, device=dev)                                  # what the decoder's backward left in d x
    chain[~live] = 0
    want = chain.clone()
    ops.hashgrid_dx_from_jac(jac0, dfeat, want, meta, layout)
    got = chain.clone()
    ops.hashgrid_dx_from_jac(jac1, dfeat, got, meta, layout, ray_mask=mask)
    assert torch.equal(got[~masked_s], want[~masked_s]), "d x of unmasked rays"
    assert plus_zero(got[masked_s]), "d x of a masked ray is not +0.0f"
    assert not bool(torch.isnan(got).any()), "a poisoned Jacobian word was read"
    # the live-sample list: only listed samples are visited; the dead ones hold the zeros the compaction wrote
    idx = torch.nonzero(live).flatten().to(torch.int32)
    n_live = idx.numel()
    buf = torch.full((_lib.buffer_size(_lib.SIZE_DECODER_LIVE_LIST, M),), -1, dtype=torch.int32, device=dev)
    buf[0], buf[1] = n_live, (n_live + 31) // 32
    buf[16:16 + n_live] = idx
    want_l = chain.clone()
    ops.hashgrid_dx_from_jac(jac0, dfeat, want_l, meta, layout, tiles=ops.LiveList(buf))
    assert torch.equal(want_l, want), "list mode = whole batch when the unlisted samples are dead"
    got_l = chain.clone()
    ops.hashgrid_dx_from_jac(jac1, dfeat, got_l, meta, layout, tiles=ops.LiveList(buf), ray_mask=mask)
    assert torch.equal(got_l, got), "masked d x, list mode"
    got_n = chain.clone()
    _lib.check(lib.mipsf_hashgrid_dx_from_jac_masked(dptr(jac0), dptr(dfeat), dptr(got_n), None, dptr(buf, torch.int32), None, 0,
                                                     M, _lib.C.byref(meta), layout, stream_ptr()), "dx masked (no mask)")
    assert torch.equal(got_n, want), "no mask = the unmasked d x"


def test_mask_needs_whole_rays(dev):
    meta = _lib.make_grid_meta(16, 2, 14, 16, PLS)
    x = torch.rand(10, 3, device=dev)
    params = torch.zeros(meta.n_params, device=dev)
    with pytest.raises(RuntimeError, match="whole rays"):
        ops.hashgrid_fwd(x, params, meta, FEAT_AOS, with_jac=True, ray_mask=torch.ones(3, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------------------------------- model
def run_model(m, cfg, table, rows, rot0, trans0, fixed, owner, noise, masked):
    from mipsfusion_amd.helper_functions.utils import get_loss_from_ret
    seen = {}
    keep = ops.hashgrid_dx_from_jac

    def spy(jac, dout, dx, *a, **k):
        keep(jac, dout, dx, *a, **k)
        seen["dfeat"], seen["dx"], seen["mask"] = dout.clone(), dx.clone(), k.get("ray_mask")

    rot, trans = rot0.clone().requires_grad_(True), trans0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    m.mask_fixed_rays = masked
    ops.hashgrid_dx_from_jac = spy
    try:
        ret = m.forward_from_table(table, rows, rot, trans, fixed, owner, noise)
        loss = get_loss_from_ret(ret, cfg["training"])
        loss.backward()
    finally:
        ops.hashgrid_dx_from_jac = keep
        m.mask_fixed_rays = True
    assert (seen["mask"] is not None) == masked
    grads = [m.embed_fn.params.grad.clone()] + [p.grad.clone() for p in m.decoder.ordered_parameters()]
    return dict(loss=loss.detach(), rot=rot.grad.clone(), trans=trans.grad.clone(), grads=grads, **seen)


@pytest.mark.parametrize("compact", [True, False], ids=["list", "tiles"])
@pytest.mark.parametrize("pattern", OWNERS)
@pytest.mark.parametrize("N,S", SHAPES)
def test_forward_from_table_with_and_without_the_mask(dev, N, S, pattern, compact):
    torch.manual_seed(7)
    cfg = synth.config_headline()
    cfg["grid"]["hash_size"] = 14
    if S != cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"]:
        cfg["training"]["n_samples_d"], cfg["training"]["n_range_d"] = S - 21, 21
    assert cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"] == S
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    m = JointEncoding(cfg, bb, nf).to(dev).train()
    m.deterministic = True                       # fixed-order sums: two runs on equal inputs give equal bits
    with torch.no_grad():
        m.embed_fn.params.copy_(torch.randn_like(m.embed_fn.params) * 0.2)
    frame = synth.make_frame(cfg, seed=5)
    table = torch.cat([frame["direction"], frame["rgb"], frame["depth"][..., None]], -1).reshape(-1, 7)[:50000].contiguous().to(dev)
    F, K = 2, 3
    c2w = synth.default_pose(cfg)
    fixed = c2w[None].repeat(F, 1, 1).to(dev)
    from mipsfusion_amd.helper_functions.geometry_helper import matrix_to_quaternion
    rot0 = matrix_to_quaternion(c2w[None, :3, :3])[0][None].repeat(K, 1).to(dev) + 0.01 * torch.randn(K, 4, device=dev)
    trans0 = c2w[None, :3, 3].repeat(K, 1).to(dev) + 0.02 * torch.randn(K, 3, device=dev)
    rows = torch.randint(0, 50000, (N,), device=dev)
    fx = fixed_rays(pattern, N)
    owner = torch.from_numpy(np.where(fx, np.arange(N) % F, F + np.arange(N) % K)).to(dev)
    noise = torch.rand(N, S, device=dev)
    keep = ops.COMPACT_LIVE
    ops.COMPACT_LIVE = compact
    try:
        a = run_model(m, cfg, table, rows, rot0, trans0, fixed, owner, noise, masked=False)
        b = run_model(m, cfg, table, rows, rot0, trans0, fixed, owner, noise, masked=True)
    finally:
        ops.COMPACT_LIVE = keep
    assert torch.isfinite(a["loss"]) and torch.equal(a["loss"], b["loss"])
    assert torch.equal(a["dfeat"], b["dfeat"]), "d feat"
    for k, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(ga, gb), "table gradient" if k == 0 else f"weight gradient {k - 1}"
    assert len(a["grads"]) == 1 + len(ops.DECODER_PARAM_ORDER) == 11
    assert torch.equal(a["rot"], b["rot"]) and torch.equal(a["trans"], b["trans"]), "pose gradients"
    ms = torch.from_numpy(fx).to(dev).repeat_interleave(S)
    assert torch.equal(a["dx"][~ms], b["dx"][~ms]), "d x of the rays of optimised poses"
    assert plus_zero(b["dx"][ms]), "d x of a fixed pose's ray is not +0.0f"
    if fx.any() and not fx.all():
        assert bool(a["dx"][ms].any()), "the unmasked run does form d x for those rays (the test would be vacuous)"
