"""GPU (-m gpu): the head and the tail of the training step against INDEPENDENT answers (tests/step_cpu.py; tests/test_step_cpu.py
holds the inputs and the yardsticks to their conditions):

  placement   sample_rays_kernel and gather_pose_place_kernel (place_ray, csrc/render.hip): z_vals, xn, counts, wants_dx and the
              gathered rows BIT FOR BIT against oracle/path_cpu.py's place_samples / ray_points / normalise_points in the formats the
              reference uses (fp32 placement and points, float64 normalisation, one cast) and the mask rule of the losses; the two
              entry points bit for bit against each other.  The unit is built without contraction, the operations and their order
              are the reference's: equality is the standard, not closeness.
  pose path   pose_rays_fwd_kernel (both forms), pose_rays_bwd_kernel, place_pose_bwd_kernel, pose_chain, pose_block_finish
              (csrc/pose.hip, csrc/pose_dev.h, csrc/render.hip) against qt_to_transform_matrix -> gather -> sum(d_cam * R, -1) (->
              ray_points -> normalise_points / norm_factor) with autograd in float64.  Per ray (rays_d) and per POSE and group (d
              quaternion, d translation), normalised by that row's largest float64 magnitude; working gate max(8 e32, 64 * 2^-24)
              under the ceilings 1e-4 (values) and 5e-4 (gradients), e32 being the same chain in fp32.  No outlier allowance, no
              further term.  A pose without a ray has a gradient of exactly 0.0; accumulate = 1 twice is the single result added to
              itself; the ticket word is zero after every call.
  frequency   freq_fwd/bwd_kernel against sine and cosine in float64 of tcnn's fp32 argument (e32: torch's fp32 sine and cosine);
              normalise_kernel and normalise_bwd_kernel bit for bit.
  Adam        adam_kernel, adam_multi_kernel, adam_small_kernel, adam_all_kernel: ONE step from the state the device holds against
              path_cpu.adam_reference in float64, element by element under the derived bound step_cpu.adam_bound (new p, exp_avg and
              exp_avg_sq); the step-dependent scalars within one fp32 ulp; guard words, tickets, alignment, zero_grad, path equality.

Measured on an MI355X (worst group per form, kernel error | e32): see DESIGN.md, "The placement, pose and optimiser kernels against
float64"."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import dptr, lib, stream_ptr

from . import step_cpu as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def report(form, tag, name, err, e32):
    print(f"\n  fp64 | {form} | {tag} | {name} | kernel {err:.2e} | e32 {e32:.2e}", end="")


def differing(a, b):
    """number of words in which two fp32 (or int32) tensors differ; shapes must agree"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(torch.int32) != b.view(torch.int32)).sum()) if a.numel() else 0


def assert_same_bits(form, tag, name, a, b):
    n = differing(a, b)
    if n:
        a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
        i = int((a.view(torch.int32) != b.view(torch.int32)).nonzero()[0])
        raise AssertionError(f"{form} {tag}: {name} differs in {n} of {a.numel()} words; first at {i}: {a[i].item()!r} against {b[i].item()!r}")


def render_cfg(cfg, n_uniform, n_near):
    return ops.make_render_cfg(cfg, cfg["mapping"]["bound"], cfg["mapping"]["localMLP_max_len"], n_uniform, n_near, 0.0)


def check_groups(form, tag, a, ref, y32, groups, ceiling):
    """a: the kernel's rows; ref / y32: the float64 answer and the fp32 yardstick.  Per row and group under the working gate; where
    float64 is exactly 0 the kernel is == 0.0"""
    a = a.detach().cpu()
    assert not bool(torch.isnan(a).any()), f"{form} {tag}: NaN"
    zero = ref == 0
    assert bool((a[zero] == 0).all()), f"{form} {tag}: {int((a[zero] != 0).sum())} entries are not 0.0 where the float64 answer is exactly 0"
    err, e32 = P.group_errors(a, ref, groups), P.group_errors(y32, ref, groups)
    worst = None
    for name, _ in groups:
        gate = P.working_gate(e32[name], ceiling)
        ratio = err[name] / gate
        n = int(np.argmax(ratio))
        if worst is None or ratio[n] > worst[4]:
            worst = (name, n, err[name][n], e32[name][n], ratio[n])
        assert bool((err[name] <= gate).all()), \
            f"{form} {tag}: {name} of row {n} off by {err[name][n]:.3e} of its maximum (gate {gate[n]:.2e}, e32 {e32[name][n]:.2e})"
    report(form, tag, f"{worst[0]} of row {worst[1]}", worst[2], worst[3])


# ============================================================================================================ placement
def _tables(c, dev):
    return tuple(t.to(dev) if t is not None else None for t in c["tables"])


def fused_place(dev, c, rc):
    """mipsf_gather_pose_place_fwd_masked -> d_cam, rgb, depth, z_vals, xn, counts, wants_dx"""
    N, S = c["N"], c["S"]
    e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)       # noqa: E731
    d_cam, rgb, depth, z, xn = e(N, 3), e(N, 3), e(N, 1), e(N, S), e(N * S, 3)
    counts = torch.full((N, 2), -1, dtype=torch.int32, device=dev)
    wants = torch.full((N,), -1, dtype=torch.int32, device=dev)
    zu, zoff, znd = _tables(c, dev)
    table, rows, owner = c["table"].to(dev), c["rows"].to(dev), c["owner"].to(dev)
    fixed, rot, trans = c["fixed"].to(dev), c["rot"].to(dev), c["trans"].to(dev)
    noise = c["noise"].to(dev) if c["noise"] is not None else None
    rcode = lib().mipsf_gather_pose_place_fwd_masked(dptr(table), table.shape[0], dptr(rows, torch.int64), dptr(fixed), dptr(rot),
                                                     dptr(trans), P.POSE_F, P.POSE_K, dptr(owner, torch.int64), dptr(noise), dptr(zu),
                                                     dptr(zoff), dptr(znd), C.byref(rc), dptr(d_cam), dptr(rgb), dptr(depth), dptr(z),
                                                     dptr(xn), dptr(counts, torch.int32), dptr(wants, torch.int32), N, stream_ptr())
    _lib.check(rcode, "gather_pose_place_fwd_masked")
    return d_cam, rgb, depth, z, xn, counts, wants


@pytest.mark.parametrize("key", P.PLACE_CASES, ids=P.place_id)
def test_placement(dev, key):
    c = P.place_case(key)
    tag, cfg, N, S = P.place_id(key), c["cfg"], c["N"], c["S"]
    rc = render_cfg(cfg, c["n_uniform"] if c["target_d"] is not None else S, c["n_near"])
    assert rc.perturb == (1 if c["noise"] is not None else 0) and float(rc.norm_factor) == cfg["training"]["norm_factor"]
    table, rows, owner = c["table"].to(dev), c["rows"].to(dev), c["owner"].to(dev)
    with torch.no_grad():
        ro, rd, _, depth = ops.gather_pose_rays(table, rows, c["rot"].to(dev), c["trans"].to(dev), c["fixed"].to(dev), owner)
    noise = c["noise"].to(dev) if c["noise"] is not None else None
    z_ref = P.place_z(c)
    xn_ref = P.place_xn(ro.cpu(), rd.cpu(), z_ref, cfg)
    td = depth if c["target_d"] is not None else None
    z, xn, counts = ops.sample_rays(ro, rd, td, noise, _tables(c, dev), rc, N, S)
    assert_same_bits("sample_rays", tag, "z_vals", z, z_ref)
    assert_same_bits("sample_rays", tag, "xn", xn, xn_ref)
    report("sample_rays", tag, "z_vals, xn: words differing", differing(z, z_ref) + differing(xn, xn_ref), 0.0)
    if c["target_d"] is None:
        return
    assert_same_bits("sample_rays", tag, "target depth", depth, c["target_d"])
    counts_ref = P.place_counts(z_ref, c["target_d"])
    assert torch.equal(counts.cpu(), counts_ref), f"sample_rays {tag}: counts {counts.cpu().tolist()} against {counts_ref.tolist()}"
    # the fused entry point: the same words, and the rows it gathers
    d_cam, rgb, depth2, z2, xn2, counts2, wants = fused_place(dev, c, rc)
    got = c["table"][c["rows"]]
    assert_same_bits("gather_pose_place", tag, "d_cam", d_cam, got[:, :3])
    assert_same_bits("gather_pose_place", tag, "rgb", rgb, got[:, 3:6])
    assert_same_bits("gather_pose_place", tag, "depth", depth2, got[:, 6:7])
    assert_same_bits("gather_pose_place", tag, "z_vals against sample_rays", z2, z)
    assert_same_bits("gather_pose_place", tag, "xn against sample_rays", xn2, xn)
    assert torch.equal(counts2.cpu(), counts_ref), f"gather_pose_place {tag}: counts"
    want = ((c["owner"] % (P.POSE_F + P.POSE_K)) >= P.POSE_F).to(torch.int32)
    assert torch.equal(wants.cpu(), want), f"gather_pose_place {tag}: wants_dx is 0 exactly for the rays of the fixed poses"
    report("gather_pose_place", tag, "z_vals, xn, counts, rows: words differing", differing(z2, z_ref) + differing(xn2, xn_ref), 0.0)
    # and through the autograd function the model calls
    out = ops.GatherPosePlaceFn.apply(c["rot"].to(dev), c["trans"].to(dev), c["fixed"].to(dev), owner, table, rows, noise,
                                      _tables(c, dev), rc, S, False)
    for name, a, b in zip(("rgb", "depth", "z_vals", "xn"), out[:4], (rgb, depth2, z2, xn2)):
        assert_same_bits("GatherPosePlaceFn", tag, name, a, b)
    assert torch.equal(out[4], counts2) and torch.equal(out[5], wants)


# ============================================================================================================ pose path
_POSE_REFS = {}


def pose_refs(key, g_o=True, g_d=True):
    k = (key, g_o, g_d)
    if k not in _POSE_REFS:
        c = P.pose_case(key)
        _POSE_REFS[k] = (P.pose_reference(c, torch.float64, g_o, g_d), P.pose_reference(c, torch.float32, g_o, g_d))
    return _POSE_REFS[k]


def pose_bwd(dev, c, g_o, g_d, accumulate=0, out=None, scratch=None):
    N, F, K = c["N"], c["F"], c["K"]
    if scratch is None:
        scratch = torch.zeros(_lib.buffer_size(_lib.SIZE_POSE_RAYS_SCRATCH, N, F, K), device=dev)
    d_rot, d_trans = out if out is not None else (torch.full((K, 4), 7.0, device=dev), torch.full((K, 3), 7.0, device=dev))
    rot, owner, d_cam = c["rot"].to(dev), c["owner"].to(dev), c["d_cam"].to(dev)
    rcode = lib().mipsf_pose_rays_bwd(dptr(g_o), dptr(g_d), dptr(rot), F, K, dptr(owner, torch.int64), dptr(d_cam), dptr(d_rot),
                                      dptr(d_trans), dptr(scratch), N, accumulate, stream_ptr())
    _lib.check(rcode, "pose_rays_bwd")
    assert int(scratch[:1].view(torch.int32).item()) == 0, "the ticket word is zero after the call"
    return d_rot, d_trans, scratch


@pytest.mark.parametrize("key", P.POSE_CASES, ids=P.pose_id)
def test_pose_rays_forward(dev, key):
    c = P.pose_case(key)
    tag = P.pose_id(key)
    r64, r32 = pose_refs(key)
    fixed = c["fixed"].to(dev) if c["F"] else None
    rot, trans, owner = c["rot"].to(dev), c["trans"].to(dev), c["owner"].to(dev)
    with torch.no_grad():
        ro, rd = ops.pose_rays(rot, trans, fixed, owner, c["d_cam"].to(dev))
        ro2, rd2, rgb, depth = ops.gather_pose_rays(c["table"].to(dev), c["rows"].to(dev), rot, trans, fixed, owner)
    assert_same_bits("pose_rays_fwd", tag, "rays_o against the pose's translation", ro, r32[0])
    check_groups("pose_rays_fwd", tag, rd, r64[1], r32[1], P.RAY_GROUP, P.CEIL_VALUE)
    assert_same_bits("pose_rays_fwd of table rows", tag, "rays_o", ro2, ro)
    assert_same_bits("pose_rays_fwd of table rows", tag, "rays_d", rd2, rd)
    got = c["table"][c["rows"]]
    assert_same_bits("pose_rays_fwd of table rows", tag, "rgb", rgb, got[:, 3:6])
    assert_same_bits("pose_rays_fwd of table rows", tag, "depth", depth, got[:, 6:7])


@pytest.mark.parametrize("key", P.POSE_CASES, ids=P.pose_id)
def test_pose_rays_backward(dev, key):
    c = P.pose_case(key)
    tag = P.pose_id(key)
    r64, r32 = pose_refs(key)
    g_o, g_d = c["g_o"].to(dev), c["g_d"].to(dev)
    d_rot, d_trans, scratch = pose_bwd(dev, c, g_o, g_d)
    check_groups("pose_rays_bwd", tag, d_rot, r64[2], r32[2], P.POSE_GROUPS_ROT, P.CEIL_GRAD)
    check_groups("pose_rays_bwd", tag, d_trans, r64[3], r32[3], P.POSE_GROUPS_TRANS, P.CEIL_GRAD)
    own = c["owner"] % (c["F"] + c["K"])
    for k in range(c["K"]):
        if int((own == c["F"] + k).sum()) == 0:
            assert bool((d_rot[k] == 0).all()) and bool((d_trans[k] == 0).all()), f"{tag}: pose {k} owns no ray: its gradient is exactly 0.0"
    if key[3] in ("five", "scattered") and c["F"] + c["K"] >= 5 and c["N"] > 4:
        return          # (the atomic fall-back past PR_MAXSEG adds in any order: two calls may differ in the last bit)
    acc = (torch.zeros(c["K"], 4, device=dev), torch.zeros(c["K"], 3, device=dev))
    pose_bwd(dev, c, g_o, g_d, accumulate=1, out=acc, scratch=scratch)
    pose_bwd(dev, c, g_o, g_d, accumulate=1, out=acc, scratch=scratch)
    # (compared as fp32 numbers: 0.0 + -0.0 is 0.0, -0.0 + -0.0 is not)
    assert torch.equal(acc[0], d_rot + d_rot), f"pose_rays_bwd {tag}: accumulate twice is not the single d quaternion added to itself"
    assert torch.equal(acc[1], d_trans + d_trans), f"pose_rays_bwd {tag}: accumulate twice is not the single d translation added to itself"


ONE_SIDED = [c for c in P.POSE_CASES if c[0] in (65, 257)]


@pytest.mark.parametrize("which", ["g_o absent", "g_d absent"])
@pytest.mark.parametrize("key", ONE_SIDED, ids=P.pose_id)
def test_pose_rays_backward_of_one_gradient(dev, key, which):
    c = P.pose_case(key)
    tag = f"{P.pose_id(key)} {which}"
    has_o, has_d = which != "g_o absent", which != "g_d absent"
    r64, r32 = pose_refs(key, has_o, has_d)
    d_rot, d_trans, _ = pose_bwd(dev, c, c["g_o"].to(dev) if has_o else None, c["g_d"].to(dev) if has_d else None)
    check_groups("pose_rays_bwd", tag, d_rot, r64[2], r32[2], P.POSE_GROUPS_ROT, P.CEIL_GRAD)
    check_groups("pose_rays_bwd", tag, d_trans, r64[3], r32[3], P.POSE_GROUPS_TRANS, P.CEIL_GRAD)
    assert has_o or bool((d_trans == 0).all())
    assert has_d or bool((d_rot == 0).all())


def test_pose_rays_accumulate_with_the_atomic_fall_back(dev):
    """accumulate = 1 where a wave has more than PR_MAXSEG owners: the sum of two calls is the float64 answer doubled, under the gate
    (bit equality with the single call does not hold there: the LDS atomics add in any order)"""
    key = next(c for c in P.POSE_CASES if c[3] == "scattered" and c[1:3] == (2, 9) and c[0] == 1000)
    c = P.pose_case(key)
    r64, r32 = pose_refs(key)
    acc = (torch.zeros(c["K"], 4, device=dev), torch.zeros(c["K"], 3, device=dev))
    _, _, scratch = pose_bwd(dev, c, c["g_o"].to(dev), c["g_d"].to(dev), accumulate=1, out=acc)
    pose_bwd(dev, c, c["g_o"].to(dev), c["g_d"].to(dev), accumulate=1, out=acc, scratch=scratch)
    check_groups("pose_rays_bwd accumulate twice", P.pose_id(key), acc[0], 2 * r64[2], 2 * r32[2], P.POSE_GROUPS_ROT, P.CEIL_GRAD)
    check_groups("pose_rays_bwd accumulate twice", P.pose_id(key), acc[1], 2 * r64[3], 2 * r32[3], P.POSE_GROUPS_TRANS, P.CEIL_GRAD)


@pytest.mark.parametrize("key", P.PPB_CASES, ids=P.ppb_id)
def test_place_pose_bwd(dev, key):
    c = P.ppb_case(key)
    tag = P.ppb_id(key)
    N, S, F, K = c["N"], c["S"], c["F"], c["K"]
    rc = render_cfg(c["cfg"], S, 0)
    r64, r32 = P.ppb_reference(c, torch.float64), P.ppb_reference(c, torch.float32)
    scratch = torch.zeros(_lib.buffer_size(_lib.SIZE_PLACE_POSE_SCRATCH, N, F, K), device=dev)
    dxn, z, rot, owner, d_cam = (c[k].to(dev) for k in ("dxn", "z", "rot", "owner", "d_cam"))

    def call(d_rot, d_trans, accumulate):
        rcode = lib().mipsf_place_pose_bwd(dptr(dxn), dptr(z), C.byref(rc), dptr(rot), F, K, dptr(owner, torch.int64), dptr(d_cam),
                                           dptr(d_rot), dptr(d_trans), dptr(scratch), N, S, accumulate, stream_ptr())
        _lib.check(rcode, "place_pose_bwd")
        assert int(scratch[:1].view(torch.int32).item()) == 0, "the ticket word is zero after the call"
    d_rot, d_trans = torch.full((K, 4), 7.0, device=dev), torch.full((K, 3), 7.0, device=dev)
    call(d_rot, d_trans, 0)
    check_groups("place_pose_bwd", tag, d_rot, r64[0], r32[0], P.POSE_GROUPS_ROT, P.CEIL_GRAD)
    check_groups("place_pose_bwd", tag, d_trans, r64[1], r32[1], P.POSE_GROUPS_TRANS, P.CEIL_GRAD)
    a_rot, a_trans = torch.zeros(K, 4, device=dev), torch.zeros(K, 3, device=dev)
    call(a_rot, a_trans, 1)
    call(a_rot, a_trans, 1)
    assert torch.equal(a_rot, d_rot + d_rot), f"place_pose_bwd {tag}: accumulate twice is not the single d quaternion added to itself"
    assert torch.equal(a_trans, d_trans + d_trans), f"place_pose_bwd {tag}: accumulate twice is not the single d translation added to itself"


# ===================================================================================== frequency encoding, normalisation
@pytest.mark.parametrize("n_freq", P.FREQ_NFREQ)
@pytest.mark.parametrize("M", P.FREQ_MS)
def test_frequency(dev, M, n_freq):
    x, dout = P.freq_case(M, n_freq)
    tag = f"M{M}-F{n_freq}"
    (o64, dx64), (o32, dx32) = P.freq_reference(x, dout, n_freq, torch.float64), P.freq_reference(x, dout, n_freq, torch.float32)
    W = 6 * n_freq
    xd, dd = x.to(dev), dout.to(dev)
    buf = torch.full((M * W + 64,), 777.0, device=dev)
    dxb = torch.full((M * 3 + 64,), 777.0, device=dev)
    _lib.check(lib().mipsf_freq_fwd(dptr(xd), dptr(buf), M, 3, n_freq, stream_ptr()), "freq_fwd")
    _lib.check(lib().mipsf_freq_bwd(dptr(xd), dptr(dd), dptr(dxb), M, 3, n_freq, stream_ptr()), "freq_bwd")
    assert bool((buf[M * W:] == 777.0).all()) and bool((dxb[M * 3:] == 777.0).all()), "the words behind the outputs are untouched"
    out, dx = buf[:M * W].reshape(M, W).cpu(), dxb[:M * 3].reshape(M, 3).cpu()
    err, e32 = P.value_error(out, o64), P.value_error(o32, o64)
    gate = float(P.working_gate(e32, P.CEIL_VALUE))
    report("freq_fwd", tag, "out", err, e32)
    assert err <= gate, f"freq_fwd {tag}: off by {err:.3e} (gate {gate:.2e}, e32 {e32:.2e})"
    check_groups("freq_bwd", tag, dx, dx64, dx32, (("dx", slice(0, 3)),), P.CEIL_GRAD)
    # the module's autograd function gives the same words
    xr = xd.clone().requires_grad_(True)
    o = ops.FrequencyFn.apply(xr, n_freq)
    o.backward(dd)
    assert_same_bits("FrequencyFn", tag, "out", o, out)
    assert_same_bits("FrequencyFn", tag, "dx", xr.grad, dx)


@pytest.mark.parametrize("use_bound,nf", [(True, 1.0), (True, 2.0), (False, 1.0), (False, 2.0)])
@pytest.mark.parametrize("M", P.FREQ_MS)
def test_normalise(dev, M, use_bound, nf):
    cfg = P.place_cfg(1, 0, perturb=0, use_bound=use_bound, norm_factor=nf)
    rc = render_cfg(cfg, 1, 0)
    gen = torch.Generator().manual_seed(M)
    pts = torch.randn(M, 3, generator=gen) * 6.0 + 2.0                     # inside and far outside the box
    g = torch.randn(M, 3, generator=gen)
    tag = f"M{M}-{'bound' if use_bound else 'len'}-nf{nf:g}"
    xn = ops.normalise_points(pts.to(dev), rc)
    assert_same_bits("normalise_points", tag, "xn", xn, P.normalised(pts, cfg))
    assert M < 85 or bool(((xn < 0) | (xn > 1)).any()), "points outside the box"
    assert_same_bits("normalise_bwd", tag, "d pts", ops.normalise_bwd(g.to(dev), rc), P.normalise_bwd_answer(g, cfg))
    report("normalise", tag, "xn, d pts: words differing", 0.0, 0.0)


# ================================================================================================================= Adam
SENTINEL, GUARD = 4242.5, 8
TICKET_WORDS, TICKET_LIVE = 576, 528           # MIPSF_ADAM_TICKET_WORDS; the tickets proper: 16 * 33 words


class Held:
    """p, g, m, v of one tensor, each a contiguous view `off` floats behind the 32-byte guard of a buffer of sentinels"""

    def __init__(self, dev, state, offs=(0, 0, 0, 0)):
        self.n, self.offs, self.bufs, self.t = state[0].numel(), offs, [], []
        for val, off in zip(state, offs):
            buf = torch.full((self.n + 2 * GUARD + off,), SENTINEL, device=dev)
            view = buf[GUARD + off: GUARD + off + self.n]
            view.copy_(val)
            assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (off % 4 == 0)
            self.bufs.append(buf)
            self.t.append(view)

    def read(self):
        return tuple(t.cpu().clone() for t in self.t)

    def guards_intact(self):
        for buf, off in zip(self.bufs, self.offs):
            if not (bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + self.n:] == SENTINEL).all())):
                return False
        return True


def group_of(dev, held, hyper, step_before):
    """a group for adam_step_small / adam_step_all with the device step counter seeded"""
    lr, b1, b2, eps, wd = hyper
    step_dev = torch.tensor([step_before], dtype=torch.int32, device=dev)
    hyper_dev = torch.zeros(2, device=dev)
    return (step_dev, hyper_dev, lr, b1, b2, eps, wd, [tuple(h.t) for h in held])


def ulps(a, want64):
    """distance of the fp32 ``a`` from the float64 ``want64`` in ulps of fp32(want64)"""
    w = np.float32(want64)
    return abs(float(a) - want64) / float(np.spacing(w))


def check_scalars(tag, hyper_dev, hyper, step):
    h0, h1 = P.adam_scalars(hyper[0], hyper[1], hyper[2], step)
    got = hyper_dev.cpu()
    assert ulps(got[0], h0) <= 1.0 and ulps(got[1], h1) <= 1.0, \
        f"{tag}: lr / bc1 = {float(got[0])!r} (float64 {h0!r}), 1 / sqrt(bc2) = {float(got[1])!r} (float64 {h1!r}) at step {step}"


def check_step(form, tag, before, after, hyper, step, zero_grad):
    """one step from the state the device held: new p, m, v element by element under the derived bound; the gradient exactly 0
    after zero_grad (every element: the tail too), else untouched.  The printed line carries the largest share of the bound in
    the kernel column and the bound itself, 1, in the e32 column"""
    want = P.adam_answer(*before, step, *hyper)
    bound = P.adam_bound(*before, step, *hyper)
    worst = None
    for name, a, r, b in zip(("p", "exp_avg", "exp_avg_sq"), (after[0], after[2], after[3]), want, bound):
        ratio = (a.double() - r).abs() / b
        assert not bool(torch.isnan(a).any()), f"{form} {tag}: NaN in {name}"
        i = int(torch.argmax(ratio))
        if worst is None or float(ratio[i]) > worst[1]:
            worst = (name, float(ratio[i]))
        assert float(ratio[i]) <= 1.0, (f"{form} {tag}: {name}[{i}] = {a[i].item()!r}, float64 {r[i].item()!r}: off by {float(ratio[i]):.2f} "
                                        f"of the bound {b[i].item():.3e}")
    if zero_grad:
        assert bool((after[1] == 0).all()), f"{form} {tag}: the gradient is not exactly 0 after zero_grad"
    else:
        assert torch.equal(after[1], before[1]), f"{form} {tag}: the gradient was written to"
    report(form, tag, f"{worst[0]}: share of the bound", worst[1], 1.0)


def run_entry(entry, dev, held, hyper, step, zero_grad, ticket=None):
    """one step of ONE tensor through one of the four entry points; -> hyper_dev (or None) and the ticket block"""
    lr, b1, b2, eps, wd = hyper
    p, g, m, v = held.t
    if entry == "adam_step":
        ops.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, zero_grad)
        return None, None
    if entry == "adam_step_multi":
        ops.adam_step_multi([p], [g], [m], [v], lr, b1, b2, eps, wd, step, zero_grad)
        return None, None
    grp = group_of(dev, [held], hyper, step - 1)
    if entry == "adam_step_small":
        ops.adam_step_small([grp], zero_grad)
    else:
        ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev) if ticket is None else ticket
        ops.adam_step_all([grp], ticket, zero_grad)
        assert bool((ticket[:TICKET_LIVE] == 0).all()), "the tickets are zero after the step"
    assert int(grp[0].item()) == step, "the device step counter advanced by one"
    check_scalars(entry, grp[1], hyper, step)
    return grp[1], ticket


ENTRIES = ("adam_step", "adam_step_multi", "adam_step_small", "adam_step_all")
ADAM_RUNS = [(e, n, i) for i, (e, n) in enumerate((e, n) for e in ENTRIES for n in P.ADAM_NS)
             if not (e == "adam_step_small" and n > _lib.ADAM_SMALL_MAX_NUMEL)]


@pytest.mark.parametrize("entry,n,i", ADAM_RUNS, ids=lambda v: str(v))
def test_adam_one_step(dev, entry, n, i):
    hyper = P.ADAM_HYPER[i % 4]
    step = (1, 2, 3, 10, 1000)[(i // 4 + i) % 5]
    zero_grad = i % 2 == 0
    held = Held(dev, P.adam_state(n))
    before = held.read()
    run_entry(entry, dev, held, hyper, step, zero_grad)
    check_step(entry, f"n{n}-step{step}-wd{hyper[4]:g}-eps{hyper[3]:g}", before, held.read(), hyper, step, zero_grad)
    assert held.guards_intact(), f"{entry} n{n}: a word next to a tensor's end was written"


@pytest.mark.parametrize("step", P.ADAM_STEPS)
def test_adam_scalars_from_a_seeded_counter(dev, step):
    """hyper_dev after the step that makes the counter `step`: within one fp32 ulp of the float64 value (a double-precision result
    rounded once; a tie may flip) -- adam_advance_n (pow), adam_step_small (pow), adam_step_all (repeated squaring), and
    adam_step_all's scalars LEFT for the next step, which the step after it takes from the ticket block"""
    hyper = P.ADAM_HYPER[step % 4]
    step_dev, hyper_dev = torch.tensor([step - 1], dtype=torch.int32, device=dev), torch.zeros(2, device=dev)
    ops.adam_advance(step_dev, hyper_dev, hyper[0], hyper[1], hyper[2])
    assert int(step_dev.item()) == step
    check_scalars("adam_advance", hyper_dev, hyper, step)
    for entry in ("adam_step_small", "adam_step_all"):
        held = Held(dev, P.adam_state(5))
        before = held.read()
        _, ticket = run_entry(entry, dev, held, hyper, step, False)
        check_step(entry, f"n5-step{step}", before, held.read(), hyper, step, False)
        if entry == "adam_step_all":
            left = ticket[TICKET_LIVE:TICKET_LIVE + 4].cpu()
            assert int(left[0]) == step + 1
            check_scalars("adam_step_all, left for the next step", left[1:3].view(torch.float32), hyper, step + 1)
            before = held.read()
            run_entry(entry, dev, held, hyper, step + 1, True, ticket=ticket)
            check_step(entry, f"n5-step{step + 1} from the scalars left", before, held.read(), hyper, step + 1, True)


@pytest.mark.parametrize("n,blocks", [(4, 2), (30720, 31), (31744, 32), (32768, 33)])
def test_adam_all_grid_sizes(dev, n, blocks):
    """the two-level ticket on grids of 2, 31, 32 and 33 workgroups: three steps in a row on one ticket block"""
    assert (n // 4 + 255) // 256 + 1 == blocks
    hyper = P.ADAM_HYPER[1]
    held = Held(dev, P.adam_state(n, seed=blocks))
    ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev)
    for step in (1, 2, 3):
        if step > 1:
            held.t[1].copy_(P.adam_state(n, seed=blocks + step)[1])
        before = held.read()
        run_entry("adam_step_all", dev, held, hyper, step, step != 2, ticket=ticket)
        check_step("adam_step_all", f"{blocks} workgroups, step {step}", before, held.read(), hyper, step, step != 2)
    assert held.guards_intact()


def test_adam_all_two_groups_of_odd_sizes(dev):
    hypers, sizes = (P.ADAM_HYPER[1], P.ADAM_HYPER[3]), ((1025, 3, 16385), (5, 1023))
    held = [[Held(dev, P.adam_state(n, seed=gi)) for n in ns] for gi, ns in enumerate(sizes)]
    groups = [group_of(dev, hs, hy, st) for hs, hy, st in zip(held, hypers, (0, 9))]
    ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev)
    for rnd in range(2):
        before = [[h.read() for h in hs] for hs in held]
        ops.adam_step_all(groups, ticket, rnd == 0)
        assert bool((ticket[:TICKET_LIVE] == 0).all())
        for gi, (hs, hy) in enumerate(zip(held, hypers)):
            step = (0, 9)[gi] + rnd + 1
            assert int(groups[gi][0].item()) == step
            check_scalars(f"group {gi}", groups[gi][1], hy, step)
            for h, b in zip(hs, before[gi]):
                check_step("adam_step_all, two groups", f"group {gi} n{h.n} step {step}", b, h.read(), hy, step, rnd == 0)
                assert h.guards_intact()
                h.t[1].copy_(P.adam_state(h.n, seed=50 + gi)[1])


@pytest.mark.parametrize("entry", ["adam_step_small", "adam_step_all"])
@pytest.mark.parametrize("change", ["lr", "betas"])
def test_adam_scalars_follow_a_change_between_two_steps(dev, entry, change):
    """a learning-rate schedule, or new betas, between two steps: the scalars adam_step_all left for the second step were worked
    out from the old values (adam_key tells), and must not be used"""
    first = P.ADAM_HYPER[1]
    second = (first[0] * 0.5,) + first[1:] if change == "lr" else (first[0], 0.8, 0.99) + first[3:]
    held = Held(dev, P.adam_state(1025))
    step_dev, hyper_dev = torch.tensor([4], dtype=torch.int32, device=dev), torch.zeros(2, device=dev)
    ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev)
    for step, hyper in ((5, first), (6, second)):
        lr, b1, b2, eps, wd = hyper
        before = held.read()
        grp = (step_dev, hyper_dev, lr, b1, b2, eps, wd, [tuple(held.t)])
        if entry == "adam_step_small":
            ops.adam_step_small([grp], False)
        else:
            ops.adam_step_all([grp], ticket, False)
            assert bool((ticket[:TICKET_LIVE] == 0).all())
        assert int(step_dev.item()) == step
        check_scalars(entry, hyper_dev, hyper, step)
        check_step(entry, f"step {step}, {change} changed" if step == 6 else f"step {step}", before, held.read(), hyper, step, False)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", ["p", "g", "m", "v", "all"])
def test_adam_buffers_that_are_not_16_byte_aligned(dev, which, off):
    """adam_all_kernel's scalar path (vec == false): one operand at a time and all together; adam_step refuses such buffers"""
    offs = tuple(off if which in (name, "all") else 0 for name in "pgmv")
    hyper, step, n = P.ADAM_HYPER[1], 3, 1027
    held = Held(dev, P.adam_state(n), offs)
    before = held.read()
    with pytest.raises(RuntimeError, match="adam buffers must be 16-byte aligned"):
        run_entry("adam_step", dev, held, hyper, step, True)
    assert all(torch.equal(a, b) for a, b in zip(before, held.read())), "a refused call writes nothing"
    run_entry("adam_step_all", dev, held, hyper, step, True)
    check_step("adam_step_all", f"{which} {off} floats off", before, held.read(), hyper, step, True)
    assert held.guards_intact(), "a word next to a tensor's end was written"


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [5, 1025, 16384])
def test_adam_paths_agree_bit_for_bit(dev, n, step):
    """all four entry points given the same scalars: adam_step_small writes hyper_dev, adam_step and adam_step_multi read it;
    adam_step_all works its own out (repeated squaring) and must arrive at the same two words"""
    hyper = P.ADAM_HYPER[3]
    lr, b1, b2, eps, wd = hyper
    results = {}
    held = Held(dev, P.adam_state(n))
    hyper_dev, _ = run_entry("adam_step_small", dev, held, hyper, step, False)
    results["adam_step_small"] = held.read()
    held = Held(dev, P.adam_state(n))
    hyper_all, _ = run_entry("adam_step_all", dev, held, hyper, step, False)
    assert_same_bits("adam_step_all", f"step {step}", "hyper_dev against adam_step_small's", hyper_all, hyper_dev)
    results["adam_step_all"] = held.read()
    held = Held(dev, P.adam_state(n))
    ops.adam_step(*held.t, lr, b1, b2, eps, wd, 0, False, hyper_dev=hyper_dev)
    results["adam_step"] = held.read()
    held = Held(dev, P.adam_state(n))
    p, g, m, v = held.t
    ops.adam_step_multi([p], [g], [m], [v], lr, b1, b2, eps, wd, 0, False, hyper_dev=hyper_dev)
    results["adam_step_multi"] = held.read()
    for name in ENTRIES[:2] + ENTRIES[3:]:
        for what, a, b in zip(("p", "g", "exp_avg", "exp_avg_sq"), results[name], results["adam_step_small"]):
            assert_same_bits(name, f"n{n} step {step}", f"{what} against adam_step_small's", a, b)
    report("adam paths", f"n{n}-step{step}", "four paths: words differing", 0.0, 0.0)
    assert math.isfinite(float(results["adam_step"][0].abs().max()))
