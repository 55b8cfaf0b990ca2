"""GPU (-m gpu): every kernel of csrc/render.hip that a training or tracking step runs -- render_fwd_kernel (evaluation, two-launch
and ticket forms), render_train_kernel (with and without `draw`), loss_finalize_kernel, loss_finalize_sums_kernel, render_bwd_kernel,
rays_bwd_kernel -- against an INDEPENDENT answer: oracle/path_cpu.py in float64 with autograd (tests/render_cpu.py), on inputs whose
every discrete decision is exact in fp32 and float64 alike (tests/test_render_cpu.py holds the inputs to that), with planted ties
and edges.  The kernel-against-kernel tests of tests/test_gpu_parity.py cannot see an expression of render_dev.h that is wrong in
all kernels alike; these can.

Gates.  A gradient is compared per ray and per column group (draw: columns 0..2, 3, 5..9; d rays_o, d rays_d: one group each),
normalised by that ray's largest reference magnitude in the group; a per-ray map by the batch maximum of the map; a loss by its own
magnitude.  Working gate per group: max(8 e32, 64 * 2^-24), never above the project's ceilings (1e-4 maps and losses, 5e-4
gradients), where e32 is the error of the SAME oracle code run in fp32 against float64 on that group (8: another summation order
and an ulp of expf; 64 * 2^-24: two expf, two divisions, a 256-term sum and G.at - dot, where e32 may be a single rounding).  No
outlier allowance.  Where the float64 gradient is exactly 0 the kernel's entry is == 0.0; NaN exactly where float64 has NaN.

One group has a third term in its working gate (the ceiling stays): column 3 of `draw`.  The kernels form A_k = MapGrad::at (the
colour and depth gradients of a sample in ONE number) and subtract dot = sum_j A_j wn_j; on a ray whose weight sits on one or two
samples that difference is a small part of A_k, and the roundings of A_k and dot, which have the size of the terms' magnitudes,
stand against it.  Autograd carries the colour and the depth gradients apart and never forms A_k, so e32 does not contain this
step: on the MI355X such rays were off by 1.2e-5 of the column's maximum beside an e32 of 4e-7 to 1e-6 (first run, four cases
above 8 e32, all of this kind, all forty times under the ceiling).  The term is the step's forward error bound from float64
quantities (render_cpu.sdf_cancellation: 16 roundings of 2^-24 on |A|_k + sum_j |A|_j wn_j, through d wn_k / d sdf_k).

One entry is not float64's: disp_map of a ray whose every weight underflows in fp32 (the planted SDF of +-8).  fp32 has
1 / max(1e-10, 0 / 0) = NaN there (torch.max keeps a NaN), float64 has 1e-56 / 1e-56 and a finite answer no fp32 code can reach:
the kernel must give the fp32 oracle's NaN.

Measured on an MI355X (worst group per form, kernel error | e32): see DESIGN.md, "The render kernels against float64"."""
import ctypes as C

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import dptr, lib, stream_ptr

from . import render_cpu as R

pytestmark = pytest.mark.gpu
LW = [1.0, 0.1, 1000.0, 10.0]
SMALL = [c for c in R.CASES if c[1] <= ops.RENDER_DRAW_MAX_S]
N33 = [c for c in R.CASES if c[0] == 33]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- shared, computed once
_REFS, _DEV = {}, {}


def refs(case, tag, **grads):
    """(float64 answer, fp32 yardstick) of a case for one set of gradients; computed once, never written to"""
    if tag not in _REFS:
        _REFS[tag] = (R.reference(case, **grads), R.reference_dtype(case, torch.float32, **grads))
    return _REFS[tag]


def on_device(case, tag, dev):
    if tag not in _DEV:
        cfg = case["cfg"]
        S = case["z"].shape[1]
        rc = ops.make_render_cfg(cfg, cfg["mapping"]["bound"], cfg["mapping"]["localMLP_max_len"], S, 0, case["emd_w"])
        _DEV[tag] = tuple(case[k].to(dev) for k in ("raw", "z", "target_rgb", "target_d", "counts")) + (rc,)
    return _DEV[tag]


def report(form, tag, name, err, e32):
    print(f"\n  fp64 | {form} | {tag} | {name} | kernel {err:.2e} | e32 {e32:.2e}", end="")


# ------------------------------------------------------------------------------------------------- the comparisons
def check_maps(form, tag, outs, r64, r32):
    """outs: rgb, depth, depth_var, disp, acc[, weights] of the kernel"""
    worst = None
    under = r32["acc_map"] == 0                     # every weight underflowed in fp32: disp is 1 / max(1e-10, 0 / 0)
    for name, k in zip(R.MAP_NAMES, outs):
        if k is None:
            continue
        k, ref, y32 = k.detach().cpu().double(), r64[name].clone(), r32[name].double().clone()
        if name == "disp_map" and bool(under.any()):
            assert bool(torch.isnan(y32[under]).all()) and bool(torch.isnan(k[under]).all()), "disp of a ray without weight is NaN"
            k, ref, y32 = k[~under], ref[~under], y32[~under]
        err, e32 = R.value_error(k, ref), R.value_error(y32, ref)
        gate = float(R.working_gate(e32, R.CEIL_VALUE))
        if worst is None or err / gate > worst[1] / worst[3]:
            worst = (name, err, e32, gate)
        assert err <= gate, f"{form} {tag}: {name} off by {err:.3e} of the batch maximum (gate {gate:.2e}, e32 {e32:.2e})"
    report(form, tag, worst[0], worst[1], worst[2])


def check_losses(form, tag, losses, total, r64, r32):
    k = losses.detach().cpu().double()
    worst = None
    assert float(k[7]) == float(r64["losses"][7]), "n_valid is a count"
    rows = [(R.LOSS_NAMES[j], k[j], r64["losses"][j], r32["losses"][j]) for j in range(7)]
    if total is not None:
        rows.append(("objective", total.detach().cpu().double().reshape(()), r64["objective"], r32["objective"]))
    for name, a, ref, y32 in rows:
        err, e32 = R.value_error(a, ref), R.value_error(y32.double(), ref)
        gate = float(R.working_gate(e32, R.CEIL_VALUE))
        if worst is None or err / gate > worst[1] / worst[3]:
            worst = (name, err, e32, gate)
        assert err <= gate, f"{form} {tag}: {name} = {float(a)!r}, float64 {float(ref)!r}: off by {err:.3e} (gate {gate:.2e}, e32 {e32:.2e})"
    report(form, tag, worst[0], worst[1], worst[2])


def check_draw(form, tag, a, case, r64, r32, rows=None):
    """d objective / d raw; column 3 also gets the bound of its cancelling step (render_cpu.sdf_cancellation: measured on an MI355X,
    rays with their weight on one or two samples were off by 1.2e-5 of the column's maximum where e32 was 4e-7 to 1e-6)"""
    check_grad(form, tag, a, r64["draw"], r32["draw"], R.DRAW_GROUPS, rows, {"sdf": R.sdf_cancellation(case, r64)})


def check_grad(form, tag, a, ref, y32, groups, rows=None, extra=None):
    """a: the kernel's gradient; ref / y32: float64 / fp32 oracle (rows: the slice of their rays that ``a`` holds); extra: {group:
    [N] further term of the working gate}"""
    a = a.detach().cpu()
    extra = dict(extra or {})
    if rows is not None:
        ref, y32 = ref[rows], y32[rows]
        extra = {k: v[rows] for k, v in extra.items()}
    assert torch.equal(torch.isnan(a), torch.isnan(ref)), f"{form} {tag}: NaN in other places than float64's"
    zero = ref == 0
    assert bool((a[zero] == 0).all()), f"{form} {tag}: {int((a[zero] != 0).sum())} entries are not 0.0 where the float64 gradient is exactly 0"
    err, e32 = R.group_errors(a, ref, groups), R.group_errors(y32, ref, groups)
    worst = None
    for name, _ in groups:
        gate = R.working_gate(e32[name], R.CEIL_GRAD, extra.get(name, 0.0))
        ratio = err[name] / gate
        n = int(np.argmax(ratio))
        if worst is None or ratio[n] > worst[4]:
            worst = (name, n, err[name][n], e32[name][n], ratio[n])
        assert bool((err[name] <= gate).all()), \
            f"{form} {tag}: group {name} of ray {n} off by {err[name][n]:.3e} of its maximum (gate {gate[n]:.2e}, e32 {e32[name][n]:.2e})"
    report(form, tag, f"{worst[0]} of ray {worst[1]}", worst[2], worst[3])


def two_launches(dev, raw, z, t_rgb, t_d, counts, rc, N, S, lw):
    """mipsf_render_fwd without a ticket: render_fwd_kernel<true, false, 4>, then loss_finalize_kernel"""
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)      # noqa: E731
    outs = [f(N, 3), f(N), f(N), f(N), f(N), f(N, S)]
    losses, partial, total = f(8), f(_lib.buffer_size(_lib.SIZE_RENDER_PARTIAL, N)), f(1)
    a = _lib.RenderFwdArgs.new(N=N, S=S, raw=dptr(raw), z_vals=dptr(z), target_rgb=dptr(t_rgb), target_d=dptr(t_d),
                               counts=dptr(counts, torch.int32), cfg=C.pointer(rc), rgb=dptr(outs[0]), depth=dptr(outs[1]),
                               depth_var=dptr(outs[2]), disp=dptr(outs[3]), acc=dptr(outs[4]), weights=dptr(outs[5]),
                               losses=dptr(losses), partial=dptr(partial), loss_weights=dptr(lw), loss_total=dptr(total))
    assert lib().mipsf_render_fwd(C.byref(a), stream_ptr()) == 0
    return outs, losses, total


# ------------------------------------------------------------------------------------------------------ the forms
@pytest.mark.parametrize("key", R.CASES, ids=R.case_id)
def test_eval_forward(dev, key):
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, tag, loss_weights=LW)
    res = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, False, want_weights=True)
    assert res[6] is None
    check_maps("eval forward", tag, res[:6], r64, r32)


@pytest.mark.parametrize("key", R.CASES, ids=R.case_id)
def test_training_forward_in_two_launches(dev, key):
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, tag, loss_weights=LW)
    outs, losses, total = two_launches(dev, raw, z, t_rgb, t_d, counts, rc, N, S, torch.tensor(LW, device=dev))
    check_maps("two launches", tag, outs, r64, r32)
    check_losses("two launches", tag, losses, total, r64, r32)


@pytest.mark.parametrize("key", R.CASES, ids=R.case_id)
def test_training_forward_in_one_launch(dev, key):
    """render_train_kernel up to S = 128, render_fwd_kernel's ticket form above"""
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, tag, loss_weights=LW)
    res = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, True, want_weights=True, loss_weights=torch.tensor(LW, device=dev))
    check_maps("one launch", tag, res[:6], r64, r32)
    check_losses("one launch", tag, res[6], res[7], r64, r32)


@pytest.mark.parametrize("key", SMALL, ids=R.case_id)
def test_gradient_written_by_the_forward_launch(dev, key):
    """want_draw: render_train_kernel<true, .> writes d objective / d raw for the loss weights alone"""
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, tag, loss_weights=LW)
    res = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, True, want_weights=True, loss_weights=torch.tensor(LW, device=dev),
                         want_draw=True)
    check_maps("forward with draw", tag, res[:6], r64, r32)
    check_losses("forward with draw", tag, res[6], res[7], r64, r32)
    check_draw("draw of the forward", tag, res[8], case, r64, r32)


@pytest.mark.parametrize("g_total", [1.0, -2.5])
@pytest.mark.parametrize("key", R.CASES, ids=R.case_id)
def test_render_bwd_of_the_objective(dev, key, g_total):
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, f"{tag} x {g_total}", loss_weights=[g_total * w for w in LW])
    lw = torch.tensor(LW, device=dev)
    losses = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, True, loss_weights=lw)[6]
    draw = ops.render_bwd(raw, z, t_rgb, t_d, counts, losses, rc, None, None, None, N, S,
                          g_total=torch.tensor([g_total], device=dev), loss_weights=lw)
    check_draw(f"render_bwd g_total {g_total:g}", tag, draw, case, r64, r32)


@pytest.mark.parametrize("key", R.CASES, ids=R.case_id)
def test_render_bwd_of_given_gradients(dev, key):
    """g_losses, g_rgb and g_depth given directly, no g_total: the autograd path of any objective other than the built-in one"""
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    gen = torch.Generator().manual_seed(key[2])
    g_losses = torch.tensor([1.0, 0.1, 100.0, 10.0]) * (0.5 + torch.rand(4, generator=gen)) * torch.tensor([1.0, -1.0, 1.0, -1.0])
    g_rgb, g_depth = torch.randn(N, 3, generator=gen) / N, torch.randn(N, generator=gen) / N
    r64, r32 = refs(case, f"{tag} given", g_losses=g_losses, g_rgb=g_rgb, g_depth=g_depth)
    losses = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, True)[6]
    draw = ops.render_bwd(raw, z, t_rgb, t_d, counts, losses, rc, g_losses.to(dev), g_rgb.to(dev), g_depth.to(dev), N, S)
    check_draw("render_bwd given gradients", tag, draw, case, r64, r32)


@pytest.mark.parametrize("cut", [16, 1])
@pytest.mark.parametrize("key", N33, ids=R.case_id)
def test_shares_of_a_batch(dev, key, cut):
    """render_fwd(share_of=) + mipsf_loss_finalize_sums + render_bwd(n_norm=): 33 rays as shares of `cut` and 33 - cut rays give the
    whole batch's float64 losses, and each share's rows of the whole batch's float64 gradient"""
    N, S = key[:2]
    tag = R.case_id(key)
    case = R.case_of(key)
    r64, r32 = refs(case, tag, loss_weights=LW)
    lw = torch.tensor(LW, device=dev)
    rc = on_device(case, tag, dev)[5]
    spans = [(0, cut), (cut, N)]
    parts = [tuple(t.to(dev) for t in (s["raw"], s["z"], s["target_rgb"], s["target_d"], s["counts"]))
             for s in (R.share(case, lo, hi) for lo, hi in spans)]
    own = []

    def keep_own(t):
        own.append(t.clone())
        return t
    for (lo, hi), p in zip(spans, parts):
        ops.render_fwd(*p, rc, hi - lo, S, True, loss_weights=lw, share_of=keep_own)
    whole = own[0] + own[1]
    assert float(whole[9]) == N
    for (lo, hi), p in zip(spans, parts):
        form = f"share {lo}:{hi}"
        res = ops.render_fwd(*p, rc, hi - lo, S, True, want_weights=True, loss_weights=lw, share_of=lambda t: whole.clone())
        assert res[8] == N
        rows = slice(lo, hi)
        r64s = {k: (v[rows] if k in R.MAP_NAMES else v) for k, v in r64.items()}
        r32s = {k: (v[rows] if k in R.MAP_NAMES else v) for k, v in r32.items()}
        check_maps(form, tag, res[:6], r64s, r32s)
        check_losses(form, tag, res[6], res[7], r64, r32)
        draw = ops.render_bwd(*p, res[6], rc, None, None, None, hi - lo, S, g_total=torch.ones(1, device=dev), loss_weights=lw,
                              n_norm=N)
        check_draw(form + " render_bwd", tag, draw, case, r64, r32, rows=rows)


@pytest.mark.parametrize("mode", ["invalid", "none"])
@pytest.mark.parametrize("key", R.EDGE_CASES, ids=R.case_id)
def test_batches_without_depth(dev, key, mode):
    """no valid depth at all ("invalid": depth_loss is 0 / 0), and the counts all zero as well ("none": the band weights, fs_loss,
    sdf_loss and every gradient entry they reach are 0 / 0 too): NaN exactly where float64 has NaN, numbers elsewhere"""
    N, S = key[:2]
    tag = f"{R.case_id(key)} {mode}"
    case = R.with_depths(R.case_of(key), mode)
    raw, z, t_rgb, t_d, counts, rc = on_device(case, tag, dev)
    r64, r32 = refs(case, tag, loss_weights=LW)
    assert bool(torch.isnan(r64["losses"][1])) and bool(torch.isnan(r64["objective"]))
    assert bool(torch.isnan(r64["losses"][3])) == (mode == "none")
    lw = torch.tensor(LW, device=dev)
    outs, losses, total = two_launches(dev, raw, z, t_rgb, t_d, counts, rc, N, S, lw)
    check_maps("no depth, two launches", tag, outs, r64, r32)
    check_losses("no depth, two launches", tag, losses, total, r64, r32)
    small = S <= ops.RENDER_DRAW_MAX_S
    res = ops.render_fwd(raw, z, t_rgb, t_d, counts, rc, N, S, True, want_weights=True, loss_weights=lw, want_draw=small)
    check_maps("no depth, one launch", tag, res[:6], r64, r32)
    check_losses("no depth, one launch", tag, res[6], res[7], r64, r32)
    if small:
        check_draw("no depth, draw of the forward", tag, res[8], case, r64, r32)
    draw = ops.render_bwd(raw, z, t_rgb, t_d, counts, res[6], rc, None, None, None, N, S, g_total=torch.ones(1, device=dev),
                          loss_weights=lw)
    check_draw("no depth, render_bwd", tag, draw, case, r64, r32)


@pytest.mark.parametrize("use_bound", [True, False], ids=["bound", "max_len"])
@pytest.mark.parametrize("N,S", R.RAYS_SIZES)
def test_rays_bwd(dev, N, S, use_bound):
    """rays_bwd_kernel on its own, with both normalisations (synth.config_headline's bound, synth.config_large_submap's
    localMLP_max_len); the incoming gradient spans 2^-10 .. 2^10"""
    case = R.make_case(N, S, 1000 + S, emd_w=0.0, rgb_missing=0, use_bound=use_bound)
    cfg = case["cfg"]
    assert bool(cfg["grid"]["use_bound_normalize"]) == use_bound
    gen = torch.Generator().manual_seed(S + N)
    dxn = torch.exp2(20.0 * torch.rand(N * S, 3, generator=gen) - 10.0) * (2.0 * torch.randint(0, 2, (N * S, 3), generator=gen) - 1.0)
    rc = ops.make_render_cfg(cfg, cfg["mapping"]["bound"], cfg["mapping"]["localMLP_max_len"], S, 0, 0.0)
    d_o, d_d = ops.rays_bwd(dxn.to(dev), case["z"].to(dev), rc, N, S)
    ref, y32 = R.rays_bwd_reference(dxn, case["z"], cfg), R.rays_bwd_reference(dxn, case["z"], cfg, torch.float32)
    tag = f"N{N}-S{S}-{'bound' if use_bound else 'max_len'}"
    for name, a, r, y in (("d rays_o", d_o, ref[0], y32[0]), ("d rays_d", d_d, ref[1], y32[1])):
        check_grad("rays_bwd", tag, a, r, y, ((name, slice(0, 3)),))
