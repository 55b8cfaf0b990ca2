"""Inputs and the float64 answer for the per-ray render, loss and ray-gradient kernels (csrc/render.hip, csrc/render_dev.h).
No tests here: tests/test_render_cpu.py holds this helper to its conditions, tests/test_gpu_render_fp64.py holds the kernels to it.

The answer is oracle/path_cpu.py's ``composite``, ``sdf_to_weights`` and ``sdf_losses`` (dtype-agnostic torch code, anchored
to the reference's recorded values by tests/test_oracle_golden.py) run in float64, with autograd for the gradients; the same
code in fp32 is the yardstick (``reference_dtype``): how far plain fp32 arithmetic lands from float64 on the same inputs.

The inputs are built so that fp32 and float64 take the same branch at every discrete decision (first crossing, keep mask,
front / band masks, valid depth): sample and target depths lie on the lattice of multiples of 2^-8, band = T = 0.125, so
``z_min + band``, ``d - T`` and ``d + T`` are exact in both formats, and every SDF is at least 2^-10 in magnitude (or an exact
zero), so no product of neighbours underflows.  A comparison therefore needs no allowance for "flipped" rays."""
import copy
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from mipsfusion_amd import synth
from oracle import path_cpu

LATTICE = 256                    # depths are k / LATTICE
Z_LO, Z_HI = 64, 896             # z in [0.25, 3.5]
TRUNC, SC_FACTOR, DEPTH_TRUNC = 0.0625, 2.0, 3.0
T_STEPS = 32                     # band = T = TRUNC * SC_FACTOR = 0.125 = T_STEPS / LATTICE
SDF_MIN = 2.0 ** -10
LOSS_NAMES = ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "fs_weight", "sdf_weight", "n_valid")
MAP_NAMES = ("rgb", "depth", "depth_var", "disp_map", "acc_map", "weights")
DRAW_GROUPS = (("colour", slice(0, 3)), ("sdf", slice(3, 4)), ("class", slice(5, 10)))
FLT_MIN = 2.0 ** -126            # below it an fp32 kernel holds no normal number: such a reference entry counts as zero

# the gates of tests/test_gpu_render_fp64.py (the issue's): the project's hard ceilings, and the working gate's two terms
CEIL_VALUE, CEIL_GRAD = 1e-4, 5e-4
GATE_FACTOR, GATE_FLOOR = 8.0, 64 * 2.0 ** -24


def _cases():
    """(N, S, seed, emd_w, rgb_missing): every S with N = 17, every N with S = 64 and S = 192; emd_w and rgb_missing alternate with
    periods 2 and 4, which lets each value meet S <= 64, 64 < S <= 128 and S > 128 (tests/test_render_cpu.py asserts it)."""
    shapes = [(17, s) for s in (1, 2, 63, 64, 65, 127, 128, 129, 192, 255, 256)]
    shapes += [(n, s) for s in (64, 192) for n in (1, 15, 16, 33)]
    return [(n, s, 100 + i, 0.01 if i % 2 == 0 else 0.0, (i // 2) % 2) for i, (n, s) in enumerate(shapes)]


CASES = _cases()
RAYS_SIZES = [(n, s) for s in (1, 64, 65, 256) for n in (1, 17)]
# the batches without depth (with_depths) are made from these: render_train_kernel with two samples per lane (EMD on), and
# render_fwd_kernel's ticket form (rgb_missing on)
EDGE_CASES = [c for c in CASES if c[:2] in ((17, 65), (17, 129))]


def case_id(c):
    return f"N{c[0]}-S{c[1]}-emd{c[3]:g}-miss{c[4]}"


# ------------------------------------------------------------------------------------------------------- inputs
def _sorted_lattice(gen, S, lo, hi):
    return torch.sort(torch.randperm(hi - lo + 1, generator=gen)[:S]).values + lo


def _put(idx, v, after):
    """make lattice value v one of the strictly increasing idx, at a position > after; returns that position"""
    S = idx.numel()
    hit = (idx == v).nonzero()
    if hit.numel():
        return int(hit[0])
    p = int(torch.searchsorted(idx, torch.tensor(v)))
    p = min(p, S - 1)
    assert p > after and (p == 0 or idx[p - 1] < v) and (p == S - 1 or v < idx[p + 1])
    idx[p] = v
    return p


def _signed(gen, n, sign):
    """n SDF values of one sign, magnitudes in [0.05, 1]; for n <= 2 in [0.9, 1.1] (see make_case)"""
    if n <= 2:
        return sign * (0.9 + 0.2 * torch.rand(n, generator=gen))
    return sign * (0.05 + 0.95 * torch.rand(n, generator=gen))


def make_case(N, S, seed, *, emd_w, rgb_missing, use_bound=True):
    """-> dict: fp32 ``raw`` [N,S,10], ``z`` [N,S], ``target_rgb`` [N,3], ``target_d`` [N,1], int32 ``counts`` [N,2], ``cfg`` (the
    dict for ops.make_render_cfg), ``emd_w``, and ``planted``: rule name -> ray index for the planted rays that fit N and S."""
    gen = torch.Generator().manual_seed(seed)
    cfg = synth.config_headline() if use_bound else synth.config_large_submap()
    cfg = copy.deepcopy(cfg)
    cfg["training"].update(trunc=TRUNC, rgb_missing=rgb_missing, n_samples=S)
    cfg["data"]["sc_factor"] = SC_FACTOR
    cfg["cam"]["depth_trunc"] = DEPTH_TRUNC

    raw = torch.randn(N, S, 10, generator=gen)
    sdf = torch.linspace(1.0, -1.0, S)[None] + 0.5 * (torch.rand(N, 1, generator=gen) - 0.5) + 0.1 * torch.randn(N, S, generator=gen)
    sdf = torch.where(sdf.abs() < SDF_MIN, torch.full_like(sdf, SDF_MIN), sdf)
    if S <= 2:
        # A ray that keeps ONE sample has the weight wn = u / (u + 1e-8), and d wn / d sdf holds 1 - wn: in fp32 -- the reference's
        # own included -- that difference is off by about 6 u of itself (2^-24 / (1e-8 / u)), 100 % at u = 0.25.  With |sdf| near 1,
        # u = sigmoid(16) sigmoid(-16) ~ 1e-7 stands beside the 1e-8 and the gradient is one fp32 can compute.
        sdf = (0.9 + 0.2 * torch.rand(N, S, generator=gen)) * torch.tensor([1.0, -1.0])[:S]
    raw[..., 5:] = torch.softmax(raw[..., 5:], -1)
    zi = torch.stack([_sorted_lattice(gen, S, Z_LO, Z_HI) for _ in range(N)])
    di = torch.randint(1, 3 * LATTICE, (N,), generator=gen)                      # d in (0, 3): valid
    far = torch.randint(3 * LATTICE, 4 * LATTICE, (N,), generator=gen)
    n = torch.arange(N)
    di = torch.where(n % 5 == 3, far, di)                                         # d in [3, 4): positive, not valid
    di = torch.where(n % 7 == 6, torch.zeros_like(di), di)                        # every 7th ray: no depth

    planted, r = {}, 0

    def plant(name, min_S):
        nonlocal r
        if r >= N or S < min_S:
            return None
        planted[name] = r
        r += 1
        return r - 1

    if (k := plant("all_positive", 1)) is not None:
        sdf[k] = _signed(gen, S, 1.0)
    if (k := plant("all_negative", 1)) is not None:
        sdf[k] = _signed(gen, S, -1.0)
    if (k := plant("last_pair", 2)) is not None:
        sdf[k] = _signed(gen, S, 1.0)
        sdf[k, S - 1] = -sdf[k, S - 1]
    for edge in (63, 127, 191):                                                   # first crossing on the pair (edge, edge + 1)
        if (k := plant(f"lane_edge_{edge}", edge + 2)) is not None:
            sdf[k] = _signed(gen, S, 1.0)
            sdf[k, edge + 1:] = -sdf[k, edge + 1:]
    if (k := plant("zero_sdf", 6)) is not None:
        # + 0.0 - -0.0 + ... + | - ...: the sign changes THROUGH the zeros, no product is negative there; first crossing later
        kx = max(4, S // 2)
        sdf[k] = _signed(gen, S, 1.0)
        sdf[k, 1], sdf[k, 2], sdf[k, 3] = 0.0, -sdf[k, 2], -0.0
        sdf[k, kx + 1:] = -sdf[k, kx + 1:]
    if (k := plant("z_cut_tie", 2)) is not None:
        kc = (S - 2) // 3
        zi[k] = _sorted_lattice(gen, S, Z_LO, Z_HI - T_STEPS)
        sdf[k] = _signed(gen, S, 1.0)
        sdf[k, kc + 1:] = -sdf[k, kc + 1:]
        _put(zi[k], int(zi[k, kc]) + T_STEPS, kc)
    if (k := plant("band_ties", 2)) is not None:
        a = (S - 2) // 4
        zi[k] = _sorted_lattice(gen, S, Z_LO, Z_HI - 2 * T_STEPS)
        _put(zi[k], int(zi[k, a]) + 2 * T_STEPS, a)
        di[k] = int(zi[k, a]) + T_STEPS
    if (k := plant("saturated", 1)) is not None:
        sdf[k] = 8.0
        sdf[k, S // 2:] = -8.0
    if (k := plant("nothing_in_front", 1)) is not None:
        di[k] = T_STEPS // 2                                                      # 0 < d < 0.25 - T
    if (k := plant("no_depth_near", 1)) is not None:
        # No depth, and samples at z <= T (the one ray that leaves [0.25, 3.5]): neither in front of d - T = -T nor behind
        # d + T = T, so ONLY the condition d > 0 keeps them out of the band.  Everywhere else a ray without depth has all its
        # samples behind d + T, and a band mask without that condition would give the same numbers.
        near = torch.tensor([8, 20, T_STEPS])[-min(3, max(1, S // 2)):]
        zi[k, :near.numel()] = near
        di[k] = 0
    raw[..., 3] = sdf

    return _finish(dict(raw=raw, z=zi.to(torch.float32) / LATTICE, target_rgb=torch.rand(N, 3, generator=gen),
                        target_d=(di.to(torch.float32) / LATTICE)[:, None], cfg=cfg, emd_w=float(emd_w), planted=planted))


def _finish(case):
    """``counts`` by the rule of place_ray (csrc/render.hip): front is z < d - T, band is neither front nor back and d > 0"""
    z, d, T = case["z"], case["target_d"], torch.tensor(TRUNC * SC_FACTOR, dtype=torch.float32)
    front = z < d - T
    back = z > d + T
    band = ~front & ~back & (d > 0)
    case["counts"] = torch.stack([front.sum(1), band.sum(1)], 1).to(torch.int32)
    return case


def with_depths(case, mode):
    """the same case with other target depths: ``"invalid"``: every depth in [3, 4) (no valid depth: depth_loss is 0 / 0),
    ``"none"``: every depth 0 (no valid depth AND counts all zero: the band weights are 0 / 0 too)"""
    c = dict(case)
    N = case["z"].shape[0]
    if mode == "invalid":
        gen = torch.Generator().manual_seed(7)
        c["target_d"] = (torch.randint(3 * LATTICE, 4 * LATTICE, (N, 1), generator=gen).to(torch.float32)) / LATTICE
    elif mode == "none":
        c["target_d"] = torch.zeros(N, 1)
    else:
        raise ValueError(mode)
    return _finish(c)


def share(case, lo, hi):
    """rays [lo, hi) of the case as a batch of their own"""
    c = dict(case)
    for k in ("raw", "z", "target_rgb", "target_d", "counts"):
        c[k] = case[k][lo:hi].contiguous()
    return c


@functools.lru_cache(maxsize=None)
def case_of(key):
    N, S, seed, emd_w, rgb_missing = key
    return make_case(N, S, seed, emd_w=emd_w, rgb_missing=rgb_missing)


# ------------------------------------------------------------------------------------------------- the answer
def _composite(raw, z, trunc, sc_factor):
    if z.shape[1] >= 2:
        return path_cpu.composite(raw, z, trunc, sc_factor)
    # S = 1: no pair of neighbours; torch.argmax refuses the empty row, the kernels take "no crossing" (index 0) as they do
    # for a row of zeros.  composite's own lines with first = 0:
    rgb = torch.sigmoid(raw[..., :3])
    sdf = raw[..., 3]
    w = torch.sigmoid(sdf / trunc) * torch.sigmoid(-sdf / trunc)
    w = w * (z < z[:, :1] + sc_factor * trunc).to(sdf.dtype)
    w = w / (w.sum(-1, keepdim=True) + 1e-8)
    depth = (w * z).sum(-1)
    acc = w.sum(-1)
    return dict(rgb=(w[..., None] * rgb).sum(-2), depth=depth, disp_map=1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc),
                acc_map=acc, depth_var=(w * (z - depth[:, None]) ** 2).sum(-1), weights=w)


def decisions(case, dtype):
    """every discrete decision of the render and the losses, evaluated in ``dtype`` by the oracle's expressions"""
    raw, z, d2 = case["raw"].to(dtype), case["z"].to(dtype), case["target_d"].to(dtype)
    tr, sc = case["cfg"]["training"]["trunc"], case["cfg"]["data"]["sc_factor"]
    sdf = raw[..., 3]
    if z.shape[1] >= 2:
        crossing = (sdf[:, 1:] * sdf[:, :-1]) < 0.0
        first = torch.argmax(crossing.to(dtype), dim=1, keepdim=True)
        any_crossing = crossing.any(1)
    else:
        first = torch.zeros(z.shape[0], 1, dtype=torch.long)
        any_crossing = torch.zeros(z.shape[0], dtype=torch.bool)
    z_cut = torch.gather(z, 1, first) + sc * tr
    truncation = tr * sc
    front = z < d2 - truncation
    back = z > d2 + truncation
    band = ~front & ~back & (d2 > 0.0)
    d = d2.squeeze(-1)
    return dict(first=first.squeeze(1), any_crossing=any_crossing, z_cut=z_cut, keep=z < z_cut, front=front, back=back, band=band,
                valid=(d > 0.0) & (d < case["cfg"]["cam"]["depth_trunc"]))


def reference_dtype(case, dtype, *, g_losses=None, g_rgb=None, g_depth=None, loss_weights=None):
    """The maps (MAP_NAMES), ``losses`` (the eight entries in the order finalize_losses writes them), ``objective`` and ``draw`` =
    d objective / d raw, with objective = sum(loss_weights * four losses) + sum(g_losses * four losses) + (g_rgb * rgb).sum() +
    (g_depth * depth).sum() (the four losses: rgb, depth, sdf, fs -- path_cpu.total_loss's order), all in ``dtype``."""
    cfg = case["cfg"]
    tr, cam, sc = cfg["training"], cfg["cam"], cfg["data"]["sc_factor"]
    raw = case["raw"].detach().to(dtype).clone().requires_grad_(True)        # (a leaf of its own: the case is never written to)
    z, target_rgb, target_d = case["z"].to(dtype), case["target_rgb"].to(dtype), case["target_d"].to(dtype)
    rend = _composite(raw, z, tr["trunc"], sc)
    # CpuScene.train_forward's lines
    d = target_d.squeeze(-1)
    valid = (d > 0.0) & (d < cam["depth_trunc"])
    rgb_w = valid.clone().unsqueeze(-1)
    rgb_w[rgb_w == 0] = tr["rgb_missing"]
    rgb_loss = F.mse_loss(rend["rgb"] * rgb_w, target_rgb * rgb_w)
    psnr = -10.0 * torch.log(rgb_loss) / math.log(10.0)
    depth_loss = F.mse_loss(rend["depth"][valid], d[valid]) if bool(valid.any()) else (rend["depth"].sum() * 0.0 + float("nan"))
    fs_loss, sdf_loss = path_cpu.sdf_losses(z, target_d, raw[..., 3], raw[..., 5:], tr["trunc"] * sc, 5, case["emd_w"])
    # (sdf_losses forms the two band weights in fp32 whatever the dtype; they are reported here in ``dtype`` from the counts)
    n_front, n_band = case["counts"][:, 0].sum().to(dtype), case["counts"][:, 1].sum().to(dtype)
    four = torch.stack([rgb_loss, depth_loss, sdf_loss, fs_loss])
    losses = torch.stack([rgb_loss, depth_loss, sdf_loss, fs_loss, psnr, 1.0 - n_front / (n_front + n_band),
                          1.0 - n_band / (n_front + n_band), valid.sum().to(dtype)]).detach()
    objective = torch.zeros((), dtype=dtype)
    for wts in (loss_weights, g_losses):
        if wts is not None:
            # a weight of exactly 0 on a NaN loss is NaN in the objective (as in the kernel's), and contributes no gradient
            objective = objective + (torch.as_tensor(wts).to(dtype) * four).sum()
    if g_rgb is not None:
        objective = objective + (torch.as_tensor(g_rgb).to(dtype) * rend["rgb"]).sum()
    if g_depth is not None:
        objective = objective + (torch.as_tensor(g_depth).to(dtype) * rend["depth"]).sum()
    out = {k: rend[k].detach() for k in MAP_NAMES}
    out["losses"], out["objective"] = losses, objective.detach()
    if objective.requires_grad:
        g = torch.autograd.grad(objective, [raw, rend["rgb"], rend["depth"]], allow_unused=True)
    else:
        g = (None, None, None)
    out["draw"] = g[0] if g[0] is not None else torch.zeros_like(raw)
    # d objective / d the rendered maps (sdf_cancellation needs them)
    out["g_rgb_map"] = g[1] if g[1] is not None else torch.zeros_like(rend["rgb"])
    out["g_depth_map"] = g[2] if g[2] is not None else torch.zeros_like(rend["depth"])
    return out


def reference(case, **grads):
    """the float64 answer"""
    return reference_dtype(case, torch.float64, **grads)


def rays_bwd_reference(dxn, z, cfg, dtype=torch.float64):
    """float64 d rays_o, d rays_d [N,3] for a gradient ``dxn`` [N*S,3] of the normalised sample points, by autograd through
    path_cpu.ray_points and path_cpu.normalise_points (and the division by training.norm_factor of query_normalised).
    dtype = torch.float32 is the yardstick: rays and sample points in fp32, the normalisation in float64 as the reference has it
    by construction."""
    N = z.shape[0]
    o = torch.zeros(N, 3, dtype=dtype, requires_grad=True)
    d = torch.ones(N, 3, dtype=dtype, requires_grad=True)
    bound64 = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float64)
    half64 = torch.tensor(cfg["mapping"]["localMLP_max_len"], dtype=torch.float64)
    pts = path_cpu.ray_points(o, d, z.to(dtype)).double()
    xn = path_cpu.normalise_points(pts, cfg["grid"], bound64, half64) / cfg["training"]["norm_factor"]
    return torch.autograd.grad((xn * dxn.double().reshape(-1, 3)).sum(), (o, d))


# ------------------------------------------------------------------------------------------------ comparisons
def _np64(a):
    return a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def value_error(a, ref, scale=None):
    """max |a - ref| / scale (default: max |ref|) over the entries where ref is a number; NaN positions must coincide"""
    a, ref = _np64(a), _np64(ref)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), "NaN in other places than the reference's"
    ok = ~np.isnan(ref) & (a != ref)              # (equal entries, infinities included, are no error)
    if not ok.any():
        return 0.0
    if scale is None:
        scale = np.abs(ref[~np.isnan(ref)]).max()
    diff = np.abs(a[ok] - ref[ok]).max()
    if scale == 0.0:
        return float("inf")
    return float(diff / scale)                    # (an infinity on one side only: inf or NaN, above every gate)


def group_errors(a, ref, groups):
    """a, ref: [N, ..., C]; groups: ((name, column slice), ...) -> {name: [N] error of each ray's group, normalised by that ray's
    largest reference magnitude in the group}.  Reference entries below fp32's smallest normal number count as zero; where a
    ray's group is all zero in the reference the error is 0 if ``a`` is all zero there too, else inf.  NaN entries of the
    reference are left out (their places are compared by ``same_nans``)."""
    a, ref = _np64(a), _np64(ref)
    N = ref.shape[0]
    out = {}
    for name, sl in groups:
        x, r = a[..., sl].reshape(N, -1), ref[..., sl].reshape(N, -1).copy()
        nan = np.isnan(r)
        r[np.abs(r) < FLT_MIN] = 0.0
        r[nan], x = 0.0, np.where(nan, 0.0, x)
        scale = np.abs(r).max(1)
        diff = np.abs(x - r).max(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = np.where(scale > 0.0, diff / scale, np.where(diff == 0.0, 0.0, np.inf))
    return out


def working_gate(e32, ceiling, extra=0.0):
    return np.minimum(np.maximum(np.maximum(GATE_FACTOR * np.asarray(e32), GATE_FLOOR), extra), ceiling)


CANCEL_ROUNDINGS = 16            # 3 in G.at, 6 butterfly levels + 4 strided additions + 2 products in dot, the subtraction


def sdf_cancellation(case, r64):
    """[N]: the forward error bound of the one cancelling step of the kernels' column 3 (sample_grad_record, csrc/render_dev.h),
    relative to each ray's largest float64 entry of the column, from float64 quantities alone.

    The kernels form A_k = G.r c0 + G.g c1 + G.b c2 + G.d z (MapGrad::at), dot = sum_j A_j wn_j, and (A_k - dot) * inv * u_k (1 -
    2 sg_k) / trunc.  A_k and dot carry roundings of the size of their terms' MAGNITUDES (|G.r| c0 + ... + |G.d| z and its
    weighted sum), whatever is left of them after the terms and then the difference cancel: with the weight of a ray on one or
    two samples A_k - dot is (1 - wn_k) of A_k or less.  Autograd never forms A_k -- it carries the colour and the depth gradients
    apart -- so the fp32 oracle's e32 does not see this step, and a multiple of e32 cannot bound it.  The bound:
    CANCEL_ROUNDINGS * 2^-24 * (|A|_k + sum_j |A|_j wn_j) * wn_k |1 - 2 sg_k| / trunc."""
    trunc = case["cfg"]["training"]["trunc"]
    raw, z, w = case["raw"].double(), case["z"].double(), r64["weights"]
    c, sg = torch.sigmoid(raw[..., :3]), torch.sigmoid(raw[..., 3] / trunc)
    abs_a = (r64["g_rgb_map"].abs()[:, None, :] * c).sum(-1) + r64["g_depth_map"].abs()[:, None] * z
    bound = (abs_a + (abs_a * w).sum(1, keepdim=True)) * w * (1.0 - 2.0 * sg).abs() / trunc
    top = torch.nan_to_num(r64["draw"][..., 3].abs(), nan=0.0)
    top = torch.where(top < FLT_MIN, torch.zeros_like(top), top).max(1).values
    cond = torch.where(top > 0, bound.max(1).values / top.clamp_min(FLT_MIN), torch.zeros_like(top))
    return (CANCEL_ROUNDINGS * 2.0 ** -24 * cond).numpy()
