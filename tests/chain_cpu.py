"""Inputs and the float64 answer for the training step AS JointEncoding.forward_from_table AND forward COMPOSE IT: the row gather,
the pose path, placement, normalisation, hash grid, decoder, render and losses, and back through all of them to the table, the
decoder, the poses and the rays.  No tests here and no GPU: tests/test_chain_cpu.py holds this helper to its conditions,
tests/test_gpu_chain_fp64.py holds the kernels to it.

The chain (``chain``) is float64 throughout with two exceptions, the two casts the upstream fixes by format and the kernels
reproduce bit for bit: ``z_vals`` (path_cpu.place_samples in fp32) and the fp32 cast of the normalised points at the grid's input.
It is composed of the links the unit tests already hold: step_cpu.pose_rays, path_cpu.place_samples / ray_points / normalise_points,
hashgrid_cpu.reference, decoder_cpu.encoding / forward / backward, render_cpu._composite, path_cpu.sdf_losses, CpuScene.train_forward's
loss lines and path_cpu.total_loss.  The yardstick (``yardstick``) is the same step in the oracle's own formats: path_cpu.CpuScene in
fp32 with autograd and the reference's ray composition; e32 is its distance from the chain.

A composed step cannot sit on a lattice, so its decisions are kept clear of rounding by PER-RAY REJECTION (``build_case``): rays are
independent in the forward pass, the builder draws candidate rays (a table row and its jitter row) from a seeded generator and keeps
one only if float64 says every decision of that ray holds with a margin:

  ReLU            every H1 and G3 pre-activation >= decoder_cpu.THRESHOLD (1e-5) in magnitude
  first crossing  every |sdf| up to and including the crossing pair (every sample of a ray without a crossing) >= render_cpu.CEIL_VALUE
                  (1e-4): a kernel inside its unit gate moves an SDF by less than that ceiling, so it cannot flip a sign
  keep/front/back z against z_first + band, d - T and d + T: apart by at least ULPS (8) fp32 ulps of the larger operand
  grid cell       at every level and axis pos = x * scale + 0.5 is at least CELL_MARGIN * (scale + 1) from an integer: the cell decides
                  which entries get a gradient, and the Jacobian jumps across it.  CELL_MARGIN: see below

A comparison then needs no allowance for flipped decisions and no outliers.  The cap is a condition: at most CAP (256) candidates per
ray.  Planted rays (no depth, beyond depth_trunc, no crossing) go through the same filter.

CELL_MARGIN.  The issue's figure is 2^-20, on the condition that the fp32 yardstick's xn lie within a quarter of it of the chain's.
They do not: the yardstick forms the pose, the rays and the sample points in fp32 (world coordinates up to 7: an ulp of 4.8e-7) before the
float64 normalisation, and lands up to 2^-21.42 * (scale + 1) from the chain's pos (N33-S64; tests/test_chain_cpu.py prints the figure per
case and asserts both halves of this paragraph).  The margin is therefore four times what the yardstick shows, rounded up to a power of
two: 2^-19.  The camera positions are held to the same margin (a ray without depth has its first sample AT the camera).

``chain(case, mutation=...)`` computes a planted seam defect instead (MUTATIONS); tests/test_chain_cpu.py shows that every one of them
moves some compared group by ten working gates on some case."""
import copy
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from mipsfusion_amd import ops, synth
from mipsfusion_amd.helper_functions.geometry_helper import matrix_to_quaternion, qt_to_transform_matrix
from oracle import path_cpu, tcnn_cpu

from . import decoder_cpu, hashgrid_cpu, render_cpu, step_cpu
from .render_cpu import CEIL_GRAD, CEIL_VALUE, FLT_MIN, GATE_FACTOR, GATE_FLOOR, working_gate  # noqa: F401 (re-exported)

PLS = float(2.0 ** (math.log2(256 / 16) / 15))
HASH_LOG2 = 16                         # dense levels (0 .. 3) and hashed levels both occur
CAP = 256                              # candidates per ray, at most
ULPS = 8
CELL_MARGIN = 2.0 ** -19               # see the module docstring
CELL_MARGIN_ISSUE = 2.0 ** -20
DEPTH_TRUNC = 3.5
TILE = 32
LOSS_NAMES = render_cpu.LOSS_NAMES
MUTATIONS = ("mask_shift", "crossing_plus_one", "straddle", "counts_swapped", "drop_ragged_tile", "owner_plus_one")

# name -> n_uniform, n_near, N, F, K, emd_w, use_bound, owner pattern, depth mode, planted.  seed: added to the case's seeds, chosen by hand
# for N1-S16 as decoder_cpu.SEEDS is where the first seed left the yardstick without headroom: seed 0 gives a depth loss of 1.3e-6 (the
# square of a millimetre on ONE ray), which the fp32 yardstick itself misses by 1.6e-4 of its value -- above the ceiling for a value
SPECS = {
    "N1-S16": dict(nu=0, nn=16, N=1, F=0, K=1, emd=0.01, bound=True, owner="optimised", seed=2),
    "N5-S33": dict(nu=22, nn=11, N=5, F=1, K=2, emd=0.01, bound=True, owner="mixed"),
    "N17-S64": dict(nu=43, nn=21, N=17, F=2, K=2, emd=0.01, bound=True, owner="alternate",
                    planted={3: "no_depth", 4: "no_depth_negative", 5: "beyond_trunc", 6: "no_crossing"}),
    "N17-S75": dict(nu=50, nn=25, N=17, F=1, K=2, emd=0.0, bound=False, owner="last_fixed"),
    "N33-S64": dict(nu=43, nn=21, N=33, F=0, K=3, emd=0.01, bound=True, owner="two_of_three"),
    "N16-S129": dict(nu=86, nn=43, N=16, F=2, K=1, emd=0.01, bound=True, owner="one_optimised"),
    "N8-S64-fixed": dict(nu=43, nn=21, N=8, F=2, K=1, emd=0.01, bound=True, owner="all_fixed"),
    "N17-S64-nodepth": dict(nu=43, nn=21, N=17, F=1, K=2, emd=0.01, bound=True, owner="mixed", depth="none"),
}
CASES = tuple(SPECS)
FORM_CASES = ("N5-S33", "N17-S64", "N17-S75", "N16-S129")       # where the further forms of the GPU test run


def _owner(pattern, N, F, K):
    n = torch.arange(N)
    if pattern == "optimised":
        return F + n % K
    if pattern == "mixed":                  # fixed and optimised poses in turn, every pose owning a ray where N allows
        return n % (F + K)
    if pattern == "alternate":              # fixed, optimised, fixed, optimised ...: the mask changes at every ray
        return torch.where(n % 2 == 0, (n // 2) % F, F + (n // 2) % K)
    if pattern == "last_fixed":
        o = F + n % K
        o[-1] = 0
        return o
    if pattern == "two_of_three":           # the last optimised pose owns no ray
        return F + n % (K - 1)
    if pattern == "one_optimised":          # one ray in three belongs to the optimised pose
        return torch.where(n % 3 == 1, torch.full_like(n, F), (n // 3) % F)
    if pattern == "all_fixed":
        return n % F
    raise ValueError(pattern)


def levels():
    return hashgrid_cpu.Levels(tcnn_cpu.make_grid_meta(16, 2, HASH_LOG2, 16, PLS))


def case_cfg(spec):
    cfg = copy.deepcopy(synth.config_headline() if spec["bound"] else synth.config_large_submap())
    cfg["grid"]["hash_size"] = HASH_LOG2
    cfg["cam"]["depth_trunc"] = DEPTH_TRUNC
    cfg["training"].update(n_samples_d=spec["nu"], n_range_d=spec["nn"], n_samples=spec["nu"] + spec["nn"])
    # the base config's depth weight is 0: with 0.1 the depth loss's gradient is part of the objective.  The batch without a valid depth
    # keeps 0: its depth loss is 0 / 0, and a weight of exactly 0 on it is NaN in the objective and adds no gradient
    cfg["training"]["depth_weight"] = 0.0 if spec.get("depth") == "none" else 0.1
    return cfg


def ulp32(v):
    """the fp32 ulp of |v| (float64 tensor in, float64 out)"""
    a = v.abs().clamp_min(FLT_MIN)
    return torch.exp2(torch.floor(torch.log2(a)) - 23.0)


# ------------------------------------------------------------------------------------------------- the forward links
def _static(name):
    """what does not depend on the rays: cfg, the table, the decoder, the poses"""
    spec = SPECS[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 4000 + spec.get("seed", 0))
    cfg = case_cfg(spec)
    lv = levels()
    params = (torch.randn(2 * lv.n_entries, generator=gen) * 0.2).numpy()
    weights = decoder_cpu.make_weights(3 + len(name))
    Fn, K = spec["F"], spec["K"]
    scales = torch.from_numpy(lv.scales.astype(np.float64))
    poses = []
    for k in range(Fn + K):
        c2w = synth.default_pose(cfg, yaw=0.3 + 0.12 * k, pitch=-0.1 + 0.02 * k)
        c2w[:3, 3] += torch.tensor([0.05 * k, 0.08 * k, 0.0])
        # a ray without depth has its first sample AT the camera (z = 0 whatever the jitter): the camera's own grid cell is held to the
        # cell margin here, by the same rejection
        for _ in range(CAP):
            t = c2w[:3, 3] + 0.1 * (2.0 * torch.rand(3, generator=gen) - 1.0)
            pos = normalise(t.double()[None], cfg)[0, None, :] * scales[:, None] + 0.5
            if float(((pos - torch.round(pos)).abs() / (scales[:, None] + 1.0)).min()) >= 2.0 * CELL_MARGIN:
                break
        else:
            raise AssertionError(f"{name}: pose {k} found no translation within the cell margin")
        c2w[:3, 3] = t
        poses.append(c2w)
    poses = torch.stack(poses)
    fixed = poses[:Fn].clone()
    # quaternions as Adam steps leave them: a little off the unit sphere
    rot = matrix_to_quaternion(poses[Fn:, :3, :3]).to(torch.float32) * (1.0 + 1e-3 * torch.randn(K, 1, generator=gen))
    trans = poses[Fn:, :3, 3].clone()
    return dict(name=name, spec=spec, cfg=cfg, levels=lv, params=params, weights=weights, fixed=fixed, rot=rot, trans=trans,
                owner=_owner(spec["owner"], spec["N"], Fn, K), emd_w=float(spec["emd"]), S=spec["nu"] + spec["nn"])


def normalise(pts64, cfg):
    b, h = step_cpu.bound64(cfg)
    return path_cpu.normalise_points(pts64, cfg["grid"], b, h) / cfg["training"]["norm_factor"]


def forward_rays(st, rays7, noise, owner, rot=None, trans=None):
    """The forward links for rays that are rows ``rays7`` [n,7] with jitter ``noise`` [n,S] seen from poses ``owner`` [n]; rot / trans:
    float64 leaves (default: the case's own, detached).  -> dict: rays_o, rays_d (float64), z (fp32), xn64, xn (fp32), grid (the
    hashgrid_cpu.reference dict), dec (decoder_cpu.forward's dict), raw [n,S,10] float64"""
    cfg, n, S = st["cfg"], rays7.shape[0], st["S"]
    rot = st["rot"].double() if rot is None else rot
    trans = st["trans"].double() if trans is None else trans
    ro, rd = step_cpu.pose_rays(rot, trans, st["fixed"].double(), owner, rays7[:, :3].double())
    target_d = rays7[:, 6:7].contiguous()
    z = path_cpu.place_samples(n, target_d, cfg["training"], cfg["cam"], noise)            # fp32: the first cast
    assert z.dtype == torch.float32
    xn64 = normalise(path_cpu.ray_points(ro, rd, z.double()).double(), cfg)
    xn = xn64.detach().to(torch.float32)                                                   # the second cast
    grid = hashgrid_cpu.reference(st["levels"], xn.numpy(), st["params"])
    feat = torch.from_numpy(grid["y"].reshape(n * S, 32))
    w64 = [t.double() for t in st["weights"]]
    pe, dpe_dx = decoder_cpu.encoding(xn, torch.float64)
    dec = decoder_cpu.forward(w64, feat, xn.double(), pe)
    dec["dpe_dx"], dec["feat"] = dpe_dx, feat
    return dict(rays_o=ro, rays_d=rd, z=z, xn64=xn64, xn=xn, grid=grid, dec=dec, raw=dec["out"].reshape(n, S, 10), target_d=target_d)


def first_crossing(sdf):
    crossing = (sdf[:, 1:] * sdf[:, :-1]) < 0.0
    return torch.argmax(crossing.to(sdf.dtype), dim=1), crossing.any(1)


def margins(st, fw):
    """-> dict of per-ray float64 margins, each as a RATIO to what build_case asks (>= 1: kept): relu, crossing, compare, cell; and
    ``first``, ``any_crossing``"""
    cfg, S = st["cfg"], st["S"]
    n = fw["z"].shape[0]
    tr, sc = cfg["training"]["trunc"], cfg["data"]["sc_factor"]
    T = tr * sc
    dec = fw["dec"]
    relu = torch.minimum(dec["H1"].abs().min(1).values, dec["G3"].abs().min(1).values).reshape(n, S).min(1).values
    sdf = fw["raw"][..., 3]
    first, any_c = first_crossing(sdf)
    upto = torch.where(any_c, first + 1, torch.full_like(first, S - 1))
    s = torch.arange(S)[None]
    cross = torch.where(s <= upto[:, None], sdf.abs(), torch.full_like(sdf, float("inf"))).min(1).values
    z, d = fw["z"].double(), fw["target_d"].double()
    comp = torch.full((n,), float("inf"), dtype=torch.float64)
    for other in (torch.gather(z, 1, first[:, None]) + sc * tr, d - T, d + T):
        gap = (z - other).abs() / (ULPS * ulp32(torch.maximum(z.abs(), other.abs().expand_as(z))))
        comp = torch.minimum(comp, gap.min(1).values)
    scales = torch.from_numpy(st["levels"].scales.astype(np.float64))
    pos = fw["xn"].double()[:, None, :] * scales[None, :, None] + 0.5                      # [M,L,3]
    cell = ((pos - torch.round(pos)).abs() / (scales[None, :, None] + 1.0)).reshape(n, -1).min(1).values
    return dict(relu=relu / decoder_cpu.THRESHOLD, crossing=cross / CEIL_VALUE, compare=comp, cell=cell / CELL_MARGIN,
                first=first, any_crossing=any_c)


# ------------------------------------------------------------------------------------------------------- the builder
def _candidates(st, gen, slots):
    """one candidate for every slot in ``slots``: a table row (direction in the camera frame | rgb | depth) and a jitter row"""
    spec, S = st["spec"], st["S"]
    n = len(slots)
    row = torch.empty(n, 7)
    row[:, :3] = torch.randn(n, 3, generator=gen) * torch.tensor([0.5, 0.4, 0.1]) + torch.tensor([0.0, 0.0, 1.0])
    row[:, 3:6] = torch.rand(n, 3, generator=gen)
    row[:, 6] = 0.4 + 2.9 * torch.rand(n, generator=gen)                                   # 0.4 .. 3.3: valid
    beyond = DEPTH_TRUNC + 0.1 + 0.8 * torch.rand(n, generator=gen)
    noise = torch.rand(n, S, generator=gen)
    planted = spec.get("planted", {})
    for i, slot in enumerate(slots):
        kind = planted.get(slot)
        if spec.get("depth") == "none":
            kind = ("no_depth", "beyond_trunc", "no_depth_negative")[slot % 3]
        elif kind is None and slot % 5 == 2:
            kind = "beyond_trunc"                                                          # (beside the planted ones)
        if kind == "no_depth":
            row[i, 6] = 0.0
        elif kind == "no_depth_negative":
            row[i, 6] = -0.5
        elif kind == "beyond_trunc":
            row[i, 6] = beyond[i]
        elif kind == "no_crossing":
            row[i, :3] *= 0.002                # a ray a few centimetres long: the SDF keeps one sign along it (the filter checks it)
    return row, noise


def ray_kind(st, slot):
    spec = st["spec"]
    if spec.get("depth") == "none":
        return ("no_depth", "beyond_trunc", "no_depth_negative")[slot % 3]
    return spec.get("planted", {}).get(slot, "beyond_trunc" if slot % 5 == 2 else "valid")


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> dict: the static parts (``_static``), ``table`` [2, R/2, 7] fp32 (the kept rows scattered among others), ``rows`` [N] int64
    (some python-style negative), ``noise`` [N,S], ``tried`` [N] candidates per ray, ``share`` (accepted / tried)"""
    st = dict(_static(name))
    N, S = st["spec"]["N"], st["S"]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + st["spec"].get("seed", 0))
    rays7, noise = torch.zeros(N, 7), torch.zeros(N, S)
    tried = torch.zeros(N, dtype=torch.long)
    open_ = list(range(N))
    for _ in range(CAP):
        if not open_:
            break
        row, nz = _candidates(st, gen, open_)
        fw = forward_rays(st, row, nz, st["owner"][open_])
        m = margins(st, fw)
        ok = (m["relu"] >= 1) & (m["crossing"] >= 1) & (m["compare"] >= 1) & (m["cell"] >= 1)
        for i, slot in enumerate(open_):
            if ray_kind(st, slot) == "no_crossing":
                ok[i] &= ~m["any_crossing"][i]
            elif st["spec"].get("depth") != "none" and slot == 0 and N > 1:
                ok[i] &= m["any_crossing"][i]                                              # at least one ray with a crossing
        tried[open_] += 1
        for i, slot in enumerate(open_):
            if ok[i]:
                rays7[slot], noise[slot] = row[i], nz[i]
        open_ = [slot for i, slot in enumerate(open_) if not ok[i]]
    assert not open_, f"{name}: rays {open_} found no candidate within the margins in {CAP} draws"
    R = 2 * (N + 2)
    perm = torch.randperm(R, generator=gen)[:N]
    table = torch.randn(R, 7, generator=gen)
    table[perm] = rays7
    rows = perm.clone()
    rows[1::2] -= R
    st.update(table=table.reshape(2, R // 2, 7).contiguous(), rows=rows, noise=noise, tried=tried, share=N / float(tried.sum()), N=N)
    return st


def rays_of(case):
    return case["table"].reshape(-1, 7)[case["rows"]]


# ------------------------------------------------------------------------------------------------------- the chain
def _composite(raw, z, trunc, sc_factor, shift_first=0):
    """render_cpu._composite; shift_first != 0 (a mutation): path_cpu.sdf_to_weights' lines with the first-crossing index moved"""
    if not shift_first:
        return render_cpu._composite(raw, z, trunc, sc_factor)
    sdf = raw[..., 3]
    w = torch.sigmoid(sdf / trunc) * torch.sigmoid(-sdf / trunc)
    first, _ = first_crossing(sdf)
    first = (first + shift_first).clamp(0, z.shape[1] - 1)
    keep = (z < torch.gather(z, 1, first[:, None]) + sc_factor * trunc).to(sdf.dtype)
    w = w * keep
    w = w / (w.sum(-1, keepdim=True) + 1e-8)
    rgb = torch.sigmoid(raw[..., :3])
    return dict(rgb=(w[..., None] * rgb).sum(-2), depth=(w * z).sum(-1))


def render_link(cfg, raw, z, target_rgb, target_d, emd_w, mutation=None):
    """raw [N,S,10] float64 (a leaf) -> rgb, depth, the eight loss entries, the objective (path_cpu.total_loss) and counts [N,2]"""
    tr, cam, sc = cfg["training"], cfg["cam"], cfg["data"]["sc_factor"]
    T = tr["trunc"] * sc
    rend = _composite(raw, z, tr["trunc"], sc, 1 if mutation == "crossing_plus_one" else 0)
    # CpuScene.train_forward's lines
    d = target_d.squeeze(-1)
    valid = (d > 0.0) & (d < cam["depth_trunc"])
    rgb_w = valid.clone().unsqueeze(-1)
    rgb_w[rgb_w == 0] = tr["rgb_missing"]
    rgb_loss = F.mse_loss(rend["rgb"] * rgb_w, target_rgb * rgb_w)
    psnr = -10.0 * torch.log(rgb_loss) / math.log(10.0)
    depth_loss = F.mse_loss(rend["depth"][valid], d[valid]) if bool(valid.any()) else (rend["depth"].sum() * 0.0 + float("nan"))
    sdf, prob = raw[..., 3], raw[..., 5:]
    fs_loss, sdf_loss = path_cpu.sdf_losses(z, target_d, sdf, prob, T, 5, emd_w)
    front, _, band = masks(z, target_d, T, torch.float64)
    counts = torch.stack([front.sum(1), band.sum(1)], 1).to(torch.int32)
    n_front, n_band = counts[:, 0].sum().double(), counts[:, 1].sum().double()
    fs_weight, sdf_weight = 1.0 - n_front / (n_front + n_band), 1.0 - n_band / (n_front + n_band)
    if mutation == "counts_swapped":
        # the weighted squared-error parts alone (emd_w = 0), re-weighted with the two counts exchanged; the EMD parts are unweighted
        fs0, sd0 = path_cpu.sdf_losses(z, target_d, sdf, prob, T, 5, 0.0)
        fs_loss = fs0 * (sdf_weight / fs_weight) + (fs_loss - fs0)
        sdf_loss = sd0 * (fs_weight / sdf_weight) + (sdf_loss - sd0)
        fs_weight, sdf_weight = sdf_weight, fs_weight
    ret = dict(rgb=rend["rgb"], depth=rend["depth"], rgb_loss=rgb_loss, depth_loss=depth_loss, sdf_loss=sdf_loss, fs_loss=fs_loss)
    losses = torch.stack([rgb_loss, depth_loss, sdf_loss, fs_loss, psnr, fs_weight, sdf_weight, valid.sum().double()]).detach()
    return ret, losses, path_cpu.total_loss(ret, tr), counts


def masks(z, target_d, T, dtype):
    """front, back, band of the losses (path_cpu.sdf_losses' three lines) in ``dtype``"""
    z, d = z.to(dtype), target_d.to(dtype)
    T = torch.tensor(T, dtype=dtype)
    front = z < d - T
    back = z > d + T
    return front, back, ~front & ~back & (d > 0.0)


def tile_facts(N, S):
    """-> (tiles, tiles that hold samples of two or more rays, the ragged remainder M mod 32)"""
    M = N * S
    tiles = (M + TILE - 1) // TILE
    ray = torch.arange(M) // S
    strad = sum(int(ray[t * TILE] != ray[min(M, t * TILE + TILE) - 1]) for t in range(tiles))
    return tiles, strad, M % TILE


def chain(case, mutation=None):
    """The float64 answer of one training step (``mutation``: a planted seam defect instead).  -> dict:
    rgb [N,3], depth [N], losses [8] (LOSS_NAMES), total, z_vals [N,S] fp32, counts [N,2] int32, xn [M,3] fp32, raw [N,S,10], draw [M,10],
    dfeat [M,32], dxn [M,3] (of every sample, unmasked), wants_dx [N] bool, entries [E] / dp [E,2] (the table gradient: every entry a
    corner lands on), grads (the ten decoder gradients, ops.DECODER_PARAM_ORDER), d_rot [K,4], d_trans [K,3], d_rays_o / d_rays_d [N,3]
    (of every ray, as the two-launch entry forms them), and the intermediates the link tests need (fw)"""
    assert mutation is None or mutation in MUTATIONS
    cfg, N, S = case["cfg"], case["N"], case["S"]
    M = N * S
    Fn, K = case["spec"]["F"], case["spec"]["K"]
    rays7, owner = rays_of(case), case["owner"]
    rot = case["rot"].double().clone().requires_grad_(True)
    trans = case["trans"].double().clone().requires_grad_(True)
    fw = forward_rays(case, rays7, case["noise"], owner, rot, trans)
    z64 = fw["z"].double()
    raw = fw["raw"].detach().clone().requires_grad_(True)
    ret, losses, total, counts = render_link(cfg, raw, z64, rays7[:, 3:6].double(), fw["target_d"].double(), case["emd_w"], mutation)
    (draw,) = torch.autograd.grad(total, raw)
    draw = draw.reshape(M, 10)
    w64 = [t.double() for t in case["weights"]]
    dec = fw["dec"]
    back = decoder_cpu.backward(w64, dec["feat"], dec, dec["dpe_dx"], draw)
    back_p = back
    if mutation == "drop_ragged_tile" and M % TILE:
        cut = draw.clone()
        cut[M - M % TILE:] = 0.0
        back_p = decoder_cpu.backward(w64, dec["feat"], dec, dec["dpe_dx"], cut)
    grid_p = hashgrid_cpu.reference(case["levels"], fw["xn"].numpy(), case["params"], back_p["dfeat"].numpy().reshape(M, 16, 2))
    grid_x = grid_p if back_p is back else hashgrid_cpu.reference(case["levels"], fw["xn"].numpy(), case["params"],
                                                                  back["dfeat"].numpy().reshape(M, 16, 2))
    dxn = back["dx"] + torch.from_numpy(grid_x["dx"])                                       # d objective / d xn (fp32 cast: identity)
    # ---- the rays: xn = ((o + d z) - lo) / div / norm_factor
    b, h = step_cpu.bound64(cfg)
    div = ((b[:, 1] - b[:, 0]) if cfg["grid"]["use_bound_normalize"] else 2 * h) * cfg["training"]["norm_factor"]
    ray_of = torch.arange(M) // S
    if mutation == "straddle":
        starts = torch.arange(1, N) * S
        starts = starts[starts % TILE != 0]                                                 # the tile of this sample began in the previous ray
        ray_of[starts] -= 1
    g = dxn / div
    d_o = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, ray_of, g)
    d_d = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, ray_of, g * z64.reshape(M, 1))
    true_ray = torch.arange(M) // S
    mag_o = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, true_ray, g.abs())
    mag_d = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, true_ray, (g * z64.reshape(M, 1)).abs())
    # ---- the poses: the rays of the fixed poses are masked (forward_from_table: wants_dx), the others go through the pose chain
    wants = (owner % (Fn + K)) >= Fn
    use = wants.clone()
    if mutation == "mask_shift":
        use = torch.cat([use[:1], use[:-1]])
    own = owner % (Fn + K)
    ro, rd = fw["rays_o"], fw["rays_d"]
    if mutation == "owner_plus_one":
        # pose k collects the rays of pose k + 1 (the last optimised pose none)
        own = torch.where(own > Fn, own - 1, torch.where(own == Fn, torch.zeros_like(own), own))
        use = use & ((owner % (Fn + K)) > Fn)
        ro, rd = step_cpu.pose_rays(rot, trans, case["fixed"].double(), own, rays7[:, :3].double())
    obj = ((ro * d_o + rd * d_d) * use[:, None].double()).sum()
    if obj.requires_grad and bool(use.any()):
        d_rot, d_trans = torch.autograd.grad(obj, (rot, trans), allow_unused=True)
    else:
        d_rot = d_trans = None
    d_rot = torch.zeros(K, 4, dtype=torch.float64) if d_rot is None else d_rot
    d_trans = torch.zeros(K, 3, dtype=torch.float64) if d_trans is None else d_trans
    if mutation == "counts_swapped":
        counts = counts.flip(1)
    return dict(rgb=ret["rgb"].detach(), depth=ret["depth"].detach(), losses=losses, total=total.detach(), z_vals=fw["z"], counts=counts,
                xn=fw["xn"], raw=raw.detach(), draw=draw, dfeat=back["dfeat"], dxn=dxn, wants_dx=wants, entries=grid_p["entries"],
                dp=grid_p["dp"], grads=back_p["grads"], d_rot=d_rot, d_trans=d_trans, d_rays_o=d_o, d_rays_d=d_d, mag_rays_o=mag_o, mag_rays_d=mag_d, fw=fw,
                back=back)


@functools.lru_cache(maxsize=None)
def answer(name):
    """the chain of a case, computed once a process and never written to"""
    return chain(build_case(name))


def table_grad(c64, lv):
    """the chain's table gradient as a dense float64 array [entries, 2] and the mask of the entries a corner lands on"""
    dense = np.zeros((lv.n_entries, 2))
    dense[c64["entries"]] = c64["dp"]
    hit = np.zeros(lv.n_entries, bool)
    hit[c64["entries"]] = True
    return dense, hit


# --------------------------------------------------------------------------------------------------- the yardstick
def cpu_scene(case):
    cfg = case["cfg"]
    bb, nf = torch.tensor(cfg["mapping"]["bound"]), torch.tensor(cfg["mapping"]["localMLP_max_len"])
    cpu = path_cpu.CpuScene(cfg, bb, nf)
    with torch.no_grad():
        cpu.embed_fn.params.copy_(torch.from_numpy(case["params"]))
        named = dict(cpu.decoder.named_parameters())
        for k, w in zip(ops.DECODER_PARAM_ORDER, case["weights"]):
            named[k].copy_(w)
    return cpu


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """the same step in the oracle's own formats: CpuScene in fp32 with autograd and the reference's ray composition
    (mipsfusion.py:320-322), as tests/test_gpu_configs.py::test_config2_full_iteration_vs_oracle builds it.  -> a dict with chain's keys
    (fp32 values), and ``pre`` (the fp32 H1 / G3 of its own points, for the ReLU decisions)"""
    case = build_case(name)
    cfg, N, S = case["cfg"], case["N"], case["S"]
    cpu = cpu_scene(case)
    rays, owner = rays_of(case), case["owner"]
    rot = case["rot"].clone().requires_grad_(True)
    trans = case["trans"].clone().requires_grad_(True)
    poses_all = torch.cat([case["fixed"], qt_to_transform_matrix(rot, trans)], 0)
    rd = torch.sum(rays[:, None, None, :3] * poses_all[owner, None, :3, :3], -1).reshape(-1, 3)
    ro = poses_all[owner, :3, -1]
    ro.retain_grad(), rd.retain_grad()
    ref = cpu.train_forward(ro, rd, rays[:, 3:6], rays[:, 6:7], case["noise"], case["emd_w"])
    path_cpu.total_loss(ref, cfg["training"]).backward()
    z = ref["z_vals"].detach()
    xn = step_cpu.place_xn(ro.detach(), rd.detach(), z, cfg)
    T = cfg["training"]["trunc"] * cfg["data"]["sc_factor"]
    front, _, band = masks(z, rays[:, 6:7], T, torch.float32)
    counts = torch.stack([front.sum(1), band.sum(1)], 1).to(torch.int32)
    n_front, n_band = counts[:, 0].sum().float(), counts[:, 1].sum().float()
    d = rays[:, 6]
    n_valid = ((d > 0.0) & (d < cfg["cam"]["depth_trunc"])).sum().float()
    losses = torch.stack([ref["rgb_loss"], ref["depth_loss"], ref["sdf_loss"], ref["fs_loss"], ref["psnr"], 1.0 - n_front / (n_front + n_band),
                          1.0 - n_band / (n_front + n_band), n_valid]).detach()
    feat = tcnn_cpu.hashgrid_forward(xn, cpu.embed_fn.params.detach(), cpu.embed_fn.meta)
    pre = decoder_cpu.evaluate(case["weights"], feat, xn, None, torch.float32)
    named = dict(cpu.decoder.named_parameters())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    return dict(rgb=ref["rgb"].detach(), depth=ref["depth"].detach(), losses=losses, z_vals=z, counts=counts, xn=xn, raw=ref["raw"].detach(),
                table=cpu.embed_fn.params.grad.detach().reshape(-1, 2), grads=[zero(named[k]) for k in ops.DECODER_PARAM_ORDER],
                d_rot=zero(rot), d_trans=zero(trans), d_rays_o=zero(ro), d_rays_d=zero(rd), pre=pre)


# ----------------------------------------------------------------------------------------------------- comparisons
def _np64(a):
    return a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def _rows(a, ref):
    """largest error of each row over that row's largest reference magnitude; a row that is zero in the reference must be zero"""
    a, ref = _np64(a), _np64(ref)
    a, ref = a.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return render_cpu.group_errors(a, ref, (("g", slice(None)),))["g"]


def _tensor(a, ref):
    a, ref = _np64(a), _np64(ref)
    top = np.abs(ref).max() if ref.size else 0.0
    diff = np.abs(a.reshape(ref.shape) - ref)
    if not diff.size or diff.max() == 0.0:
        return 0.0, -1
    w = int(diff.argmax())
    return (float(diff.reshape(-1)[w] / top) if top > 0 else float("inf")), w


VALUE_GROUPS = ("rgb", "depth") + tuple(LOSS_NAMES)


def errors(res, c64, lv, entry="table"):
    """{group: (largest error, place)} of ``res`` -- a kernel run's results or the yardstick's, tensors on the host: rgb, depth, losses [8],
    table [entries, 2], grads (ten), d_rot, d_trans; d_rays_o / d_rays_d where it has them -- against the chain ``c64``:
      rgb, depth         per ray over that ray's largest float64 magnitude (place: the ray)
      the loss entries   relative; NaN places must coincide (asserted)
      table              element by element over the tensor's largest float64 magnitude (place: the flat element)
      decoder gradients  per tensor, the same
      d_rot, d_trans     per pose over that row's largest magnitude (place: the pose); a pose without a ray: exactly zero or inf
      d_rays_o, d_rays_d per ray over that ray's largest SUM OF TERM MAGNITUDES (mag_rays_*: sum over the ray's samples of |d xn| / div, and
                         of |d xn| z / div).  A ray's gradient is a sum of S terms of either sign; over its own magnitude a ray whose terms
                         cancel would be held to what no fp32 sum can give (the yardstick itself is 3e-4 off there at S = 129), over the
                         term magnitudes one misplaced sample still shows as 1 / S of the scale, four orders above the gate"""
    out = {}
    for k in ("rgb", "depth"):
        e = _rows(res[k], c64[k])
        out[k] = (float(e.max()), int(e.argmax()))
    la, lr = _np64(res["losses"]), _np64(c64["losses"])
    assert np.array_equal(np.isnan(la), np.isnan(lr)), f"NaN loss entries {np.isnan(la)} where the chain has {np.isnan(lr)}"
    for i, k in enumerate(LOSS_NAMES):
        if np.isnan(lr[i]) or la[i] == lr[i]:
            out[k] = (0.0, i)
        else:
            out[k] = (float(abs(la[i] - lr[i]) / abs(lr[i])) if lr[i] != 0 else float("inf"), i)
    if "table" in res:
        dense, _ = table_grad(c64, lv)
        out["table"] = _tensor(res["table"], dense)
    if "grads" in res:
        for k, a, r in zip(ops.DECODER_PARAM_ORDER, res["grads"], c64["grads"]):
            out[k] = _tensor(a, r)
    for k in ("d_rot", "d_trans"):
        if k in res and res[k] is not None:
            e = _rows(res[k], c64[k])
            out[k] = (float(e.max()), int(e.argmax())) if e.size else (0.0, -1)
    for k in ("d_rays_o", "d_rays_d"):
        if k in res and res[k] is not None:
            a, r, mag = _np64(res[k]), _np64(c64[k]), _np64(c64["mag_" + k[2:]]).max(1)
            diff = np.abs(a - r).max(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.where(mag > 0, diff / mag, np.where(diff == 0, 0.0, np.inf))
            out[k] = (float(e.max()), int(e.argmax()))
    return out


def ceiling(group):
    return CEIL_VALUE if group in VALUE_GROUPS else CEIL_GRAD


def gate(group, e32):
    """the project's working gate, unchanged: min(max(GATE_FACTOR * e32, GATE_FLOOR), ceiling)"""
    return float(working_gate(e32, ceiling(group)))


@functools.lru_cache(maxsize=None)
def e32(name):
    """{group: the yardstick's error against the chain}"""
    case = build_case(name)
    return {k: v[0] for k, v in errors(yardstick(name), answer(name), case["levels"]).items()}


def place(case, c64, group, where):
    """a failure's place in words: the ray, the sample, the tile, and that place's decision margins from the chain"""
    S = case["S"]
    m = margins(case, c64["fw"])
    if group in ("rgb", "depth", "d_rays_o", "d_rays_d"):
        r = where
        return (f"ray {r} (samples {r * S} .. {r * S + S - 1}, tiles {r * S // TILE} .. {(r * S + S - 1) // TILE}, owner {int(case['owner'][r])}, "
                f"first crossing {int(m['first'][r])}{'' if bool(m['any_crossing'][r]) else ' (none)'}; margins / asked: relu {float(m['relu'][r]):.1f} "
                f"crossing {float(m['crossing'][r]):.1f} compare {float(m['compare'][r]):.1f} cell {float(m['cell'][r]):.1f})")
    if group == "table":
        entry = where // 2
        lv = case["levels"]
        level = int(np.searchsorted(np.asarray(lv.offsets), entry, side="right") - 1)
        idx = c64["fw"]["grid"]["idx"][:, level] + lv.offsets[level]
        samples = np.flatnonzero((idx == entry).any(1))
        return (f"entry {entry} feature {where % 2} (level {level}); corners of samples {samples[:8].tolist()} = rays "
                f"{sorted(set((samples // S).tolist()))[:8]}, tiles {sorted(set((samples // TILE).tolist()))[:8]}")
    if group in ("d_rot", "d_trans"):
        Fn, K = case["spec"]["F"], case["spec"]["K"]
        rays = torch.nonzero((case["owner"] % (Fn + K)) == Fn + where).flatten().tolist()
        return f"optimised pose {where}, rays {rays}"
    return f"element {where}"
