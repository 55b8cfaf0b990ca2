"""Inputs and the independent answers for the head and the tail of the training step: sample placement (sample_rays_kernel,
gather_pose_place_kernel: csrc/render.hip place_ray), the pose path (pose_rays_fwd/bwd_kernel, place_pose_bwd_kernel, pose_chain,
pose_block_finish: csrc/pose.hip, csrc/pose_dev.h, csrc/render.hip), the frequency encoding and the normalisation, and Adam
(csrc/elementwise.hip).  No tests here and no GPU: tests/test_step_cpu.py holds this helper to its conditions,
tests/test_gpu_step_fp64.py holds the kernels to it.

The answers are code the repository already has: oracle/path_cpu.py (place_samples, ray_points, normalise_points, adam_reference),
oracle/tcnn_cpu.py (the frequency argument), helper_functions/geometry_helper.qt_to_transform_matrix with torch autograd in float64,
and the mask rule of the losses (path_cpu.sdf_losses: front, back, band).  working_gate, value_error, group_errors, FLT_MIN and the
ceilings are tests/render_cpu.py's."""
import copy
import functools
import math

import numpy as np
import torch

from mipsfusion_amd import synth
from mipsfusion_amd.helper_functions.geometry_helper import quaternion_to_matrix, qt_to_transform_matrix
from oracle import path_cpu, tcnn_cpu

from .render_cpu import CEIL_GRAD, CEIL_VALUE, FLT_MIN, group_errors, value_error, working_gate  # noqa: F401 (re-exported)

U = 2.0 ** -24                       # one fp32 rounding


# ================================================================================================= 1. placement
# Lattice: near 0, far 4, depths k / 16, the depth-guided offsets j / 16 (range_d 0.25, 9 of them), T = trunc * sc_factor = 0.125.
# d - T and d + T are then exact in fp32 and float64 alike, so the two formats decide front / back / band alike on EVERY fp32 z
# (tests/test_step_cpu.py asserts it for every case, no sample left out), lattice or not.
NEAR, FAR = 0, 4
RANGE_D, TRUNC, SC_FACTOR = 0.25, 0.0625, 2.0
T_TOTAL = TRUNC * SC_FACTOR
ONE_BELOW = 1.0 - 2.0 ** -24         # the largest fp32 below 1: the top of torch.rand's range


def place_cfg(n_uniform, n_near, *, perturb, use_bound=True, norm_factor=1.0):
    cfg = copy.deepcopy(synth.config_headline() if use_bound else synth.config_large_submap())
    cfg["cam"].update(near=NEAR, far=FAR)
    cfg["data"]["sc_factor"] = SC_FACTOR
    cfg["training"].update(trunc=TRUNC, n_samples_d=n_uniform, n_range_d=n_near, range_d=RANGE_D, n_samples=n_uniform + n_near,
                           perturb=perturb, norm_factor=norm_factor)
    return cfg


# (name, n_uniform, n_near, N, perturb, use_bound, norm_factor, target): target "depth" | "none" (target_d = None: n_near = 0)
def _place_cases():
    out = []
    # the lattice cases with the planted rays: uniform step 1/8 (33) and 1/4 (17), depth-guided step 1/16
    for i, (nu, pert, ub, nf) in enumerate([(33, 0, True, 1.0), (33, 1, False, 2.0), (17, 0, False, 1.0), (17, 1, True, 2.0)]):
        out.append((f"lattice{nu}-p{pert}-{'bound' if ub else 'len'}-nf{nf:g}", nu, 9, 33, pert, ub, nf, "depth"))
    # n_samples_d = 0: the depth-guided list alone, which the reference does not sort (scene_rep.py:166-167)
    out.append(("near-only-p0", 0, 9, 5, 0, True, 1.0, "depth"))
    out.append(("near-only-p1", 0, 9, 4, 1, False, 2.0, "depth"))
    # target_d = None: n_samples uniform samples, no counts
    out.append(("no-target-p0", 33, 0, 5, 0, True, 2.0, "none"))
    out.append(("no-target-p1", 64, 0, 3, 1, False, 1.0, "none"))
    # the shapes: S in {1, 2, 63, 64, 65, 128, 129, 255, 256}; (0, 1), (1, 0), n_near > n_uniform; N in {1, 3, 4, 5, 33}
    shapes = [(0, 1), (1, 0), (1, 1), (42, 21), (20, 43), (43, 21), (21, 43), (44, 21), (85, 43), (86, 43), (170, 85), (171, 85)]
    ns = (1, 3, 4, 5, 33)
    for i, (nu, nn) in enumerate(shapes):
        out.append((f"S{nu + nn}-{nu}+{nn}-N{ns[i % 5]}-p{i % 2}", nu, nn, ns[i % 5], i % 2, i % 3 != 0, 2.0 if i % 4 == 1 else 1.0,
                    "depth"))
    for i, n in enumerate(ns):                                    # every N at the headline shape
        out.append((f"S64-43+21-N{n}-p{(i + 1) % 2}-all-N", 43, 21, n, (i + 1) % 2, i % 2 == 0, 1.0, "depth"))
    return out


PLACE_CASES = _place_cases()
POSE_F, POSE_K = 2, 3                # the poses of the fused entry point: rays of fixed and of optimisable poses mixed


def place_id(c):
    return c[0]


@functools.lru_cache(maxsize=None)
def place_case(key):
    """-> dict: cfg, N, S, n_uniform, n_near, fp32 ``target_d`` [N,1] (or None), ``noise`` [N,S] (or None), ``tables`` (the three
    linspace tables the kernels take), and for the fused entry point: ``table`` [R,7] (d_cam, rgb, depth rows), ``rows`` [N] int64
    (some negative), ``owner`` [N] int64 (some negative), ``fixed`` [F,4,4], ``rot`` [K,4], ``trans`` [K,3], ``planted``."""
    name, nu, nn, N, perturb, use_bound, nf, target = key
    S = nu + nn
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    cfg = place_cfg(nu, nn, perturb=perturb, use_bound=use_bound, norm_factor=nf)
    planted = {}
    if target == "none":
        target_d = None
    else:
        di = torch.randint(4, 64, (N,), generator=gen)                             # d in [0.25, 4): multiples of 1/16
        # planted depths, as far as N has room (the lattice cases have N = 33: all of them)
        plan = [("ties_even", 16),          # d = 1: near list 0.75 .. 1.25: five ties with the 1/8 grid, among them z == d -+ T
                ("ties_odd", 17),           # d = 17/16: d - T and d + T are depth-guided samples, four other ties
                ("no_depth_zero", 0),       # d = 0: the near list is linspace(near, far): every entry ties; z = 0, 1/8 <= T
                ("no_depth_negative", -8),  # d = -0.5: the same list; back everywhere
                ("below_all", 1),           # d = 1/16: depth-guided samples below every uniform one (negative z)
                ("above_all", 72),          # d = 4.5: every depth-guided sample above every uniform one
                ("at_far", 64)]             # d = 4: ties at 3.75, 3.875, 4
        for r, (pname, v) in enumerate(plan):
            if r < N:
                di[r] = v
                planted[pname] = r
        target_d = (di.to(torch.float32) / 16.0)[:, None]
    noise = None
    if perturb:
        noise = torch.rand(N, S, generator=gen)
        noise[:, ::7] = 0.0                                                        # exactly 0 and exactly 1 - 2^-24 on chosen samples
        noise[:, 3::7] = ONE_BELOW
        noise[0, -1], noise[N - 1, 0] = ONE_BELOW, ONE_BELOW
    tr, cam = cfg["training"], cfg["cam"]
    if target_d is not None:
        tables = (torch.linspace(cam["near"], cam["far"], max(0, nu)), torch.linspace(-tr["range_d"], tr["range_d"], steps=nn),
                  torch.linspace(cam["near"], cam["far"], steps=nn))
    else:
        tables = (torch.linspace(cam["near"], cam["far"], S), None, None)
    # the ray table of the fused entry point: rows in another order than the rays, the rays' rows scattered among others
    R = 2 * N + 3
    perm = torch.randperm(R, generator=gen)[:N]
    table = torch.randn(R, 7, generator=gen)
    table[:, :3] = table[:, :3] * torch.tensor([0.6, 0.6, 0.2]) + torch.tensor([0.0, 0.0, 1.0])    # camera directions, z forward
    if target_d is not None:
        table[perm, 6] = target_d[:, 0]
    rows = perm.clone()
    rows[1::2] -= R                                                                # python-style negative rows
    owner = torch.randint(0, POSE_F + POSE_K, (N,), generator=gen)
    owner[: min(N, POSE_F + POSE_K)] = torch.arange(POSE_F + POSE_K)[: min(N, POSE_F + POSE_K)]
    owner[2::3] -= POSE_F + POSE_K
    rot = make_quaternions(POSE_K, gen, start=0)
    fixed = make_fixed(POSE_F, gen)
    trans = torch.randn(POSE_K, 3, generator=gen) * 0.5 + torch.tensor([1.0, 3.0, 1.0])
    # (translations inside the box of both normalisations; far = 4 along a ray leaves it: "points that leave the box")
    fixed[:, :3, 3] = torch.randn(POSE_F, 3, generator=gen) * 0.5 + torch.tensor([1.0, 3.0, 1.0])
    return dict(cfg=cfg, N=N, S=S, n_uniform=nu, n_near=nn, target_d=target_d, noise=noise, tables=tables, table=table, rows=rows,
                owner=owner, fixed=fixed, rot=rot, trans=trans, planted=planted, R=R)


def place_z(case):
    """the answer for z_vals: path_cpu.place_samples in fp32"""
    cfg = case["cfg"]
    return path_cpu.place_samples(case["N"], case["target_d"], cfg["training"], cfg["cam"], case["noise"])


def bound64(cfg):
    return torch.tensor(cfg["mapping"]["bound"], dtype=torch.float64), torch.tensor(cfg["mapping"]["localMLP_max_len"], dtype=torch.float64)


def normalised(pts32, cfg):
    """fp32(normalise_points(float64(pts32)) / norm_factor): the normalisation is float64 by construction in the reference and in
    the kernels (normalise1, csrc/common.h): same operations, same order, one cast"""
    b, h = bound64(cfg)
    return (path_cpu.normalise_points(pts32.double(), cfg["grid"], b, h) / cfg["training"]["norm_factor"]).to(torch.float32)


def place_xn(rays_o32, rays_d32, z32, cfg):
    """the answer for xn [N*S,3]: the fp32 sample points o + fp32(d * z) (two roundings: the unit is built without contraction),
    normalised in float64, cast once"""
    assert rays_o32.dtype == rays_d32.dtype == z32.dtype == torch.float32
    return normalised(path_cpu.ray_points(rays_o32, rays_d32, z32), cfg)


def masks(z, target_d, dtype):
    """front, back, band of the losses (path_cpu.sdf_losses' three lines) evaluated in ``dtype``"""
    z, d = z.to(dtype), target_d.to(dtype)
    T = torch.tensor(T_TOTAL, dtype=dtype)
    front = z < d - T
    back = z > d + T
    band = ~front & ~back & (d > 0.0)
    return front, back, band


def place_counts(z32, target_d):
    """[N,2] int32: #front, #band per ray by the mask rule on the fp32 z_vals"""
    front, _, band = masks(z32, target_d, torch.float32)
    return torch.stack([front.sum(1), band.sum(1)], 1).to(torch.int32)


# ================================================================================================== 2. pose path
QUAT_KINDS = ("unit", "half", "double", "identity", "half_turn", "off_sphere")


def make_quaternions(K, gen, start=0):
    """[K,4] fp32: pose k has kind QUAT_KINDS[(start + k) % 6]: unit, |q| = 0.5, |q| = 2, identity, w = 0 (a half turn), unit + 1e-3
    off the sphere (as Adam steps leave one)"""
    q = torch.randn(K, 4, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    for k in range(K):
        kind = QUAT_KINDS[(start + k) % 6]
        if kind == "half":
            q[k] *= 0.5
        elif kind == "double":
            q[k] *= 2.0
        elif kind == "identity":
            q[k] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
        elif kind == "half_turn":
            q[k, 0] = 0.0
            q[k] = q[k] / q[k].norm()
        elif kind == "off_sphere":
            q[k] *= 1.001
    q = q.to(torch.float32)
    for k in range(K):
        if QUAT_KINDS[(start + k) % 6] == "half_turn":
            q[k, 0] = 0.0
    return q


def make_fixed(F, gen):
    """[F,4,4] fp32 rigid transforms"""
    T = torch.eye(4).repeat(F, 1, 1)
    if F:
        q = torch.randn(F, 4, generator=gen, dtype=torch.float64)
        T[:, :3, :3] = quaternion_to_matrix(q / q.norm(dim=1, keepdim=True)).to(torch.float32)
        T[:, :3, 3] = torch.randn(F, 3, generator=gen)
    return T


LAYOUTS = ("runs", "skip", "four", "five", "scattered", "negative", "midwave")


def make_owner(layout, N, F, K):
    """[N] int64 owners (python-style negatives allowed, none out of range)"""
    P = F + K
    n = torch.arange(N)
    if layout == "runs":                    # long uniform runs, every pose in turn
        return n * P // N
    if layout == "skip":                    # runs that leave the LAST optimisable pose (and with K >= 3 the first too) without a ray
        use = [p for p in range(P) if p != P - 1 and not (K >= 3 and p == F)] or [0]
        return torch.tensor(use)[n * len(use) // N]
    if layout == "four":                    # exactly four distinct owners in every full wave (P >= 4): the last slot of PR_MAXSEG
        return ((n % 64) // 16 + 4 * (n // 64)) % P
    if layout == "five":                    # five in every full wave (P >= 5): the fifth goes through the atomic fall-back
        return ((n % 64) * 5 // 64 + 5 * (n // 64)) % P
    if layout == "scattered":               # min(P, 64) distinct owners in every full wave
        return n % P
    if layout == "negative":                # runs, every second ray with the python-style negative index of the same pose
        o = n * P // N
        return torch.where(n % 2 == 1, o - P, o)
    if layout == "midwave":                 # the pose boundary falls on lane 32 of every wave
        return ((n + 32) // 64) % P
    raise ValueError(layout)


POSE_NS = (1, 63, 64, 65, 255, 256, 257, 1000)
POSE_FK = ((0, 1), (1, 5), (2, 9), (0, 64), (63, 1))


def _pose_cases():
    """(N, F, K, layout, quaternion start): every (F, K) at every N with the layouts in rotation, and every layout at N = 257 and
    N = 1000 for every (F, K)"""
    out, seen = [], set()
    i = 0
    for fk in POSE_FK:
        for N in POSE_NS:
            out.append((N, *fk, LAYOUTS[i % len(LAYOUTS)], i % 6))
            i += 1
    for fk in POSE_FK:
        for N in (257, 1000):
            for lay in LAYOUTS:
                out.append((N, *fk, lay, i % 6))
                i += 1
    res = []
    for c in out:
        if c[:4] not in seen:
            seen.add(c[:4])
            res.append(c)
    return res


POSE_CASES = _pose_cases()


def pose_id(c):
    return f"N{c[0]}-F{c[1]}-K{c[2]}-{c[3]}-q{c[4]}"


@functools.lru_cache(maxsize=None)
def pose_case(key):
    N, F, K, layout, qstart = key
    gen = torch.Generator().manual_seed(1000 * N + 10 * (F + K) + qstart)
    d_cam = torch.randn(N, 3, generator=gen) * torch.tensor([0.6, 0.6, 0.2]) + torch.tensor([0.0, 0.0, 1.0])
    R = N + 5
    perm = torch.randperm(R, generator=gen)[:N]
    table = torch.randn(R, 7, generator=gen)
    table[perm, :3] = d_cam
    rows = perm.clone()
    rows[::3] -= R
    return dict(N=N, F=F, K=K, owner=make_owner(layout, N, F, K), d_cam=d_cam, table=table, rows=rows, fixed=make_fixed(F, gen),
                rot=make_quaternions(K, gen, qstart), trans=torch.randn(K, 3, generator=gen),
                g_o=torch.randn(N, 3, generator=gen), g_d=torch.randn(N, 3, generator=gen))


def pose_rays(rot, trans, fixed, owner, d_cam):
    """the chain of the reference in the dtype of its inputs: qt_to_transform_matrix -> gather by owner -> sum(d_cam * R, -1)"""
    T = qt_to_transform_matrix(rot, trans)
    poses = torch.cat([fixed.to(T), T]) if fixed is not None and fixed.shape[0] else T
    Pn = poses[owner]                                                              # (negative owners index from the end, as python)
    return Pn[:, :3, 3], torch.sum(d_cam[:, None, :] * Pn[:, :3, :3], -1)


def pose_reference(case, dtype, g_o=True, g_d=True):
    """-> rays_o, rays_d, d_rot, d_trans in ``dtype`` (float64: the answer; float32: the yardstick), the gradients of
    sum(g_o * rays_o) + sum(g_d * rays_d) by autograd (a part left out: that gradient is absent)"""
    rot = case["rot"].to(dtype).clone().requires_grad_(True)
    trans = case["trans"].to(dtype).clone().requires_grad_(True)
    ro, rd = pose_rays(rot, trans, case["fixed"].to(dtype), case["owner"], case["d_cam"].to(dtype))
    obj = torch.zeros((), dtype=dtype)
    if g_o:
        obj = obj + (case["g_o"].to(dtype) * ro).sum()
    if g_d:
        obj = obj + (case["g_d"].to(dtype) * rd).sum()
    gr, gt = torch.autograd.grad(obj, (rot, trans), allow_unused=True)
    gr = torch.zeros_like(rot) if gr is None else gr
    gt = torch.zeros_like(trans) if gt is None else gt
    return ro.detach(), rd.detach(), gr, gt


def emulate_pose_bwd(case, g_o=True, g_d=True):
    """pose_rays_bwd_kernel restated in numpy fp32 (products per ray, per-pose sums by pairwise addition, pose_chain operation by
    operation): what a correct fp32 kernel gives, in ANOTHER summation order than torch's: tests/test_step_cpu.py holds it to the
    working gate, so that the gate is one an fp32 kernel can meet."""
    f = np.float32
    N, F, K = case["N"], case["F"], case["K"]
    P = F + K
    owner = case["owner"].numpy() % P
    d = case["d_cam"].numpy().astype(f)
    gd = case["g_d"].numpy().astype(f) if g_d else np.zeros((N, 3), f)
    go = case["g_o"].numpy().astype(f) if g_o else np.zeros((N, 3), f)
    v = np.concatenate([(gd[:, :, None] * d[:, None, :]).reshape(N, 9), go], 1)
    G = np.zeros((P, 12), f)
    for p in range(P):
        rows = v[owner == p]
        while rows.shape[0] > 1:                                                   # pairwise: a tree, as wave_sum's
            if rows.shape[0] % 2:
                rows = np.concatenate([rows, np.zeros((1, 12), f)])
            rows = rows[0::2] + rows[1::2]
        if rows.shape[0]:
            G[p] = rows[0]
    q = case["rot"].numpy().astype(f)
    d_rot = np.zeros((K, 4), f)
    for k in range(K):
        w, x, y, z = q[k]
        g = G[F + k]
        n = w * w + x * x + y * y + z * z
        s = f(2.0) / n
        A = [-(y * y + z * z), x * y - z * w, x * z + y * w, x * y + z * w, -(x * x + z * z), y * z - x * w, x * z - y * w, y * z + x * w,
             -(x * x + y * y)]
        GA = f(0)
        for i in range(9):
            GA = GA + g[i] * A[i]
        two = f(2)
        dAw = (-z * g[1] + y * g[2]) + (z * g[3] - x * g[5]) + (-y * g[6] + x * g[7])
        dAx = (y * g[1] + z * g[2]) + (y * g[3] - two * x * g[4] - w * g[5]) + (z * g[6] + w * g[7] - two * x * g[8])
        dAy = (-two * y * g[0] + x * g[1] + w * g[2]) + (x * g[3] + z * g[5]) + (-w * g[6] + z * g[7] - two * y * g[8])
        dAz = (-two * z * g[0] - w * g[1] + x * g[2]) + (w * g[3] - two * z * g[4] + y * g[5]) + (x * g[6] + y * g[7])
        c = s * GA * two / n
        d_rot[k] = [s * dAw - c * w, s * dAx - c * x, s * dAy - c * y, s * dAz - c * z]
    return torch.from_numpy(d_rot), torch.from_numpy(G[F:, 9:].copy())


POSE_GROUPS_ROT = (("d quaternion", slice(0, 4)),)
POSE_GROUPS_TRANS = (("d translation", slice(0, 3)),)
RAY_GROUP = (("rays_d", slice(0, 3)),)

# ---- place_pose_bwd: d xn -> the pose gradients in one launch
PPB_NS, PPB_SS = (1, 15, 16, 17, 33), (1, 64, 65, 256)


def _ppb_cases():
    """(N, S, use_bound, norm_factor, F, K): every N x S x both normalisations; norm_factor 2 and the pose counts in rotation"""
    out, i = [], 0
    fks = ((2, 3), (0, 1), (1, 5), (0, 2))
    for N in PPB_NS:
        for S in PPB_SS:
            for ub in (True, False):
                out.append((N, S, ub, 2.0 if i % 3 == 0 else 1.0, *fks[i % 4]))
                i += 1
    return out


PPB_CASES = _ppb_cases()


def ppb_id(c):
    return f"N{c[0]}-S{c[1]}-{'bound' if c[2] else 'len'}-nf{c[3]:g}-F{c[4]}-K{c[5]}"


@functools.lru_cache(maxsize=None)
def ppb_case(key):
    N, S, use_bound, nf, F, K = key
    gen = torch.Generator().manual_seed(7 * N + 13 * S + int(use_bound) + int(nf) * 3)
    cfg = place_cfg(S, 0, perturb=0, use_bound=use_bound, norm_factor=nf)
    z = torch.sort(torch.rand(N, S, generator=gen) * 4.0, dim=1).values
    # the incoming gradient spans 2^-10 .. 2^10, as tests/test_gpu_render_fp64.py::test_rays_bwd's
    dxn = torch.exp2(20.0 * torch.rand(N * S, 3, generator=gen) - 10.0) * (2.0 * torch.randint(0, 2, (N * S, 3), generator=gen) - 1.0)
    owner = torch.randint(0, F + K, (N,), generator=gen)                           # fixed and optimisable poses mixed
    owner[1::4] -= F + K
    d_cam = torch.randn(N, 3, generator=gen) * torch.tensor([0.6, 0.6, 0.2]) + torch.tensor([0.0, 0.0, 1.0])
    return dict(N=N, S=S, F=F, K=K, cfg=cfg, z=z, dxn=dxn, owner=owner, d_cam=d_cam, fixed=make_fixed(F, gen),
                rot=make_quaternions(K, gen, N + S), trans=torch.randn(K, 3, generator=gen))


def ppb_reference(case, dtype):
    """d_rot, d_trans of sum(xn * dxn): the pose chain, ray_points and the float64 normalisation, poses and points in ``dtype``"""
    cfg = case["cfg"]
    rot = case["rot"].to(dtype).clone().requires_grad_(True)
    trans = case["trans"].to(dtype).clone().requires_grad_(True)
    ro, rd = pose_rays(rot, trans, case["fixed"].to(dtype), case["owner"], case["d_cam"].to(dtype))
    pts = path_cpu.ray_points(ro, rd, case["z"].to(dtype)).double()
    b, h = bound64(cfg)
    xn = path_cpu.normalise_points(pts, cfg["grid"], b, h) / cfg["training"]["norm_factor"]
    gr, gt = torch.autograd.grad((xn * case["dxn"].double()).sum(), (rot, trans), allow_unused=True)
    return (torch.zeros_like(rot) if gr is None else gr), (torch.zeros_like(trans) if gt is None else gt)


# ============================================================================= 3. frequency encoding, normalisation
FREQ_MS, FREQ_NFREQ = (1, 85, 86, 1000), (8, 5)          # M * 3 = 255 and 258 threads: either side of a 256-thread block


@functools.lru_cache(maxsize=None)
def freq_case(M, n_freq):
    """x [M,3] with 0, 0.5, 1, negative values and values above 1 in the first rows; dout [M, 6 n_freq] with octave k weighted 2^-k:
    every octave then weighs alike in dx (its factor is 2^k pi), where a flat dout leaves dx to the top octave alone"""
    gen = torch.Generator().manual_seed(31 * M + n_freq)
    x = torch.rand(M, 3, generator=gen) * 1.5 - 0.25
    special = torch.tensor([0.0, 0.5, 1.0, -0.375, 1.75, -0.0, 0.25, 1.0 - 2.0 ** -24, 2.0 ** -20])
    flat = x.reshape(-1)
    flat[: min(flat.numel(), special.numel())] = special[: flat.numel()]
    dout = torch.randn(M, 3, n_freq, 2, generator=gen) * torch.exp2(-torch.arange(n_freq, dtype=torch.float32))[None, None, :, None]
    return x, dout.reshape(M, 6 * n_freq).contiguous()


def freq_args(x32, n_freq):
    """[M,3,n_freq,2] fp32: the argument as tcnn forms it, fma(ldexp(x, k), pi_f, s * pi_f / 2) (oracle/tcnn_cpu.py's lines)"""
    t = torch.ldexp(x32[:, :, None], torch.arange(n_freq)[None, None, :])
    return torch.stack([tcnn_cpu._fma32(t, tcnn_cpu.PI_F32, s * tcnn_cpu.HALF_PI_F32) for s in range(2)], -1)


def freq_reference(x32, dout32, n_freq, dtype):
    """-> out [M, 6 n_freq], dx [M,3]: sine and cosine of the fp32 argument taken in ``dtype`` (float64: the answer, float32: torch's
    own sine and cosine, the yardstick), the sum of dx in ``dtype``"""
    arg = freq_args(x32, n_freq).to(dtype)
    out = torch.sin(arg).reshape(x32.shape[0], -1)
    fpi = (torch.exp2(torch.arange(n_freq, dtype=torch.float32)) * np.float32(tcnn_cpu.PI_F32)).to(dtype)     # exact in fp32: 2^k pi_f
    dx = (dout32.to(dtype).reshape(arg.shape) * (fpi[None, None, :, None] * torch.cos(arg))).sum((-1, -2))
    return out, dx


def normalise_bwd_answer(g32, cfg):
    """fp32((float64(g) / nf) / div)"""
    b, h = bound64(cfg)
    div = (b[:, 1] - b[:, 0]) if cfg["grid"]["use_bound_normalize"] else 2 * h
    return ((g32.double() / cfg["training"]["norm_factor"]) / div).to(torch.float32)


# =========================================================================================================== 4. Adam
def f32(x):
    """the fp32 value of a python scalar, as the C entry points receive it"""
    return float(np.float32(x))


def adam_scalars(lr, beta1, beta2, step):
    """float64 lr / bc1 and 1 / sqrt(bc2) of the fp32 scalars"""
    lr, b1, b2 = f32(lr), f32(beta1), f32(beta2)
    return lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)


def adam_answer(p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """path_cpu.adam_reference in float64 on the fp32 state and the fp32 scalars -> new p, m, v (float64)"""
    return path_cpu.adam_reference(p.double(), g.double(), m.double(), v.double(), step, f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd))


def adam_bound(p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """Per-element bounds (float64 tensors) on |kernel - adam_answer| for the new p, m, v of ONE step of adam1 (csrc/elementwise.hip):

        gg = g + wd * p;  m' = m + (gg - m) * omb1;  v' = v * b2 + (omb2 * gg) * gg;  p' = p - h0 * (m' / (sqrt(v') * h1 + eps))

    with omb1 = fp32(1 - b1), omb2 = fp32(1 - b2), h0 = fp32(lr / bc1), h1 = fp32(1 / sqrt(bc2)).  Every rounding is counted ONCE at
    u = 2^-24 against the float64 magnitude it acts on, errors are pushed through to first order, and every constant is then
    DOUBLED (second-order terms, a sqrt or a division that is an ulp off, a scalar whose tie flipped):

      gg : the product wd p and the sum: 2 roundings, each on at most |g| + |wd p|           E_g = 2 u (|g| + |wd p|)
      m' : gg - m, omb1's own rounding, the product, the sum: 4 roundings, each on at most |m| + |gg| (the last on |m'|, which is
           a mean of the two); E_g arrives scaled by (1 - b1)                               E_m = 4 u (|m| + |gg|) + (1 - b1) E_g
      v' : v b2, omb2's rounding, omb2 gg, (.) gg, the sum: 5 roundings on terms of a NON-NEGATIVE sum, so each is at most u v';
           E_g arrives through d (omb2 gg^2) = 2 omb2 |gg| E_g                              E_v = 5 u v' + 2 (1 - b2) |gg| E_g
      p' : D = sqrt(v') h1 + eps: sqrt, h1's rounding, the product, the sum: 4 roundings on terms of a non-negative sum, and E_v
           through the root: (E_v / v') / 2 on the share sqrt(v') h1 / D.  U = h0 m' / D: the division, h0's rounding, the product:
           3 more, and E_m / D scaled by h0.  The subtraction rounds once on p': ulp(p').
                                             E_p = u |p'| + |U| (7 u + (E_v / v') / 2 * sqrt(v') h1 / D) + h0 E_m / D

    bounds = 2 E + one denormal step.  With v' = 0 (v = 0 and gg = 0) E_v is 0 and the root's term is left out."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    b1, b2, eps, wd = f32(beta1), f32(beta2), f32(eps), f32(wd)
    h0, h1 = adam_scalars(lr, beta1, beta2, step)
    p1, m1, v1 = adam_answer(p, g, m, v, step, lr, beta1, beta2, eps, wd)
    gg = g + wd * p
    e_g = 2 * U * (g.abs() + (wd * p).abs())
    e_m = 4 * U * (m.abs() + gg.abs()) + (1 - b1) * e_g
    e_v = 5 * U * v1 + 2 * (1 - b2) * gg.abs() * e_g
    root = v1.sqrt() * h1
    D = root + eps
    upd = (h0 * m1 / D).abs()
    rel_v = torch.where(v1 > 0, e_v / v1.clamp_min(1e-300), torch.zeros_like(v1))
    e_p = U * p1.abs() + upd * (7 * U + 0.5 * rel_v * root / D) + h0 * e_m / D
    tiny = 2.0 ** -149
    return 2 * e_p + tiny, 2 * e_m + tiny, 2 * e_v + tiny


def adam1_f32(p, g, m, v, step, lr, beta1, beta2, eps, wd, mutation=None):
    """adam1 restated in numpy fp32, operation by operation (the scalars as make_adam forms them); mutation: "no_wd" (weight decay
    dropped) | "eps_in_sqrt" (eps moved inside the square root)"""
    f = np.float32
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    h0d, h1d = adam_scalars(lr, beta1, beta2, step)
    h0, h1, b2 = f(h0d), f(h1d), f(beta2)
    omb1, omb2 = f(1.0 - float(f(beta1))), f(1.0 - float(f(beta2)))
    eps, wd = f(eps), f(wd)
    gg = g
    if wd != 0 and mutation != "no_wd":
        gg = gg + wd * p
    m = m + (gg - m) * omb1
    v = v * b2 + (omb2 * gg) * gg
    if mutation == "eps_in_sqrt":
        denom = np.sqrt(v + eps) * h1
    else:
        denom = np.sqrt(v) * h1 + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        p = p - h0 * (m / denom)
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


ADAM_NS = (1, 3, 4, 5, 1023, 1024, 1025, 16384, 16385, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1)
ADAM_HYPER = ((0.01, 0.9, 0.99, 1e-15, 0.0), (0.001, 0.9, 0.999, 1e-8, 1e-6), (0.01, 0.9, 0.99, 1e-8, 0.0), (0.002, 0.8, 0.99, 1e-15, 1e-6))
ADAM_STEPS = (1, 2, 3, 10, 1000, 100000)


@functools.lru_cache(maxsize=None)
def adam_state(n, seed=0):
    """fp32 p, g, m, v [n]: gradients log-uniform in 1e-12 .. 1e-2 with either sign and exact zeros; moments as some earlier
    steps would have left them, over the same range; the first elements planted: v = 0 with g = 0 (m = 0 and m != 0: dense
    semantics still move p), g = 0 with v > 0, p = 0"""
    gen = torch.Generator().manual_seed(17 * n + seed)
    sign = lambda: 2.0 * torch.randint(0, 2, (n,), generator=gen) - 1.0      # noqa: E731
    logu = lambda lo, hi: torch.pow(10.0, lo + (hi - lo) * torch.rand(n, generator=gen))      # noqa: E731
    p = sign() * logu(-3, 0)
    g = sign() * logu(-12, -2)
    g[torch.rand(n, generator=gen) < 0.15] = 0.0
    m = sign() * logu(-12, -2)
    v = logu(-12, -2) ** 2
    plant = [dict(g=0.0, v=0.0, m=0.0), dict(g=0.0, v=0.0, m=1e-10), dict(g=0.0), dict(p=0.0), dict(g=1e-12), dict(g=-1e-2)]
    for i, d in enumerate(plant[:n]):
        for k, val in d.items():
            dict(p=p, g=g, m=m, v=v)[k][i] = val
    return p, g, m, v
