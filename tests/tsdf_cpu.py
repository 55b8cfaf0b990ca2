"""Float64 restatement of the TSDF fusion (mipsfusion_amd/tsdf.py, csrc/tsdf.hip, include/mipsf_tsdf.h) in numpy, following the
header's rule literally: every floating-point operation below is one IEEE float64 operation (numpy contracts nothing), EVERY voxel
is tested against EVERY view in ascending view order (no bricks, no culling), and the running values are rounded to fp32 after
every view.  The device's tsdf, weight and colour words and its two counts must EQUAL what this file gives.  It is a checker, not
the product.  It also holds the cases the tests share, each computed once.
"""
import math

import numpy as np

from . import raster_cpu as R

VIEW_CHUNK = 256                      # MIPSF_TSDF_VIEW_CHUNK
BRICK = (8, 8, 16)                    # MIPSF_TSDF_BRICK_X, _Y, _Z
MEAN_GATE, MAX_GATE = 0.1, 1.0        # wall distance of the fused box room's vertices in voxels (CPU and GPU test): the measured
                                      # 0.041 .. 0.060 and 0.500 with room for a last-bit difference, not a target


def make_ticks(origin, voxel, dims):
    return [np.asarray(origin, np.float64)[a] + float(voxel) * np.arange(dims[a], dtype=np.float64) for a in range(3)]


def new_state(dims, color=False):
    dims = tuple(int(d) for d in dims)
    return {"tsdf": np.zeros(dims, np.float32), "weight": np.zeros(dims, np.float32), "color": np.zeros(dims + (3,), np.float32) if color else None}


def _project(ticks, pose, K, H, W):
    """the header's projection of every voxel into one view -> z, inside, row, col (arrays [X,Y,Z]; row and col 0 where not inside)"""
    fx, fy, cx, cy = R.intrinsics(K)
    p = [t.astype(np.float32).astype(np.float64).reshape([-1 if a == d else 1 for a in range(3)]) for d, t in enumerate(ticks)]
    Rm, t = pose[:3, :3], pose[:3, 3]
    q = [p[d] - t[d] for d in range(3)]
    cam = [(Rm[0, c] * q[0] + Rm[1, c] * q[1]) + Rm[2, c] * q[2] for c in range(3)]
    z = -cam[2]
    u = cx + fx * (cam[0] / z)
    v = cy - fy * (cam[1] / z)
    col, row = np.floor(u + 0.5), np.floor(v + 0.5)
    inside = (z > 0) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    return z, inside, np.where(inside, row, 0).astype(np.int64), np.where(inside, col, 0).astype(np.int64)


def integrate(state, ticks, depth, poses, K, trunc, depth_max=math.inf, max_weight=math.inf, rgb=None, return_pairs=False):
    """fuses the views into `state` in place -> (updates, observed) (, updated bool [n,X,Y,Z])"""
    D = np.asarray(depth, np.float32)
    D = D[None] if D.ndim == 2 else D
    P = R._poses(poses)
    C3 = None if rgb is None else np.asarray(rgb, np.float32).reshape(D.shape + (3,))
    assert (C3 is None) == (state["color"] is None) and len(P) == len(D)
    _, H, W = D.shape
    trunc, depth_max, max_weight = float(trunc), float(depth_max), float(max_weight)
    updates, pairs = 0, []
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            z, inside, ri, ci = _project(ticks, pose, K, H, W)
            d = D[k][ri, ci].astype(np.float64)
            usable = (d > 0) & (d < np.inf) & (d <= depth_max)
            sdf = d - z
            updated = inside & usable & (sdf >= -trunc)
            val = sdf / trunc
            val = np.where(val > 1.0, 1.0, val)
            w0 = state["weight"].astype(np.float64)
            w1 = w0 + 1.0
            new = ((state["tsdf"].astype(np.float64) * w0 + val) / w1).astype(np.float32)
            state["tsdf"] = np.where(updated, new, state["tsdf"])
            if C3 is not None:
                c = C3[k][ri, ci].astype(np.float64)
                newc = ((state["color"].astype(np.float64) * w0[..., None] + c) / w1[..., None]).astype(np.float32)
                state["color"] = np.where(updated[..., None], newc, state["color"])
            state["weight"] = np.where(updated, np.where(w1 < max_weight, w1, max_weight).astype(np.float32), state["weight"])
            updates += int(updated.sum())
            if return_pairs:
                pairs.append(updated)
    out = (updates, int((state["weight"] > 0).sum()))
    return out + (np.stack(pairs) if pairs else np.zeros((0,) + state["tsdf"].shape, bool),) if return_pairs else out


def marching_volume(state, min_weight=1.0):
    return np.where(state["weight"] >= np.float32(min_weight), state["tsdf"], np.float32(-np.inf)).astype(np.float32)


def extract_mesh(state, origin, voxel, min_weight=1.0):
    """-> (world vertices float64, faces int64, index-unit vertices float64)"""
    from . import mcubes_cpu
    v, f = mcubes_cpu.marching_cubes(marching_volume(state, min_weight), 0.0, 1.0)
    return np.asarray(origin, np.float64) + v * float(voxel), f, v


def sample_color(points, weight, color):
    """the header's rule of mipsf_tsdf_sample -> fp32 [m,3]"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    dims = weight.shape
    i0, i1, f = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            x, D = pts[:, a], dims[a]
            if D > 1:
                lo = np.minimum(np.maximum(np.floor(x), 0.0), float(D - 2))
                lo = np.where(np.isfinite(x), lo, 0.0)
                i0.append(lo.astype(np.int64)), i1.append(lo.astype(np.int64) + 1), f.append(np.minimum(np.maximum(x - lo, 0.0), 1.0))
            else:
                i0.append(np.zeros(len(x), np.int64)), i1.append(np.zeros(len(x), np.int64)), f.append(np.minimum(np.maximum(x, 0.0), 1.0))
        den, num = np.zeros(len(pts)), np.zeros((len(pts), 3))
        for corner in range(8):
            a, b, c = corner & 4, corner & 2, corner & 1
            share = ((f[0] if a else 1.0 - f[0]) * (f[1] if b else 1.0 - f[1])) * (f[2] if c else 1.0 - f[2])
            idx = ((i1[0] if a else i0[0]), (i1[1] if b else i0[1]), (i1[2] if c else i0[2]))
            m = np.where(weight[idx] > 0, share, 0.0)
            den = den + m
            num = num + m[:, None] * color[idx].astype(np.float64)
        out = np.where(den[:, None] > 0, num / den[:, None], 0.0).astype(np.float32)
    out[~np.isfinite(pts).all(1)] = 0
    return out


# ------------------------------------------------------------------------------------------------------------ the device's culling
def brick_keeps(ticks, poses, K, H, W, trunc, depth_max=math.inf):
    """csrc/tsdf.hip's view_can_update, restated: bool [n, bricks_x, bricks_y, bricks_z], whether the brick takes the view.  The
    culling is the one part of the kernel the header does not fix; tests/test_tsdf_cpu.py holds it to `never leaves out a pair the
    rule updates` without a GPU."""
    fx, fy, cx, cy = R.intrinsics(K)
    P = R._poses(poses)
    t32 = [t.astype(np.float32).astype(np.float64) for t in ticks]
    nb = [-(-len(t) // b) for t, b in zip(t32, BRICK)]
    lo = [np.array([t[i * b:(i + 1) * b].min() for i in range(n)]) for t, b, n in zip(t32, BRICK, nb)]
    hi = [np.array([t[i * b:(i + 1) * b].max() for i in range(n)]) for t, b, n in zip(t32, BRICK, nb)]
    shape = lambda a, d: a.reshape([-1 if x == d else 1 for x in range(3)])      # noqa: E731
    c = [shape(0.5 * lo[d] + 0.5 * hi[d], d) for d in range(3)]
    h = [np.maximum(shape(hi[d], d) - c[d], c[d] - shape(lo[d], d)) for d in range(3)]
    radius = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    out = np.zeros((len(P),) + tuple(nb), bool)
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            Rm, t = pose[:3, :3], pose[:3, 3]
            if not np.isfinite(pose[:3]).all():
                continue
            scale = 1.0 + sum(abs(t[d]) + np.abs(c[d]) for d in range(3))
            rr = radius * 1.000001 + 1.0e-9 * scale
            q = [c[d] - t[d] for d in range(3)]
            cc = [(Rm[0, a] * q[0] + Rm[1, a] * q[1]) + Rm[2, a] * q[2] for a in range(3)]
            rc = [rr * math.sqrt((Rm[0, a] * Rm[0, a] + Rm[1, a] * Rm[1, a]) + Rm[2, a] * Rm[2, a]) * 1.000001 for a in range(3)]
            zc = -cc[2]
            keep = (zc + rc[2] > 0) & (zc - rc[2] <= depth_max + trunc)
            a0, a1 = (-1.5 - cx) / fx, (W + 0.5 - cx) / fx
            keep &= ((cc[0] - a0 * zc) + (rc[0] + abs(a0) * rc[2]) >= 0) & ((cc[0] - a1 * zc) - (rc[0] + abs(a1) * rc[2]) <= 0)
            b0, b1 = (cy - H - 0.5) / fy, (cy + 1.5) / fy
            keep &= ((cc[1] - b0 * zc) + (rc[1] + abs(b0) * rc[2]) >= 0) & ((cc[1] - b1 * zc) - (rc[1] + abs(b1) * rc[2]) <= 0)
            out[k] = keep
    return out


def pairs_by_brick(updated):
    """updated bool [n,X,Y,Z] -> bool [n,bx,by,bz]: whether some voxel of the brick is updated by the view"""
    n, X, Y, Z = updated.shape
    nb = [-(-s // b) for s, b in zip((X, Y, Z), BRICK)]
    pad = np.zeros((n, nb[0] * BRICK[0], nb[1] * BRICK[1], nb[2] * BRICK[2]), bool)
    pad[:, :X, :Y, :Z] = updated
    return pad.reshape(n, nb[0], BRICK[0], nb[1], BRICK[1], nb[2], BRICK[2]).any((2, 4, 6))


# ------------------------------------------------------------------------------------------------------------ known answers
def wall_distance(vertices, lo, hi):
    """distance of every vertex to the nearest of the six wall planes of the box lo..hi"""
    v = np.asarray(vertices, np.float64)
    return np.minimum(np.abs(v - lo), np.abs(v - hi)).min(1)


# ------------------------------------------------------------------------------------------------------------ cases
BOX_OFFSETS = ((0.21, -0.4, 0.33), (-0.6, 1.2, -0.5))
BOX_CASES = {"box/40x56/v0.15/t4": ("40x56", 0.15, 4), "box/33x47/v0.20/t3": ("33x47", 0.20, 3), "box/40x56/v0.10/t4": ("40x56", 0.10, 4)}
TINY_SIZE = (8, 12, (8.0, 8.0, 5.5, 3.5))                     # H, W, K of the many-views case
EQUALITY_CASES = tuple(BOX_CASES) + ("two_rooms/v0.20", "one_voxel", "1x5x70", "outside", "bad_pixels", "max_weight_2", "many_views", "colour", "random_poses")
_cases = {}


def box_poses20():
    import torch
    return torch.cat([R.box_poses(offset=o) for o in BOX_OFFSETS])


def box_grid(voxel):
    _, _, lo, hi = R.box_room()
    origin = lo - 3 * voxel
    dims = [int(x) + 1 for x in np.ceil((hi - lo + 6 * voxel) / voxel)]
    return origin, dims


def box_depth(poses, K, H, W):
    _, _, lo, hi = R.box_room()
    return np.stack([R.box_exit_depth(lo, hi, p.numpy(), K, H, W) for p in poses]).astype(np.float32)


def case(name):
    """name -> dict(origin, voxel, dims, ticks, trunc, depth fp32 [n,H,W], rgb or None, poses fp32 tensor, K, H, W, depth_max,
    max_weight, state: the restatement's answer, updates, observed, updated bool [n,X,Y,Z]); computed once"""
    if name in _cases:
        return _cases[name]
    import torch
    from mipsfusion_amd import synth
    depth_max, max_weight, rgb = math.inf, math.inf, None
    _, _, lo, hi = R.box_room()
    centre = 0.5 * (lo + hi)
    if name in BOX_CASES or name in ("max_weight_2", "bad_pixels"):
        size, voxel, tv = BOX_CASES.get(name, ("33x47", 0.20, 3))
        H, W, K = R.SIZES[size]
        poses = box_poses20()
        depth = box_depth(poses, K, H, W)
        origin, dims = box_grid(voxel)
        trunc = tv * voxel
        if name == "max_weight_2":
            max_weight = 2.0
        if name == "bad_pixels":                                 # a quarter of every image each: 0, NaN, +inf, negative; beyond depth_max
            poses, depth = poses[:6], depth[:6].copy()
            depth[:, :H // 2, :W // 2][:, ::2, ::2] = 0.0
            depth[:, :H // 2, :W // 2][:, 1::2, ::2] = np.nan
            depth[:, :H // 2, :W // 2][:, ::2, 1::2] = np.inf
            depth[:, :H // 2, :W // 2][:, 1::2, 1::2] = -1.5
            depth[:, H // 2:, :W // 2][:, ::3] = -np.inf
            depth_max = 3.0
    elif name == "two_rooms/v0.20":
        H, W, K = R.SIZES["40x56"]
        poses = R.rooms_poses()
        T = synth.TWO_ROOMS
        depth = np.stack([synth.render_rooms_frame(T["room_a"], T["room_b"], T["door"], p, H, W, *K, seed=3)["depth"].numpy() for p in poses])
        voxel, trunc = 0.2, 0.8
        v, _ = synth.two_rooms_mesh()
        origin = v.min(0) - 3 * voxel
        dims = [int(x) + 1 for x in np.ceil((v.max(0) - v.min(0) + 6 * voxel) / voxel)]
    elif name in ("one_voxel", "1x5x70"):
        H, W, K = R.SIZES["33x47"]
        poses = box_poses20()
        depth = box_depth(poses, K, H, W)
        voxel, trunc = 0.05, 0.3
        dims = [1, 1, 1] if name == "one_voxel" else [1, 5, 70]
        origin = np.array([centre[0] + 0.4, centre[1] - 0.1, hi[2] - 69 * voxel + 0.4]) if name == "1x5x70" else np.array([lo[0] + 0.1, centre[1], centre[2]])
    elif name == "outside":                                      # both views look along -z; the volume lies 3 m behind them
        H, W, K = R.SIZES["33x47"]
        poses = R.box_poses(views=((0.0, 0.0), (0.3, -0.1), (-0.4, 0.2)))
        depth = box_depth(poses, K, H, W)
        voxel, trunc = 0.1, 0.3
        dims = [9, 10, 21]
        origin = centre + np.array([-0.4, -0.5, 3.0])
    elif name == "many_views":                                   # one more view than a workgroup's list holds
        H, W, K = TINY_SIZE
        reps = -(-(VIEW_CHUNK + 1) // 20)
        poses = torch.cat([R.box_poses(offset=tuple(np.asarray(o) + 0.02 * r * np.array([1.0, -0.5, 0.7]))) for r in range(reps) for o in BOX_OFFSETS])
        poses = poses[:VIEW_CHUNK + 1]
        depth = box_depth(poses, K, H, W)
        voxel, trunc = 0.25, 0.75
        origin, dims = box_grid(voxel)
    elif name == "random_poses":                                 # cameras inside, beside and far from the volume, noise for depth
        H, W, K = R.SIZES["33x47"]
        g = np.random.default_rng(11)
        voxel, trunc, dims = 0.1, 0.25, [19, 21, 35]
        origin = np.array([-0.9, -1.0, -1.7])
        where = np.concatenate([g.uniform(-1.0, 1.0, (12, 3)) * [0.9, 1.0, 1.7], g.uniform(-4.0, 4.0, (12, 3))])
        poses = torch.stack([R.pose_of(tuple(p), float(g.uniform(0, 2 * math.pi)), float(g.uniform(-1.5, 1.5))) for p in where])
        depth = g.uniform(0.2, 3.0, (len(poses), H, W)).astype(np.float32)
        depth[g.random(depth.shape) < 0.1] = 0.0
    elif name == "colour":
        H, W, K = R.SIZES["33x47"]
        poses = R.box_poses()
        bound = synth.config_reference_defaults()["mapping"]["bound"]
        frames = [synth.render_box_frame(bound, p, H, W, *K, drop=0) for p in poses]
        depth = np.stack([f["depth"].numpy() for f in frames])
        rgb = np.stack([f["rgb"].numpy() for f in frames])
        voxel, trunc = 0.2, 0.6
        origin, dims = box_grid(voxel)
    else:
        raise KeyError(name)
    ticks = make_ticks(origin, voxel, dims)
    state = new_state(dims, rgb is not None)
    updates, observed, updated = integrate(state, ticks, depth, poses, K, trunc, depth_max, max_weight, rgb, return_pairs=True)
    _cases[name] = {"origin": np.asarray(origin, np.float64), "voxel": voxel, "dims": tuple(dims), "ticks": ticks, "trunc": trunc, "depth": depth,
                    "rgb": rgb, "poses": poses, "K": K, "H": H, "W": W, "depth_max": depth_max, "max_weight": max_weight, "state": state,
                    "updates": updates, "observed": observed, "updated": updated}
    return _cases[name]
