"""Float64 restatement of the TSDF tracker's model side (mipsfusion_amd/tsdf.py, csrc/tsdf_track.hip, include/mipsf_track.h) in
numpy, following the header's rules literally: every floating-point operation below is one IEEE float64 operation (numpy contracts
nothing), the ray cast evaluates EVERY sample of EVERY ray and knows nothing of bricks, and the registration tests every live pixel.
The device's depth, normal and colour words and its hit count must EQUAL what this file gives; the registration's pair sets and
counts too, its pose to the rounding of the sums' order and of sin and cos.  It is a checker, not the product.  It also holds the
cases the tests share, each computed once.
"""
import math

import numpy as np

from . import icp_cpu
from . import raster_cpu as R
from . import tsdf_cpu as T

MAX_SAMPLES = 0x100000                # MIPSF_TRACK_MAX_SAMPLES
BRICK = T.BRICK
# |depth - closed form| of the fused box room's ray cast, in voxels, over the hits (CPU and GPU test): twice the largest mean and
# the largest max measured with this restatement on box/40x56/v0.15/t4, views 0, 7 and 13 (tests/test_track_cpu.py prints them)
DEPTH_MEAN_GATE, DEPTH_MAX_GATE = 0.0786, 1.349   # 2 x 0.0393, 2 x 0.6743


# ------------------------------------------------------------------------------------------------------------ the field
def field(state, origin, voxel, p, min_weight=1.0):
    """p: list of three arrays -> (known bool, f float64), the header's trilinear field"""
    tsdf, weight = state["tsdf"], state["weight"]
    dims = tsdf.shape
    with np.errstate(all="ignore"):
        g = [(p[a] - origin[a]) / voxel for a in range(3)]
        fl = [np.floor(x) for x in g]
        valid = np.ones(np.shape(g[0]), bool)
        for a in range(3):
            valid &= (fl[a] >= 0.0) & (fl[a] <= float(dims[a]) - 2.0)
        i0 = [np.where(valid, fl[a], 0.0).astype(np.int64) for a in range(3)]
        i1 = [np.minimum(i0[a] + 1, dims[a] - 1) for a in range(3)]
        fr = [g[a] - fl[a] for a in range(3)]
        known = valid.copy()
        w = {}
        for c in range(8):
            idx = (i1[0] if c & 4 else i0[0], i1[1] if c & 2 else i0[1], i1[2] if c & 1 else i0[2])
            known &= weight[idx].astype(np.float64) >= min_weight
            w[c] = tsdf[idx].astype(np.float64)
        c00 = w[0] * (1.0 - fr[2]) + w[1] * fr[2]
        c01 = w[2] * (1.0 - fr[2]) + w[3] * fr[2]
        c10 = w[4] * (1.0 - fr[2]) + w[5] * fr[2]
        c11 = w[6] * (1.0 - fr[2]) + w[7] * fr[2]
        c0 = c00 * (1.0 - fr[1]) + c01 * fr[1]
        c1 = c10 * (1.0 - fr[1]) + c11 * fr[1]
        f = c0 * (1.0 - fr[0]) + c1 * fr[0]
    return known, np.where(known, f, 0.0)


def raycast(state, origin, voxel, poses, K, H, W, step, near=0.0, far=math.inf, min_weight=1.0, color=False, back_face=True):
    """-> dict(depth fp32 [n,H,W], normals fp32 [n,H,W,3], color fp32 [n,H,W,3] or None, hits int, samples int: field evaluations
    of the walk).  back_face=False leaves the back-face stop out (for the test that shows what it is for)."""
    fx, fy, cx, cy = R.intrinsics(K)
    P = R._poses(poses) if len(poses) else np.zeros((0, 4, 4))
    origin = np.asarray(origin, np.float64)
    voxel, step, near, far, min_weight = float(voxel), float(step), float(near), float(far), float(min_weight)
    dims = state["tsdf"].shape
    n = len(P)
    depth = np.zeros((n, H, W), np.float32)
    normals = np.zeros((n, H, W, 3), np.float32)
    colors = np.zeros((n, H, W, 3), np.float32) if color else None
    samples = 0
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    row, col = row.reshape(-1), col.reshape(-1)
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            Rm, t = pose[:3, :3], pose[:3, 3]
            dcx, dcy, dcz = (col - cx) / fx, -((row - cy) / fy), -1.0
            d = [(Rm[r, 0] * dcx + Rm[r, 1] * dcy) + Rm[r, 2] * dcz for r in range(3)]
            ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            miss = ~((ln > 0.0) & (ln < np.inf))
            dt = step / ln
            t_in, t_out = np.full(H * W, near), np.full(H * W, far)
            for a in range(3):
                lo, hi = origin[a], origin[a] + voxel * (float(dims[a]) - 1.0)
                ta, tb = (lo - t[a]) / d[a], (hi - t[a]) / d[a]
                mn, mx = np.where(tb < ta, tb, ta), np.where(tb > ta, tb, ta)
                moving = d[a] != 0.0
                t_in = np.where(moving & (mn > t_in), mn, t_in)
                t_out = np.where(moving & (mx < t_out), mx, t_out)
                miss |= ~moving & ((t[a] < lo) | (t[a] > hi))
            miss |= ~(t_out >= t_in)
            alive = ~miss
            prev_known, prev, prev_t = np.zeros(H * W, bool), np.zeros(H * W), np.zeros(H * W)
            hit, tstar = np.zeros(H * W, bool), np.zeros(H * W)
            i = 0
            while alive.any() and i < MAX_SAMPLES:
                ti = t_in + float(i) * dt
                alive &= ti <= t_out
                if not alive.any():
                    break
                samples += int(alive.sum())
                known, f = field(state, origin, voxel, [t[a] + d[a] * ti for a in range(3)], min_weight)
                both = alive & prev_known & known
                is_hit = both & (prev > 0.0) & (f <= 0.0)
                tstar = np.where(is_hit, prev_t + dt * (prev / (prev - f)), tstar)
                hit |= is_hit
                back = both & ~is_hit & (prev < 0.0) & (f > 0.0) if back_face else np.zeros(H * W, bool)
                alive &= ~is_hit & ~back
                prev_known, prev, prev_t = known, f, ti
                i += 1
            d32 = tstar.astype(np.float32)
            hit &= (d32 > 0) & (d32 < np.float32(np.inf))
            depth[k] = np.where(hit, d32, np.float32(0)).reshape(H, W)
            ps = [t[a] + d[a] * tstar for a in range(3)]
            grad, allk = [], hit.copy()
            for a in range(3):
                kp, fp = field(state, origin, voxel, [ps[b] + voxel if b == a else ps[b] for b in range(3)], min_weight)
                km, fm = field(state, origin, voxel, [ps[b] - voxel if b == a else ps[b] for b in range(3)], min_weight)
                allk &= kp & km
                grad.append(fp - fm)
            L = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2])
            ok = allk & (L > 0.0) & (L < np.inf)
            for a in range(3):
                normals[k, :, :, a] = np.where(ok, (grad[a] / L).astype(np.float32), np.float32(0)).reshape(H, W)
            if color:
                g = np.stack([(ps[a] - origin[a]) / voxel for a in range(3)], -1)
                c = T.sample_color(np.where(hit[:, None], g, 0.0), state["weight"], state["color"])
                colors[k] = np.where(hit[:, None], c, np.float32(0)).reshape(H, W, 3)
    return {"depth": depth, "normals": normals, "color": colors, "hits": int((depth != 0).sum()), "samples": samples}


def brick_marks(state, min_weight=1.0):
    """the header's marks -> bool [bricks_x, bricks_y, bricks_z]; only the test of the skipping's share looks at them"""
    cand = (state["weight"].astype(np.float64) >= float(min_weight)) & (state["tsdf"] <= 0)
    dims = cand.shape
    nb = [-(-s // b) for s, b in zip(dims, BRICK)]
    out = np.zeros(nb, bool)
    for bx in range(nb[0]):
        for by in range(nb[1]):
            for bz in range(nb[2]):
                lo = [max(b * s - 1, 0) for b, s in zip((bx, by, bz), BRICK)]
                hi = [min(b * s + s + 1, d) for b, s, d in zip((bx, by, bz), BRICK, dims)]
                out[bx, by, bz] = cand[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].any()
    return out


# ------------------------------------------------------------------------------------------------------------ registration
def _apply(M, x, y, z):
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def evaluate(Tm, model_depth, model_normals, pose_ref, live, K, depth_max, max_dist):
    """one evaluation of the header's rule -> dict(partner int64 [H*W], n, usable, sum_d2, A, b, ambiguous)"""
    fx, fy, cx, cy = R.intrinsics(K)
    H, W = live.shape
    Q = np.asarray(pose_ref, np.float32).astype(np.float64)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    row, col = row.reshape(-1), col.reshape(-1)
    with np.errstate(all="ignore"):
        d = np.asarray(live, np.float32).astype(np.float64).reshape(-1)
        usable = (d > 0) & (d < np.inf) & (d <= depth_max)
        p = _apply(Tm, d * ((col - cx) / fx), -(d * ((row - cy) / fy)), -d)
        q = [p[r] - Q[r, 3] for r in range(3)]
        cam = [(Q[0, c] * q[0] + Q[1, c] * q[1]) + Q[2, c] * q[2] for c in range(3)]
        z = -cam[2]
        u, v = cx + fx * (cam[0] / z), cy - fy * (cam[1] / z)
        col2, row2 = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = usable & (z > 0) & (col2 >= 0) & (col2 < W) & (row2 >= 0) & (row2 < H)
        ci, ri = np.where(inside, col2, 0).astype(np.int64), np.where(inside, row2, 0).astype(np.int64)
        dm = np.asarray(model_depth, np.float32).reshape(H, W)[ri, ci].astype(np.float64)
        nrm = np.asarray(model_normals, np.float32).reshape(H, W, 3)[ri, ci].astype(np.float64)
        n2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        cand = inside & (dm > 0) & (dm < np.inf) & (n2 > 0)
        c2, r2 = ci.astype(np.float64), ri.astype(np.float64)
        vm = _apply(Q, dm * ((c2 - cx) / fx), -(dm * ((r2 - cy) / fy)), -dm)
        e = [p[r] - vm[r] for r in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        md2 = max_dist * max_dist
        pair = cand & (d2 <= md2)
        res = (e[0] * nrm[:, 0] + e[1] * nrm[:, 1]) + e[2] * nrm[:, 2]
        # what a last-bit difference could flip
        near_int = lambda x: np.abs(x - np.round(x)) < 1e-9      # noqa: E731
        amb = usable & (np.abs(z) < 1e-12)
        amb |= usable & (z > 0) & (near_int(u + 0.5) | near_int(v + 0.5))
        amb |= inside & ((np.abs(dm) < 1e-12) & (dm != 0) | (n2 < 1e-12) & (n2 != 0))
        amb |= cand & (np.abs(d2 - md2) <= 1e-12 * md2)
    P3 = np.stack(p, 1)[pair]
    nn = nrm[pair]
    J = np.concatenate([np.cross(P3, nn), nn], 1)
    n = int(pair.sum())
    return {"partner": np.where(pair, ri * W + ci, -1), "n": n, "usable": int(usable.sum()), "sum_d2": float(d2[pair].sum()),
            "A": J.T @ J, "b": J.T @ res[pair], "ambiguous": int(amb.sum())}


def register(model_depth, model_normals, pose_ref, live, pose_init, K, depth_max=math.inf, max_dist=0.5, max_iteration=30,
             relative_fitness=1e-6, relative_rmse=1e-6):
    """the loop of mipsf_track_register -> dict(transformation, pose fp32, n, fitness, rmse, iterations, partner, pairs_per_eval,
    ambiguous_per_eval)"""
    Tm = np.asarray(pose_init, np.float32).astype(np.float64).copy()
    it, prev, pairs, ambiguous = 0, None, [], []
    while True:
        ev = evaluate(Tm, model_depth, model_normals, pose_ref, live, K, float(depth_max), float(max_dist))
        fitness = ev["n"] / ev["usable"] if ev["usable"] else 0.0
        rmse = math.sqrt(ev["sum_d2"] / ev["n"]) if ev["n"] else 0.0
        pairs.append(ev["n"]), ambiguous.append(ev["ambiguous"])
        stop = it >= max_iteration or (it > 0 and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse)
        if stop:
            break
        x = icp_cpu.solve_psd(ev["A"], -ev["b"]) if ev["n"] else None
        if x is not None:
            U = icp_cpu.rotation_zyx(x)
            Tm[:3] = U @ Tm[:3]
            Tm[:3, 3] += x[3:]
        prev = (fitness, rmse)
        it += 1
    return {"transformation": Tm, "pose": Tm.astype(np.float32), "n": ev["n"], "fitness": fitness, "rmse": rmse, "iterations": it,
            "partner": ev["partner"], "pairs_per_eval": pairs, "ambiguous_per_eval": ambiguous}


def odometry(depth, K, first_pose, origin, voxel, dims, trunc, min_correspondences=0, **kw):
    """tsdf_odometry on the host -> (poses fp32 [n,4,4], records, state); the poses go from stage to stage as fp32"""
    D = np.asarray(depth, np.float32)
    n, H, W = D.shape
    ticks = T.make_ticks(origin, voxel, dims)
    state = T.new_state(dims)
    poses = np.zeros((n, 4, 4), np.float32)
    poses[0] = np.asarray(first_pose, np.float32)
    T.integrate(state, ticks, D[:1], poses[:1], K, trunc)
    records = [None]
    for k in range(1, n):
        m = raycast(state, origin, voxel, poses[k - 1:k], K, H, W, 0.5 * trunc)
        r = register(m["depth"][0], m["normals"][0], poses[k - 1], D[k], poses[k - 1], K, max_dist=trunc, **kw)
        r["lost"] = r["n"] < min_correspondences
        poses[k] = poses[k - 1] if r["lost"] else r["pose"]
        if not r["lost"]:
            T.integrate(state, ticks, D[k:k + 1], poses[k:k + 1], K, trunc)
        records.append(r)
    return poses, records, state


def pose_error(a, b):
    """-> (degrees, metres) between two camera-to-world poses"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c)))), float(np.linalg.norm(a[:3, 3] - b[:3, 3]))


def perturbed(pose, deg, cm, seed):
    """`pose` turned by `deg` degrees about a seeded axis through the camera and moved `cm` centimetres along a seeded direction"""
    pose = np.asarray(pose, np.float64)
    M = icp_cpu.offset_transform(deg, cm, seed, centre=pose[:3, 3])
    return (M @ pose).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ cases
BOX_VIEWS = (0, 7, 13)                # of tsdf_cpu.box_poses20()
RAYCAST_CASES = ("box/40x56/v0.15/t4", "box/33x47/v0.20/t3", "box/40x56/v0.10/t4", "two_rooms/v0.20", "colour", "enter_through_a_face",
                 "unobserved", "behind_a_wall", "min_weight_2", "step_trunc/4", "step_trunc", "near_far", "side_1", "one_voxel", "side_2",
                 "image_1x1", "image_17x33", "no_views", "plane")
_cases = {}


def plane_volume():
    """20 x 20 x 70 voxels of 0.25, every weight 1, tsdf = (k - 4)/4 clipped to -1 .. 1: the surface is the lattice plane k = 4,
    and a sample on a lattice point of it is 0.0 exactly"""
    dims = (20, 20, 70)
    state = T.new_state(dims)
    state["weight"][:] = 1.0
    state["tsdf"][:] = np.clip((np.arange(70, dtype=np.float32) - 4.0) / 4.0, -1.0, 1.0)
    return state, np.array([-2.0, -3.0, 1.0]), 0.25, dims


def _crop(c, lo, hi):
    """the sub-volume lo .. hi (voxel indices, exclusive) of a fused case as a volume of its own"""
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    state = {"tsdf": np.ascontiguousarray(c["state"]["tsdf"][sl]), "weight": np.ascontiguousarray(c["state"]["weight"][sl]), "color": None}
    return state, c["origin"] + c["voxel"] * np.asarray(lo, np.float64)


def case(name):
    """name -> dict(state, origin, voxel, dims, poses fp32 tensor [n,4,4], K, H, W, step, near, far, min_weight, color, want: the
    restatement's answer); computed once"""
    if name in _cases:
        return _cases[name]
    import torch
    near, far, min_weight, color = 0.0, math.inf, 1.0, False
    box = "box/33x47/v0.20/t3"
    _, _, lo, hi = R.box_room()
    centre = 0.5 * (lo + hi)
    if name in T.BOX_CASES or name in ("min_weight_2", "step_trunc/4", "step_trunc", "near_far"):
        c = T.case(name if name in T.BOX_CASES else box)
        state, origin, poses = c["state"], c["origin"], c["poses"][list(BOX_VIEWS)]
        voxel, trunc, K, H, W = c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        step = {"step_trunc/4": 0.25 * trunc, "step_trunc": trunc}.get(name, 0.5 * trunc)
        if name == "min_weight_2":
            min_weight = 2.0
        if name == "near_far":                                   # the walls lie at 1.2 .. 4 m: both cut
            near, far = 1.9, 2.6
    elif name == "two_rooms/v0.20":
        c = T.case(name)
        state, origin, poses, voxel, trunc, K, H, W = c["state"], c["origin"], c["poses"], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        step = 0.5 * trunc
    elif name == "colour":
        c = T.case(name)
        state, origin, poses, voxel, trunc, K, H, W = c["state"], c["origin"], c["poses"][:3], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        step, color = 0.5 * trunc, True
    elif name in ("enter_through_a_face", "side_2"):             # the cameras of the room, outside the cropped volume
        c = T.case(box)
        X, Y, Z = c["dims"]
        state, origin = _crop(c, (0, 0, 0), (X, Y // 3, Z)) if name == "enter_through_a_face" else _crop(c, (3, 0, 0), (5, Y, Z))
        poses, voxel, trunc, K, H, W = c["poses"][[1, 3, 6, 7]], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        step = 0.5 * trunc
    elif name == "unobserved":                                   # tsdf_cpu's volume that no view updated, looked at from 1 m away
        c = T.case("outside")
        state, origin, voxel, trunc, K, H, W = c["state"], c["origin"], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        mid = origin + 0.5 * voxel * (np.asarray(c["dims"]) - 1)
        poses = torch.stack([R.pose_of(tuple(mid + [0.0, 0.0, 2.0]), 0.0, 0.0), R.pose_of(tuple(mid), 0.4, 0.2)])
        step = 0.5 * trunc
    elif name == "behind_a_wall":                                # between the wall z = hi[2] and the volume's face, looking into the room
        c = T.case(box)
        state, origin, voxel, trunc, K, H, W = c["state"], c["origin"], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        poses = torch.stack([R.pose_of((centre[0], centre[1], hi[2] + 0.45), 0.0, p) for p in (0.0, 0.2)]
                            + [R.pose_of((centre[0], centre[1], hi[2] + 1.5), 0.0, 0.0)])
        step = 0.5 * trunc
    elif name in ("side_1", "one_voxel"):
        c = T.case("1x5x70" if name == "side_1" else "one_voxel")
        state, origin, voxel, trunc, K, H, W = c["state"], c["origin"], c["voxel"], c["trunc"], c["K"], c["H"], c["W"]
        poses, step = c["poses"][:2], 0.5 * trunc
    elif name in ("image_1x1", "image_17x33", "no_views"):
        c = T.case(box)
        state, origin, voxel, trunc = c["state"], c["origin"], c["voxel"], c["trunc"]
        H, W, K = {"image_1x1": (1, 1, (30.0, 30.0, 0.0, 0.0)), "image_17x33": (17, 33, (25.0, 26.0, 16.3, 8.1)), "no_views": (5, 7, (5.0, 5.0, 3.0, 2.0))}[name]
        poses = c["poses"][:0] if name == "no_views" else c["poses"][[2, 8, 15]]
        step = 0.5 * trunc
    elif name == "plane":
        # looking along -z from above the volume's top face, the camera on a lattice line: the principal ray has d.x = d.y = 0 and
        # its samples fall on lattice points, the last of them on f == 0; the same from beside the volume (that ray misses);
        # an oblique view from inside
        state, origin, voxel, dims = plane_volume()
        trunc, step = 1.0, 0.25
        H, W, K = 9, 11, (12.0, 12.0, 5.0, 4.0)
        top = origin[2] + voxel * (dims[2] - 1)
        a, b, c3 = torch.eye(4), torch.eye(4), R.pose_of((0.1, -0.7, 9.3), 0.2, -0.15)
        a[:3, 3] = torch.tensor([origin[0] + 5 * voxel, origin[1] + 7 * voxel, top + 0.5])
        b[:3, 3] = torch.tensor([origin[0] - 1.0, origin[1] + 7 * voxel, top + 0.5])
        poses = torch.stack([a, b, c3])
    else:
        raise KeyError(name)
    want = raycast(state, origin, voxel, poses, K, H, W, step, near, far, min_weight, color)
    _cases[name] = {"state": state, "origin": np.asarray(origin, np.float64), "voxel": voxel, "dims": state["tsdf"].shape, "trunc": trunc,
                    "poses": poses, "K": K, "H": H, "W": W, "step": step, "near": near, "far": far, "min_weight": min_weight, "color": color,
                    "want": want}
    return _cases[name]


# the registration: the exact depth of a perturbed camera against the model cast from view 7 of the fused box room
REG_VOLUME, REG_VIEW = "box/40x56/v0.15/t4", 7
REG_OFFSETS = {"0.64deg_2.3cm": (0.64, 2.3, 1), "1.9deg_5.8cm": (1.9, 5.8, 2), "3.8deg_11.7cm": (3.8, 11.7, 3)}
REG_CASES = tuple(REG_OFFSETS) + ("bad_pixels", "depth_max", "max_dist", "no_model")
_reg = {}


def reg_model():
    if "model" not in _reg:
        c = T.case(REG_VOLUME)
        m = raycast(c["state"], c["origin"], c["voxel"], c["poses"][REG_VIEW:REG_VIEW + 1], c["K"], c["H"], c["W"], 0.5 * c["trunc"])
        _reg["model"] = (m["depth"][0], m["normals"][0], c["poses"][REG_VIEW].numpy())
    return _reg["model"]


def reg_case(name):
    """name -> dict(model_depth, model_normals, pose_ref, live fp32 [H,W], pose_init fp32, truth fp32, K, depth_max, max_dist, kw)"""
    if name in _reg:
        return _reg[name]
    c = T.case(REG_VOLUME)
    _, _, lo, hi = R.box_room()
    md, mn, ref = reg_model()
    deg, cm, seed = REG_OFFSETS.get(name, REG_OFFSETS["1.9deg_5.8cm"])
    truth = perturbed(ref, deg, cm, seed)
    live = R.box_exit_depth(lo, hi, truth, c["K"], c["H"], c["W"]).astype(np.float32)
    depth_max, max_dist = math.inf, c["trunc"]
    H, W = c["H"], c["W"]
    if name == "bad_pixels":                                     # tsdf_cpu's pattern: a quarter of the image 0, NaN, +inf, negative
        live[:H // 2, :W // 2][::2, ::2] = 0.0
        live[:H // 2, :W // 2][1::2, ::2] = np.nan
        live[:H // 2, :W // 2][::2, 1::2] = np.inf
        live[:H // 2, :W // 2][1::2, 1::2] = -1.5
    if name == "depth_max":                                      # half the frame lies beyond it
        depth_max = float(np.median(live))
    if name == "max_dist":
        max_dist = 0.045
    if name == "no_model":
        md, mn = np.zeros_like(md), np.zeros_like(mn)
    _reg[name] = {"model_depth": md, "model_normals": mn, "pose_ref": ref, "live": live, "pose_init": ref, "truth": truth, "K": c["K"],
                  "depth_max": depth_max, "max_dist": max_dist, "H": H, "W": W}
    return _reg[name]


def reg_want(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _reg:
        c = reg_case(name)
        _reg[key] = register(c["model_depth"], c["model_normals"], c["pose_ref"], c["live"], c["pose_init"], c["K"], c["depth_max"], c["max_dist"], **kw)
    return _reg[key]


# the odometry: an arc of 8 frames in the box room at 33 x 47 looking up into a corner (three planes in view: with one or two the
# registration slides along them), a degree and a centimetre and a half a frame, voxels of 10 cm
ODO_FRAMES = 8
_odo = {}


def odo_case():
    """-> dict(depth fp32 [8,H,W], truth fp32 [8,4,4], K, H, W, origin, voxel, dims, trunc, bounds [3,2])"""
    if not _odo:
        H, W, K = R.SIZES["33x47"]
        _, _, lo, hi = R.box_room()
        centre = 0.5 * (lo + hi)
        truth = np.stack([R.pose_of(tuple(centre + [0.21 + 0.015 * k, -0.4 + 0.004 * k, 0.33 - 0.009 * k]), 0.7 + 0.017 * k, 1.3 + 0.006 * k).numpy()
                          for k in range(ODO_FRAMES)]).astype(np.float32)
        depth = np.stack([R.box_exit_depth(lo, hi, p, K, H, W) for p in truth]).astype(np.float32)
        voxel = 0.1
        origin, dims = T.box_grid(voxel)
        bounds = np.stack([origin, origin + voxel * (np.asarray(dims) - 1.5)], 1)             # ceil((hi - lo)/voxel) + 1 = dims
        _odo.update(depth=depth, truth=truth, K=K, H=H, W=W, origin=np.asarray(origin, np.float64), voxel=voxel, dims=tuple(dims), trunc=4 * voxel,
                    bounds=bounds)
    return _odo
