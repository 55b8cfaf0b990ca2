"""Float64 restatement of the switch-pose rectification (mipsfusion_amd/pose_corrector.py, csrc/icp.hip) in numpy + scipy's
cKDTree, and the generators of the test cases.  It restates open3d's published estimate_normals() / registration_icp() from
reading (no open3d is installed and upstream pins no version): this file is the contract the kernels are held to.

Exactness: distances are ``((dx*dx + dy*dy) + dz*dz)`` of float64-widened coordinates, candidates are ordered by (distance,
index).  The tree's own distances are not trusted: a few candidates more than needed are queried, their distances recomputed
with the expression above, the list re-sorted, and the farthest candidate the tree returned must be strictly farther than the
last one kept (else more are queried), so nothing the tree left out can belong to the list.
"""
import math
import os

import numpy as np
import torch
from scipy.spatial import cKDTree

KNN = 30
WORKERS = min(16, os.cpu_count() or 1)      # threads of the tree queries
AMBIGUOUS_REL = 1e-9


def d2_exact(q, p):
    d = q - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_exact(target, queries, k, tree=None):
    """-> (idx [m,k] int64, d2 [m,k]) ordered by (d2, index); target, queries float64; k <= len(target)"""
    n, m = len(target), len(queries)
    assert 1 <= k <= n
    tree = tree if tree is not None else cKDTree(target)
    idx_out, d2_out = np.zeros((m, k), np.int64), np.zeros((m, k))
    todo, extra = np.arange(m), 8
    while len(todo):
        kk = min(n, k + extra)
        _, idx = tree.query(queries[todo], kk, workers=WORKERS)
        idx = idx.reshape(len(todo), kk)
        d2 = d2_exact(queries[todo][:, None, :], target[idx])
        order = np.lexsort((idx, d2), axis=1)
        idx, d2 = np.take_along_axis(idx, order, 1), np.take_along_axis(d2, order, 1)
        settled = np.ones(len(todo), bool) if kk == n else d2[:, -1] > d2[:, k - 1] * (1 + 1e-12)
        idx_out[todo[settled]], d2_out[todo[settled]] = idx[settled, :k], d2[settled, :k]
        todo, extra = todo[~settled], extra * 4
    return idx_out, d2_out


def cloud_cpu(rows, owner, poses):
    """torch-CPU evaluation of the upstream expression (PoseCorrector.py:70-87) -> (points fp32 [m,3], kept row indices)"""
    rows, poses = rows.cpu(), poses.cpu()
    owner = owner.cpu().long() if isinstance(owner, torch.Tensor) else torch.arange(rows.shape[0]) // int(owner)
    rays_d = torch.sum(rows[:, None, :3] * poses[owner, :3, :3], -1)
    pts = poses[owner, :3, 3] + rays_d * rows[:, 6:7]
    keep = rows[:, 6] > 0
    return pts[keep], torch.nonzero(keep).reshape(-1)


def nearest_cpu(source64, target32, max_dist, tree=None, second=False):
    """-> partner [m] int64 (-1: none within max_dist), d2 [m] (inf there); second=True also the runner-up's d2 (inf if none)"""
    m = len(source64)
    t = np.asarray(target32, np.float64)
    if len(t) == 0:
        out = (np.full(m, -1, np.int64), np.full(m, np.inf))
        return out + (np.full(m, np.inf),) if second else out
    k = min(2 if second else 1, len(t))
    idx, d2 = knn_exact(t, np.asarray(source64, np.float64), k, tree)
    pair = d2[:, 0] <= max_dist * max_dist
    out = (np.where(pair, idx[:, 0], -1), np.where(pair, d2[:, 0], np.inf))
    if second:
        out += (d2[:, 1] if k == 2 else np.full(m, np.inf),)
    return out


def normals_cpu(points32):
    """-> (normals [n,3], neighbours [n,min(30,n)], eigenvalues [n,3] ascending): covariance about the neighbourhood mean,
    the eigenvector of the smallest eigenvalue by numpy.linalg.eigh; (0,0,1) for n < 3"""
    p = np.asarray(points32, np.float64)
    n = len(p)
    out = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    if n == 0:
        return out, np.zeros((0, 0), np.int64), np.zeros((0, 3))
    k = min(KNN, n)
    idx, _ = knn_exact(p, p, k)
    if n < 3:
        return out, idx, np.zeros((n, 3))
    nb = p[idx]
    e = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", e, e) / k
    w, v = np.linalg.eigh(cov)
    return v[:, :, 0], idx, w


def rotation_zyx(x):
    sa, ca, sb, cb, sc, cc = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def solve_psd(A, b):
    """Cholesky solve; None when a pivot is not above 1e-12 of its diagonal entry (no full rank, whatever the rounding made of
    it) or the solution is not finite -- the registration then makes no update"""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (d > 0.0 and d > 1e-12 * A[j, j]):
            return None
        L[j, j] = math.sqrt(d)
        for r in range(j + 1, n):
            L[r, j] = (A[r, j] - (L[r, :j] * L[j, :j]).sum()) / L[j, j]
    x = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return x if np.all(np.isfinite(x)) else None


def icp_cpu(source32, target32, normals64, max_dist, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """The registration loop as the issue states it -> dict(transformation, n, fitness, rmse, iterations, partner,
    pairs_per_eval, ambiguous_per_eval, cond_max, stop_diffs)"""
    P = np.asarray(source32, np.float64).copy()
    t = np.asarray(target32, np.float64)
    tree = cKDTree(t) if len(t) else None
    m = len(P)

    def evaluate(first):
        j, d2, d2b = nearest_cpu(P, target32, max_dist, tree, second=True)
        pair = j >= 0
        amb = 0
        if not first:
            near_tie = pair & np.isfinite(d2b) & (d2b - np.where(pair, d2, 0.0) <= AMBIGUOUS_REL * d2b)
            d_all = np.sqrt(nearest_d2_any)
            at_edge = np.abs(d_all - max_dist) < 1e-9
            amb = int(np.count_nonzero(near_tie | at_edge))
        n = int(pair.sum())
        return {"j": j, "n": n, "fitness": n / m if m else 0.0, "rmse": math.sqrt(d2[pair].sum() / n) if n else 0.0, "amb": amb}

    # distance of every source point to its nearest target point whatever max_dist says (for the |d - max_dist| criterion)
    def refresh_any():
        if tree is None or m == 0:
            return np.full(m, np.inf)
        return knn_exact(t, P, 1, tree)[1][:, 0]
    T = np.eye(4)
    nearest_d2_any = refresh_any()
    res = evaluate(True)
    pairs, ambiguous, conds, diffs = [res["n"]], [0], [], []
    it = 0
    while it < max_iteration:
        U = np.eye(4)
        if res["n"]:
            sel = res["j"] >= 0
            p, q, nn = P[sel], t[res["j"][sel]], normals64[res["j"][sel]]
            r = ((p - q) * nn).sum(1)
            J = np.concatenate([np.cross(p, nn), nn], 1)
            A, b = J.T @ J, J.T @ r
            x = solve_psd(A, -b)
            if x is not None:
                U[:3, :3], U[:3, 3] = rotation_zyx(x), x[3:]
                conds.append(float(np.linalg.cond(A)))
        T = U @ T
        P = P @ U[:3, :3].T + U[:3, 3]
        it += 1
        prev = res
        nearest_d2_any = refresh_any()
        res = evaluate(False)
        pairs.append(res["n"]), ambiguous.append(res["amb"])
        diffs.append((abs(prev["fitness"] - res["fitness"]), abs(prev["rmse"] - res["rmse"])))
        if diffs[-1][0] < relative_fitness and diffs[-1][1] < relative_rmse:
            break
    return {"transformation": T, "n": res["n"], "fitness": res["fitness"], "rmse": res["rmse"], "iterations": it,
            "partner": res["j"], "pairs_per_eval": pairs, "ambiguous_per_eval": ambiguous, "cond_max": max(conds) if conds else 0.0,
            "stop_diffs": diffs}


def rectify_cpu(target32, source32, pose_this, settings):
    """switch_pose_rectifying on given clouds, composed as the device path composes it -> (flag, n, pose fp32 [4,4] numpy)"""
    normals = normals_cpu(target32)[0]
    r = icp_cpu(source32, target32, normals, settings["align_threshold"])
    pose_this = np.asarray(pose_this, np.float32)
    if r["n"] < settings["min_correspondence"]:
        return False, r["n"], pose_this, r
    rel = r["transformation"].astype(np.float32)
    if float(torch.linalg.norm(torch.from_numpy(rel[:3, 3]))) >= settings["min_trans_dist"]:
        rel = np.eye(4, dtype=np.float32)
    return True, r["n"], (torch.from_numpy(rel) @ torch.from_numpy(pose_this)).numpy(), r


# ------------------------------------------------------------------------------------------------------------ cases
ROOM = np.array([6.0, 4.0, 3.0])


def room_points(n, seed, x_max=None, noise=0.002):
    """n points on the faces of the room [0,6]x[0,4]x[0,3] (x <= x_max when given) with `noise` m of normal noise, fp32"""
    g = np.random.default_rng(seed)
    a, b, c = ROOM
    areas = np.array([b * c, b * c, a * c, a * c, a * b, a * b])
    pts = np.zeros((0, 3))
    while len(pts) < n:
        k = 2 * (n - len(pts)) + 16
        face = g.choice(6, k, p=areas / areas.sum())
        u = g.random((k, 3)) * ROOM
        axis, side = face // 2, face % 2
        u[np.arange(k), axis] = side * ROOM[axis]
        u += g.normal(0.0, noise, (k, 3))
        if x_max is not None:
            u = u[u[:, 0] <= x_max]
        pts = np.concatenate([pts, u])
    return pts[:n].astype(np.float32)


def offset_transform(deg, cm, seed, centre=ROOM / 2):
    """a rigid motion of `deg` degrees about a seeded axis through `centre` and `cm` centimetres along a seeded direction"""
    g = np.random.default_rng(seed)
    ax = g.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = math.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    tr = g.normal(size=3)
    tr *= cm / 100.0 / np.linalg.norm(tr)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, centre - R @ centre + tr
    return M


# name -> (target points, source points, offset degrees, offset cm); target covers x <= 5 of the 6 m room: fitness about 0.75
ROOM_CASES = {
    "room_300k": (300000, 30000, 1.0, 2.0),
    "room_100k": (100000, 30000, 3.0, 1.0),
    "room_30k": (30000, 30000, 0.5, 5.0),
    "room_1000": (30000, 1000, 2.0, 3.0),
    "room_31": (30000, 31, 1.0, 2.0),
    "room_29": (30000, 29, 1.0, 2.0),
    "room_2": (30000, 2, 1.0, 2.0),
    "room_1": (30000, 1, 1.0, 2.0),
}


def room_case(name):
    """-> (source fp32 [ns,3], target fp32 [nt,3], max_dist)"""
    nt, ns, deg, cm = ROOM_CASES[name]
    seed = sorted(ROOM_CASES).index(name)
    target = room_points(nt, 100 + seed, x_max=5.0)
    src = room_points(ns, 200 + seed).astype(np.float64)
    M = offset_transform(deg, cm, 300 + seed)
    return (src @ M[:3, :3].T + M[:3, 3]).astype(np.float32), target, 0.05


def wall_points(nx=60, ny=50, pitch=0.02, z=1.25):
    """a noise-free fronto-parallel wall sampled on a square lattice: ranks 30 and 31 share shells of equal distance"""
    x, y = np.meshgrid(np.arange(nx) * pitch, np.arange(ny) * pitch, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1).astype(np.float32)


def synth_scene(n_kf=4, rays_per_kf=(40, 60), drift_deg=1.0, drift_cm=2.0, seed=0):
    """Real ray rows of synth frames of the box room: `n_kf` keyframes around a view and one more frame between them.
    -> dict(cfg, kf_rows [n_kf, r, 7], kf_poses [n_kf,4,4], frame_rows [r,7], frame_pose_gt, frame_pose_drifted)"""
    from mipsfusion_amd import synth
    from mipsfusion_amd.helper_functions import sampling_helper as sh
    cfg = synth.config_reference_defaults()
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(cfg)
    kr, kc = sh.sample_pixels_uniformly(H, W, rays_per_kf[0], rays_per_kf[1])

    def rows_of(frame):
        full = torch.cat([frame["direction"], frame["rgb"], frame["depth"][..., None]], -1)
        return full[kr, kc].reshape(-1, 7).contiguous()
    poses = []
    for i in range(n_kf + 1):
        c2w = synth.default_pose(cfg, yaw=0.3 + 0.12 * (i - n_kf / 2), pitch=-0.6 + 0.03 * i)
        c2w[:3, 3] += torch.tensor([0.08 * i, 0.02 * i, -0.05 * i])
        poses.append(c2w)
    frames = [synth.make_frame(cfg, c2w=p, seed=seed + i, frame_id=i) for i, p in enumerate(poses)]
    mid = n_kf // 2
    kf_ids = [i for i in range(n_kf + 1) if i != mid]
    D = torch.from_numpy(offset_transform(drift_deg, drift_cm, 7 + seed, centre=poses[mid][:3, 3].double().numpy())).float()
    return {"cfg": cfg, "kf_rows": torch.stack([rows_of(frames[i]) for i in kf_ids]), "kf_poses": torch.stack([poses[i] for i in kf_ids]),
            "frame_rows": rows_of(frames[mid]), "frame_pose_gt": poses[mid], "frame_pose_drifted": D @ poses[mid]}


def synth_case(**kw):
    """-> (source fp32, target fp32, max_dist) of a synth scene, clouds by the torch-CPU expression"""
    s = synth_scene(**kw)
    r = s["kf_rows"].shape[1]
    target, _ = cloud_cpu(s["kf_rows"].reshape(-1, 7), r, s["kf_poses"])
    source, _ = cloud_cpu(s["frame_rows"], s["frame_rows"].shape[0], s["frame_pose_drifted"][None])
    return source.numpy(), target.numpy(), 0.05
