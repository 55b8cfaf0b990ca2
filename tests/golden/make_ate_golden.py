"""Writes tests/golden/ate.npz: trajectories and what the reference's tools/eval_ate.py (align, evaluate_ate) makes of them.
    python tests/golden/make_ate_golden.py <root of the reference checkout>
Only arrays are kept.  Poses are float64 [N,4,4]; an invalid true pose is dropped and translations are divided by the scale
BEFORE the reference sees them, as its convert_poses does; evaluate_ate then runs with its own scale of 1.
"""
import os
import sys
import warnings

import numpy as np

STATS = ("rmse", "mean", "median", "std", "min", "max")


def rotation(g):
    q = g.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def poses(xyz, g):
    p = np.tile(np.eye(4), (len(xyz), 1, 1))
    for k in range(len(xyz)):
        p[k, :3, :3] = rotation(g)
    p[:, :3, 3] = xyz
    return p


def walk(g, n, planar=False):
    xyz = np.cumsum(g.normal(0, 0.05, (n, 3)), axis=0) + g.uniform(-2, 2, 3)
    if planar:
        xyz[:, 2] = 0.0
    return xyz


def moved(g, xyz, noise):
    """the estimate: the true positions under the inverse of a random rigid motion, plus noise"""
    R, t = rotation(g), g.uniform(-1, 1, 3)
    return (xyz - t) @ R + g.normal(0, noise, xyz.shape)


def cases():
    out = {}
    g = np.random.default_rng(2024)
    gt = walk(g, 2)
    out["two"] = (poses(moved(g, gt, 0.01), g), poses(gt, g), 1.0)
    for n in (50, 300):
        gt = walk(g, n)
        out[f"rigid{n}"] = (poses(moved(g, gt, 0.02), g), poses(gt, g), 1.0)
    # a planar trajectory: the cross-covariance has a singular value near zero whose sign the noise decides; take the first
    # seed at which the reflection branch fires
    for seed in range(100):
        h = np.random.default_rng(seed)
        gt = walk(h, 40, planar=True)
        est = moved(h, gt, 0.0)
        est = est + np.cross(est[1] - est[0], est[2] - est[0])[None] * h.normal(0, 1e-3, (40, 1))
        W = (est - est.mean(0)).T @ (gt - gt.mean(0))
        U, _, Vh = np.linalg.svd(W.T)
        if np.linalg.det(U) * np.linalg.det(Vh) < 0:
            out["planar"] = (poses(est, h), poses(gt, h), 1.0)
            break
    else:
        raise SystemExit("no seed fires the reflection branch")
    gt = poses(walk(g, 60), g)
    est = poses(moved(g, gt[:, :3, 3], 0.02), g)
    gt[7, 1, 3] = np.nan
    gt[8, 0, 0] = np.inf
    gt[31, 2, 3] = -np.inf
    gt[59] = np.nan
    out["invalid"] = (est, gt, 1.0)
    gt = walk(g, 80) * 2.5
    out["scaled"] = (poses(moved(g, gt, 0.05), g), poses(gt, g), 2.5)
    return out


def main(reference_root):
    sys.path.insert(0, os.path.join(reference_root, "tools"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        import eval_ate
        arrays = {}
        for name, (est, gt, scale) in cases().items():
            valid = np.isfinite(gt.reshape(len(gt), -1)).all(1)
            e, t = est[valid, :3, 3] / scale, gt[valid, :3, 3] / scale
            rot, trans, err = eval_ate.align(np.matrix(e.T), np.matrix(t.T))
            res = eval_ate.evaluate_ate({k: t[k] for k in range(len(t))}, {k: e[k] for k in range(len(e))})
            assert res["compared_pose_pairs"] == len(e)
            arrays.update({f"{name}.est": est, f"{name}.gt": gt, f"{name}.scale": np.float64(scale), f"{name}.R": np.asarray(rot),
                           f"{name}.t": np.asarray(trans).reshape(3), f"{name}.residuals": np.asarray(err),
                           f"{name}.stats": np.array([res[f"absolute_translational_error.{s}"] for s in STATS]),
                           f"{name}.pairs": np.int64(len(e))})
            print(name, len(e), "pairs, rmse", arrays[f"{name}.stats"][0])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ate.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1])
