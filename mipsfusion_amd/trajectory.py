"""Absolute trajectory error the way it is published: the estimated positions aligned onto the true ones by Horn's closed form
(a rotation and a translation, no scale), then the statistics of the residual distances.  This is the reference's
``tools/eval_ate.py`` (``align``, ``evaluate_ate``, ``convert_poses``) without the timestamp association, the plots and the TUM
export.  A few dozen float64 numbers a call: host only, numpy, deliberately not a kernel.

``GraphedSequence``, ``tools/run_sequence.py`` and ``bench.py`` report an ``ate_rmse_m`` that is NOT aligned (the plain distance
between estimated and true positions); ``trajectory_metrics(..., align=False)`` gives that number.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np


class TrajectoryMetrics(NamedTuple):
    rmse: float
    mean: float
    median: float
    std: float
    min: float
    max: float
    pairs: int                       # frames compared: those whose true pose is finite
    R: np.ndarray                    # [3,3], t [3]: aligned = R @ est + t (the identity and 0 with align=False)
    t: np.ndarray
    residuals: np.ndarray            # [pairs] distances after the alignment, metres


def _host(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    elif isinstance(x, (list, tuple)) and len(x) and hasattr(x[0], "detach"):
        x = np.stack([p.detach().cpu().numpy() for p in x])
    return np.asarray(x, dtype=np.float64)


def _residuals(est: np.ndarray, gt: np.ndarray, R: np.ndarray, t: np.ndarray) -> np.ndarray:
    d = est @ R.T + t - gt
    return np.sqrt(np.sum(d * d, axis=1))


def align_trajectory(est_xyz, gt_xyz) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Horn's closed form -> (R [3,3], t [3], residuals [N]) with R @ est + t ~ gt: centred cross-covariance, SVD, the
    det(U) * det(Vh) < 0 reflection fix, t = mean(gt) - R @ mean(est).  est_xyz, gt_xyz [N,3]."""
    est, gt = _host(est_xyz), _host(gt_xyz)
    if est.ndim != 2 or est.shape[1] != 3 or est.shape != gt.shape:
        raise ValueError(f"align_trajectory: expected two of [N,3], got {est.shape} and {gt.shape}")
    if est.shape[0] < 1:
        raise ValueError("align_trajectory: no positions")
    me, mg = est.mean(0), gt.mean(0)
    Wm = (est - me).T @ (gt - mg)                        # sum over the frames of outer(est_c, gt_c)
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vh
    t = mg - R @ me
    return R, t, _residuals(est, gt, R, t)


def _positions(p, what: str) -> np.ndarray:
    p = _host(p)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        return p
    if p.ndim == 2 and p.shape[1] == 3:
        return p
    raise ValueError(f"{what}: expected [N,4,4] poses or [N,3] positions, got {p.shape}")


def trajectory_metrics(poses_est, poses_gt, scale: float = 1.0, align: bool = True) -> TrajectoryMetrics:
    """ATE of an estimated trajectory.  poses_est, poses_gt: [N,4,4] camera-to-world poses or [N,3] positions.  Frames whose TRUE
    pose holds a NaN or an inf are dropped (ScanNet has such); translations are divided by `scale`; rmse, mean, median, std, min and
    max are those of the residual distances after the alignment.  ``align=False`` compares the positions as they are.  Fewer than
    2 valid pairs raise ValueError."""
    est, gt = _positions(poses_est, "poses_est"), _positions(poses_gt, "poses_gt")
    if est.shape[0] != gt.shape[0]:
        raise ValueError(f"trajectory_metrics: {est.shape[0]} estimated and {gt.shape[0]} true poses")
    valid = np.isfinite(gt.reshape(gt.shape[0], -1)).all(axis=1)
    est_xyz = (est[:, :3, 3] if est.ndim == 3 else est)[valid] / float(scale)
    gt_xyz = (gt[:, :3, 3] if gt.ndim == 3 else gt)[valid] / float(scale)
    if est_xyz.shape[0] < 2:
        raise ValueError(f"trajectory_metrics: {est_xyz.shape[0]} valid pose pairs, at least 2 are needed")
    if align:
        R, t, res = align_trajectory(est_xyz, gt_xyz)
    else:
        R, t = np.eye(3), np.zeros(3)
        res = _residuals(est_xyz, gt_xyz, R, t)
    return TrajectoryMetrics(float(np.sqrt(np.dot(res, res) / len(res))), float(np.mean(res)), float(np.median(res)), float(np.std(res)),
                             float(np.min(res)), float(np.max(res)), int(len(res)), R, t, res)
