"""mipsfusion_amd.trajectory against what the reference's tools/eval_ate.py gave on the same trajectories (tests/golden/ate.npz,
written by tests/golden/make_ate_golden.py).

Gate: both sides call the same LAPACK on a 3 x 3 matrix; only the order of the covariance sum and of the residuals' arithmetic
differs.  The largest difference measured over all cases, in R, t, the residuals and the six statistics, was 2.23e-15 (absolute,
values of order 1 and below: a residual of the `scaled` case; the largest in R 5.6e-16, in t 1.6e-15, in a statistic 4.5e-16);
the gate is 100 times that: 2.3e-13.
"""
import math
import os

import numpy as np
import pytest

from mipsfusion_amd import trajectory as T

GATE = 2.3e-13
STATS = ("rmse", "mean", "median", "std", "min", "max")
CASES = ("two", "rigid50", "rigid300", "planar", "invalid", "scaled")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ate.npz"))


@pytest.mark.parametrize("name", CASES)
def test_aligned_ate_equals_the_reference(golden, name):
    g = {k.split(".", 1)[1]: golden[k] for k in golden.files if k.startswith(name + ".")}
    m = T.trajectory_metrics(g["est"], g["gt"], scale=float(g["scale"]))
    assert m.pairs == int(g["pairs"]) == len(m.residuals)
    diffs = {"residuals": float(np.abs(m.residuals - g["residuals"]).max()),
             "stats": max(abs(getattr(m, s) - float(v)) for s, v in zip(STATS, g["stats"]))}
    if name != "two":                    # two positions leave the rotation about their line free: the statistics decide there
        diffs["R"], diffs["t"] = float(np.abs(m.R - g["R"]).max()), float(np.abs(m.t - g["t"]).max())
    print(name, {k: f"{v:.2e}" for k, v in diffs.items()})
    assert max(diffs.values()) <= GATE, diffs
    assert abs(np.linalg.det(m.R) - 1.0) < 1e-12


def test_the_planar_case_takes_the_reflection_branch(golden):
    est, gt = golden["planar.est"][:, :3, 3], golden["planar.gt"][:, :3, 3]
    W = (est - est.mean(0)).T @ (gt - gt.mean(0))
    U, _, Vh = np.linalg.svd(W.T)
    assert np.linalg.det(U) * np.linalg.det(Vh) < 0
    R, t, res = T.align_trajectory(est, gt)
    assert np.linalg.det(R) > 0.999 and np.abs(U @ Vh - R).max() > 0.1          # without the fix it would be a reflection


def test_invalid_true_poses_are_dropped(golden):
    est, gt = golden["invalid.est"], golden["invalid.gt"]
    valid = np.isfinite(gt.reshape(len(gt), -1)).all(1)
    assert valid.sum() == 56
    m = T.trajectory_metrics(est, gt)
    ref = T.trajectory_metrics(est[valid], gt[valid])
    assert m.pairs == 56 and m.rmse == ref.rmse and np.array_equal(m.residuals, ref.residuals)
    assert np.isfinite(m.residuals).all()


def test_positions_and_poses_and_tensors_are_the_same(golden):
    import torch
    est, gt = golden["rigid50.est"], golden["rigid50.gt"]
    a = T.trajectory_metrics(est, gt)
    b = T.trajectory_metrics(est[:, :3, 3], gt[:, :3, 3])
    c = T.trajectory_metrics(torch.from_numpy(est), [torch.from_numpy(p) for p in gt])
    assert a.rmse == b.rmse == c.rmse and np.array_equal(a.R, b.R) and np.array_equal(a.R, c.R)


def test_unaligned_is_the_sequence_runner_s_number(golden):
    """align=False reproduces the ate_rmse_m expression of mipsfusion_amd/sequence.py (summarise), which works on fp32 poses"""
    import torch
    est = torch.from_numpy(golden["rigid300.est"]).float()
    gt = torch.from_numpy(golden["rigid300.gt"]).float()
    err = [float((est[k][:3, 3].cpu().float() - gt[k][:3, 3].float()).norm()) for k in range(len(est))]
    want = float(np.sqrt(np.mean(np.square(err))))
    m = T.trajectory_metrics(est, gt, align=False)
    assert abs(m.rmse - want) <= 1e-6 * want and round(m.rmse, 4) == round(want, 4)           # fp32 norms against float64 ones
    assert abs(m.max - max(err)) <= 1e-6 * max(err)
    assert np.array_equal(m.R, np.eye(3)) and not m.t.any()
    assert m.rmse > 10 * T.trajectory_metrics(est, gt).rmse                                    # the walk was moved rigidly


def test_too_few_pairs_and_bad_shapes_raise(golden):
    est, gt = golden["two.est"], golden["two.gt"].copy()
    assert T.trajectory_metrics(est, gt).pairs == 2
    gt[1, 0, 3] = math.nan
    with pytest.raises(ValueError, match="at least 2"):
        T.trajectory_metrics(est, gt)
    with pytest.raises(ValueError):
        T.trajectory_metrics(est[:1], golden["two.gt"])
    with pytest.raises(ValueError):
        T.trajectory_metrics(np.zeros((4, 2)), np.zeros((4, 2)))


def test_the_package_exports_the_trajectory_metrics():
    import mipsfusion_amd
    assert mipsfusion_amd.trajectory_metrics is T.trajectory_metrics and mipsfusion_amd.align_trajectory is T.align_trajectory
