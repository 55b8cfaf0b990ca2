"""CPU checks of the float64 restatement of the switch-pose rectification (tests/icp_cpu.py): against brute force on small
clouds, and the caps the GPU tests (tests/test_gpu_icp.py) rely on, asserted on every case those tests use."""
import numpy as np
import pytest

from . import icp_cpu as R

ICP_CASES = sorted(R.ROOM_CASES) + ["synth"]


def _case(name):
    return R.synth_case() if name == "synth" else R.room_case(name)


def _brute_knn(t, q, k):
    d2 = R.d2_exact(q[:, None, :], t[None, :, :])
    idx = np.tile(np.arange(len(t)), (len(q), 1))
    order = np.lexsort((idx, d2), axis=1)[:, :k]
    return order, np.take_along_axis(d2, order, 1)


@pytest.mark.parametrize("seed", [0, 1])
def test_knn_equals_brute_force_with_ties(seed):
    g = np.random.default_rng(seed)
    t = np.round(g.random((400, 3)) * 8).astype(np.float32).astype(np.float64) / 8       # a coarse lattice: many exact ties
    q = np.concatenate([t[:50], g.random((50, 3))])
    for k in (1, 2, 30):
        idx, d2 = R.knn_exact(t, q, k)
        bi, bd = _brute_knn(t, q, k)
        assert np.array_equal(idx, bi) and np.array_equal(d2, bd)


def test_nearest_handles_duplicates_and_an_empty_target():
    g = np.random.default_rng(3)
    t = g.random((200, 3)).astype(np.float32)
    t2 = np.concatenate([t, t[:20]])
    j, d2 = R.nearest_cpu(t[:20].astype(np.float64), t2, 0.05)
    assert np.array_equal(j, np.arange(20)) and np.all(d2 == 0)
    j, d2 = R.nearest_cpu(t[:5].astype(np.float64), np.zeros((0, 3), np.float32), 0.05)
    assert np.all(j == -1) and np.all(np.isinf(d2))


def test_normals_of_a_plane_and_of_degenerate_clouds():
    w = R.wall_points()
    n, idx, ev = R.normals_cpu(w)
    assert np.all(np.abs(np.abs(n[:, 2]) - 1) < 1e-12) and idx.shape == (len(w), 30)
    bi, _ = _brute_knn(w[:200].astype(np.float64), w[:5].astype(np.float64), 30)
    sub, _ = R.knn_exact(w[:200].astype(np.float64), w[:5].astype(np.float64), 30)
    assert np.array_equal(bi, sub)
    for m in (1, 2):
        n, idx, _ = R.normals_cpu(w[:m])
        assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (m, 1))) and idx.shape == (m, m)


def test_icp_recovers_a_known_motion_on_a_small_room():
    tgt = R.room_points(20000, 1)
    M = R.offset_transform(1.5, 2.0, 2)
    src = (R.room_points(2000, 5, noise=0.0).astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    r = R.icp_cpu(src, tgt, R.normals_cpu(tgt)[0], 0.05)
    err = r["transformation"] @ M - np.eye(4)
    assert r["iterations"] < 30 and np.abs(err).max() < 2e-3, (r["iterations"], np.abs(err).max())
    far = R.icp_cpu(src + 100.0, tgt, R.normals_cpu(tgt)[0], 0.05)
    assert far["n"] == 0 and far["iterations"] == 1 and np.array_equal(far["transformation"], np.eye(4))


@pytest.mark.parametrize("name", ICP_CASES)
def test_caps_the_gpu_tests_rely_on(name):
    """Per case: ambiguous points (best two squared distances within 1e-9 relative, or |d - max_dist| < 1e-9, from the second
    evaluation on) <= 0.1 % of the source; cond(J^T J) <= 1e6; no stopping difference within 1 % of 1e-6; points whose normal
    is not gated ((l1 - l0)/l2 < 1e-3) <= 0.1 % of the target."""
    src, tgt, max_dist = _case(name)
    normals, _, ev = R.normals_cpu(tgt)
    r = R.icp_cpu(src, tgt, normals, max_dist)
    print(name, "iterations", r["iterations"], "pairs", r["pairs_per_eval"], "ambiguous", r["ambiguous_per_eval"],
          "cond %.3g" % r["cond_max"], "fitness %.4f rmse %.5f" % (r["fitness"], r["rmse"]))
    assert max(r["ambiguous_per_eval"]) <= 1e-3 * len(src)
    assert r["cond_max"] <= 1e6
    for df, dr in r["stop_diffs"]:
        assert not (0.99e-6 <= df <= 1.01e-6) and not (0.99e-6 <= dr <= 1.01e-6)
    gap = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    assert np.count_nonzero(gap < 1e-3) <= 1e-3 * len(tgt)
    assert r["iterations"] < 30
