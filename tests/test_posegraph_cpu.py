"""CPU tests of the sub-map pose graph: the numpy restatement (tests/posegraph_cpu.py) against central
differences and an independent optimiser, its sensitivity to the order of its sums, and the host helpers of
mipsfusion_amd/pose_graph.py against the reference's loops written out."""
import numpy as np
import pytest
import scipy.optimize as so
import torch

from mipsfusion_amd import pose_graph as pg

from . import posegraph_cpu as R

TH = R.SMALL_ANGLE


# ------------------------------------------------------------------------------------------------------------- Jacobian
def _edge_with_residual(theta, seed):
    """three nodes and one edge (1, 2) whose residual is exactly (tau, axis * theta) / weight 0.7"""
    rng = np.random.default_rng(seed)
    Xa, Xb = R.random_pose(rng, 0.7, 3.0), R.random_pose(rng, 1.1, 3.0)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    xi = np.concatenate([rng.uniform(-1, 1, 3), ax * theta])
    P = R.se3_exp(xi) @ R.rigid_inverse(R.rigid_inverse(Xa) @ Xb)
    return np.stack([np.eye(4), Xa, Xb]), np.array([[1, 2]]), P[None], np.array([0.7]), xi


@pytest.mark.parametrize("theta", [0.0, 1e-9, TH * (1 - 1e-9), TH * (1 + 1e-9), 1.0, 3.1])
def test_jacobian_agrees_with_central_differences(theta):
    """gate 1e-8: truncation of a central difference is about h^2 = 1e-12 times a third derivative, rounding about 1e-16 / h =
    1e-10; measured 1.8e-10 .. 4.1e-10 over these six angles"""
    X, edges, P, w, xi = _edge_with_residual(theta, 11)
    r, G = R.residuals(X, edges, P, w, jacobian=True)
    assert np.abs(r[0] / 0.7 - xi).max() < 1e-13
    J = R.dense_jacobian(G, edges, 3)
    assert not J[:, :6].any(), "columns of node 0"
    h, F = 1e-6, np.zeros_like(J)
    for node in (1, 2):
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Xp, Xm = X.copy(), X.copy()
            Xp[node], Xm[node] = R.se3_exp(d) @ X[node], R.se3_exp(-d) @ X[node]
            F[:, 6 * node + k] = (R.residuals(Xp, edges, P, w) - R.residuals(Xm, edges, P, w))[0] / (2 * h)
    err = np.abs(J - F).max()
    print(f"theta {theta:g}: |J - central differences| max {err:.2e}")
    assert err < 1e-8
    assert np.array_equal(J[:, 6:12], -J[:, 12:18])


def test_node_zero_has_no_columns():
    X, edges, P, w, _ = _edge_with_residual(0.4, 3)
    edges = np.array([[0, 2]])
    _, G = R.residuals(X, edges, P, w, jacobian=True)
    J = R.dense_jacobian(G, edges, 3)
    assert not J[:, :12].any() and J[:, 12:].any()
    A, b = R.assemble(*R.residuals(X, edges, P, w, jacobian=True), edges, 3)
    assert not A[:6].any() and not b[:6].any()


def test_small_angle_branch_meets_the_closed_forms():
    """just under and just over the threshold every result differs by less than 1e-12 (series error theta^8 = 4e-11 relative to
    coefficients that multiply theta^2-sized terms; closed-form cancellation 1e-16 / theta^2 = 4e-14)"""
    under, over = np.nextafter(TH, 0.0), TH
    tau = np.array([0.8, -0.5, 0.3])
    worst = 0.0
    for axis in (np.array([1.0, 0, 0]), np.array([0, 0, 1.0]), np.array([0.6, 0, 0.8])):
        a, b = np.concatenate([tau, axis * under]), np.concatenate([tau, axis * over])
        for f in (R.left_jacobian_inverse, R.se3_exp, lambda x: R.se3_log(R.se3_exp(x))):
            worst = max(worst, np.abs(f(a) - f(b)).max())
        # the same coefficient through both branches, at the size of the term it multiplies (a K, b K^2, c1 (PT + ..), c2 (PPT + ..),
        # c3 (PTPP + ..), ci K^2: the closed forms of c2 and c3 cancel to 1e-16 / theta^4 = 2e-11 on their own)
        both = zip(*[R._coefficients(np.float64(t)) for t in (under, over)])
        worst = max(worst, max(abs(float(u) - float(o)) * TH ** k for (u, o), k in zip(both, (1, 2, 1, 2, 3, 2))))
    print(f"largest difference across the small-angle threshold {worst:.2e}")
    assert worst < 1e-12
    rot = R.so3_exp(np.array([1e-4, 0, 0]))[0], R.so3_exp(np.array([R.SMALL_QUAT * 2 * (1 - 1e-9), 0, 0]))[0], \
        R.so3_exp(np.array([R.SMALL_QUAT * 2 * (1 + 1e-9), 0, 0]))[0]
    assert abs(R.so3_log(rot[0])[0] - 1e-4) < 1e-16 and abs(R.so3_log(rot[2])[0] - R.so3_log(rot[1])[0] - 4e-12) < 1e-15


def test_projection_follows_the_branch_rule_and_is_a_rotation():
    rng = np.random.default_rng(0)
    T = np.stack([R.random_pose(rng, a, 2.0) for a in (0.0, 0.3, 1.5, 2.0, 3.0, 3.14159)] + [np.diag([1.0, -1, -1, 1]), np.diag([-1.0, 1, -1, 1]),
                                                                                                np.diag([-1.0, -1, 1, 1])])
    Pm = R.project(T.astype(np.float32))
    assert np.abs(Pm - T).max() < 1e-6
    assert np.abs(Pm[:, :3, :3] @ np.swapaxes(Pm[:, :3, :3], 1, 2) - np.eye(3)).max() < 1e-15
    assert np.array_equal(R.project(np.eye(4)[None])[0], np.eye(4))


# ------------------------------------------------------------------------------------------------------------- optimiser
CHAINS = [(2, 0.05, 1.0), (3, 0.2, 0.1), (8, 0.5, 1.0), (12, 0.3, 0.1)]


@pytest.mark.parametrize("n,drift,weight", CHAINS)
def test_final_loss_is_that_of_an_independent_optimiser(n, drift, weight):
    X, e, o, w = R.chain_graph(n, drift=drift, seed=n, weight=weight)
    out = R.optimize(X, e, o, w, steps=50, patience=3, decreasing=1e-22)
    Xp, Pp, e64 = R.project(X), R.project(o), e.astype(np.int64)

    def f(d):
        Y = Xp.copy()
        Y[1:] = R.se3_exp(d.reshape(-1, 6)) @ Xp[1:]
        r = R.residuals(Y, e64, Pp, w).ravel()
        return np.concatenate([r, np.zeros(max(0, d.size - r.size))])       # MINPACK wants at least as many residuals as unknowns
    ls = so.least_squares(f, np.zeros(6 * (n - 1)), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    print(f"N {n}: first {out['first_loss']:.6e} final {out['loss']:.12e} scipy {2 * ls.cost:.12e} steps {out['steps']} rejections {out['rejections']}")
    assert out["loss"] <= 2 * ls.cost * (1 + 1e-6)
    ref = R.optimize(X, e, o, w)
    assert ref["loss"] <= ref["first_loss"] and 1 <= ref["steps"] <= 10


@pytest.mark.parametrize("n,drift,weight", CHAINS + [(20, 0.3, 1.0)])
def test_order_of_sums_moves_the_anchors_by_rounding_only(n, drift, weight):
    """LAPACK against a hand-rolled fixed-order Cholesky with the edges of every block added in reverse.  Gate 1e-11 * max(1, |t|):
    a hundredth of the GPU test's float64 gate, so that the order of sums (the one thing the kernel is free to choose) cannot use
    that gate up.  Measured: 0 .. 1.8e-15 at translations up to 9 m; the float32 outputs are equal."""
    X, e, o, w = R.chain_graph(n, drift=drift, seed=n, weight=weight, step=3.0)
    a = R.optimize(X, e, o, w)
    b = R.optimize(X, e, o, w, solve=R.solve_fixed, reverse_edges=True)
    scale = max(1.0, np.abs(a["anchors"][:, :3, 3]).max())
    dev = np.abs(a["anchors"] - b["anchors"]).max()
    print(f"N {n}: largest anchor deviation {dev:.2e} at |t| up to {scale:.1f}; float32 equal {np.array_equal(a['anchors32'], b['anchors32'])}")
    assert dev <= 1e-11 * scale
    assert (a["steps"], a["solves"], a["rejections"], a["status"]) == (b["steps"], b["solves"], b["rejections"], b["status"])


def test_zero_drift_is_a_fixed_point_with_nan_quality():
    X, e, o, w = R.exact_graph()
    out = R.optimize(X, e, o, w)
    assert out["first_loss"] == 0.0 and out["loss"] == 0.0 and out["steps"] == 3 and out["rejections"] == 0
    assert out["status"] == R.STATUS_NAN_QUALITY and np.array_equal(out["anchors"], R.project(X))
    assert out["radius"] == 1e4 * 0.5 * 0.25 * 0.125


def test_a_node_without_an_edge_stays_as_projected():
    X, e, o, w = R.chain_graph(5, loop=(3, 0), drift=0.3, seed=9, weight=1.0)
    keep = e.max(1) < 4
    out = R.optimize(X, e[keep], o[keep], w[keep])
    assert np.array_equal(out["anchors"][4], R.project(X)[4]) and not np.array_equal(out["anchors"][2], R.project(X)[2])


# ------------------------------------------------------------------------------------------------------------- rejections
def test_rejecting_fixture():
    """Lever arms of tens of metres with a loop disagreement beyond 2.5 rad make full steps overshoot: of 648 chains searched
    (N in {3, 4, 6, 10}, step in {1, 10, 40} m, drift in {2.6, 2.9, 3.1} rad, key weight in {1, 5, 50}, seeds 0..5) 214 rejected at
    least once, every one of them at a step of 10 m or more.  The fixtures kept reject 2..4 times, each `last < loss` decision with a
    relative margin above 1e-5."""
    for name, want in (("reject3", 3), ("reject6", 3), ("reject_w5", 4)):
        X, e, o, w = R.GPU_FIXTURES[name]()
        out = R.optimize(X, e, o, w)
        assert out["rejections"] == want and out["status"] == 0 and out["loss"] < out["first_loss"]
        assert R.decision_margin(out) > 1e-9


def test_a_decision_on_the_noise_floor_cannot_use_up_the_gpu_gate():
    """Near convergence `last < loss` compares two losses that differ by rounding; the kernel's rounding may take such a decision the
    other way.  With every decision whose relative margin is at most 1e-12 (1e4 roundings) flipped, the anchors of the GPU
    fixtures move by less than 1e-10 * max(1, |t|), a tenth of the GPU test's float64 gate, and the steps done stay."""
    worst = 0.0
    for name in sorted(R.GPU_FIXTURES):
        if name == "zero_drift":
            continue                                                        # exact: nothing rounds
        g = R.GPU_FIXTURES[name]()
        a, b = R.optimize(*g), R.optimize(*g, flip_below=1e-12)
        scale = np.maximum(1.0, np.abs(a["anchors"][:, :3, 3]).max(1))[:, None, None]
        worst = max(worst, float((np.abs(a["anchors"] - b["anchors"]) / scale).max()))
        assert a["steps"] == b["steps"] and a["status"] == b["status"]
    print(f"largest move of an anchor when noise-floor decisions flip: {worst:.2e}")
    assert worst < 1e-10


def test_failed_factorisation_sets_the_status_bit():
    X, e, o, w = R.chain_graph(3, drift=0.2, seed=2)
    out = R.optimize(X, e, o, w * np.array([1.0, 1.0, 1e200]))
    assert out["status"] & R.STATUS_FACTORISATION_FAILED and np.array_equal(out["anchors"], R.project(X))


# ------------------------------------------------------------------------------------------------------------- host helpers
def _reference_pairs(keyframe_submaps, n_submaps):
    """keyframeSet.add_adjcent_pair + find_adjacent_localMLP_pair, written out"""
    adj = torch.zeros(n_submaps, n_submaps)
    for a, b in keyframe_submaps:
        if a >= 0 and b >= 0:
            adj[a][b] = 1
            adj[b][a] = 1
    pairs, part = [], []
    for i in range(n_submaps):
        for j in range(n_submaps):
            if j <= i:
                continue
            if adj[i][j] > 0:
                pairs.append(torch.tensor([j, i], dtype=torch.int32))
                if i not in part:
                    part.append(i)
                if j not in part:
                    part.append(j)
    pairs = torch.sort(torch.stack(pairs, 0), -1)[0]
    return pairs, torch.sort(torch.tensor(part))[0]


def test_adjacent_pairs_and_gate_follow_the_reference():
    table = [[0, -1], [0, -1], [1, 0], [1, -1], [2, 1], [2, -1], [0, 2], [3, 2], [3, -1], [1, 3], [1, 0]]
    pairs, part = pg.adjacent_pairs(table)
    want_pairs, want_part = _reference_pairs(table, 5)
    assert pairs.dtype == torch.int32 and torch.equal(pairs, want_pairs) and torch.equal(part, want_part)
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert pg.global_ba_gate(part, 4) and not pg.global_ba_gate(part, 5)
    assert not pg.global_ba_gate(pg.adjacent_pairs([[0, -1], [1, -1]])[1], 2)
    one, p1 = pg.adjacent_pairs(torch.tensor([[0, -1], [1, 0]]))
    assert one.tolist() == [[0, 1]] and pg.global_ba_gate(p1, 2) and not pg.global_ba_gate(p1, 1)


def test_build_edges_follows_the_reference():
    rng = np.random.default_rng(5)
    X = torch.from_numpy(np.stack([R.random_pose(rng, 0.5, 3.0) for _ in range(4)]))
    prev, aft = torch.from_numpy(R.random_pose(rng, 0.2, 1.0)), torch.from_numpy(R.random_pose(rng, 0.3, 1.0))
    pairs = torch.tensor([[0, 1], [1, 2], [2, 3]], dtype=torch.int32)
    edges, poses = [], []                                                   # PoseCorrector.py:186-201
    for pair in pairs:
        edges.append(pair)
        poses.append(X[pair[1]].inverse() @ X[pair[0]])
    edges.append(torch.stack([torch.tensor(0, dtype=torch.int32), torch.tensor(3, dtype=torch.int32)], 0))
    poses.append(prev @ aft.inverse())
    got_e, got_p, got_w = pg.build_edges(X.float(), pairs, prev, aft, id_prev=3, id_aft=0, key_edge_weight=0.1)
    assert got_e.dtype == torch.int32 and torch.equal(got_e, torch.stack(edges))
    assert got_p.dtype == torch.float64 and float((got_p - torch.stack(poses)).abs().max()) < 1e-6
    got_e, got_p, got_w = pg.build_edges(X, pairs, prev, aft, id_prev=3, id_aft=0, key_edge_weight=0.1)
    assert float((got_p - torch.stack(poses)).abs().max()) < 1e-14 and got_w.tolist() == [1.0, 1.0, 1.0, 0.1]
    # every adjacency edge starts at a residual of zero
    r = R.residuals(R.project(X.numpy()), got_e.numpy().astype(np.int64), R.project(got_p.numpy()), got_w.numpy())
    assert np.abs(r[:3]).max() < 1e-14 and np.abs(r[3]).max() > 1e-3


def test_checks_refuse_what_the_kernel_refuses():
    X = torch.eye(4).repeat(3, 1, 1)
    eye = torch.eye(4)
    pairs = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError):
        pg.check_graph(65, torch.tensor([[0, 1]]))
    with pytest.raises(ValueError):
        pg.check_graph(3, torch.zeros(1025, 2, dtype=torch.int64) + torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        pg.check_graph(3, torch.tensor([[0, 1], [2, 2]]))
    with pytest.raises(ValueError):
        pg.check_graph(3, torch.tensor([[0, 3]]))
    with pytest.raises(ValueError):
        pg.check_graph(1, torch.tensor([[0, 1]]))
    pg.check_graph(3, pg.build_edges(X, pairs, eye, eye, 2, 0, 0.1)[0])
    bad = X.clone()
    bad[1, 0, 0] = -1.0                                                      # determinant -1
    with pytest.raises(ValueError):
        pg.check_rotations(bad, "anchors")
    bad = X.clone()
    bad[2, :3, :3] *= 1.001
    with pytest.raises(ValueError):
        pg.check_rotations(bad, "anchors")
    pg.check_rotations(X, "anchors")
    for f in (pg.pose_graph_optimize,):                                     # refused before any device is touched
        with pytest.raises(ValueError):
            f(X, torch.tensor([[0, 1], [1, 3]]), eye, eye, 2, 0)


def test_rebase_keeps_poses_relative_to_their_anchor():
    rng = np.random.default_rng(2)
    old = torch.from_numpy(np.stack([R.random_pose(rng, 0.5, 3.0) for _ in range(3)]))
    new = torch.from_numpy(np.stack([R.random_pose(rng, 0.5, 3.0) for _ in range(3)]))
    W = torch.from_numpy(np.stack([R.random_pose(rng, 0.9, 5.0) for _ in range(7)]))
    s = torch.tensor([0, 0, 1, 2, 2, 1, 0])
    out = pg.rebase(W.float(), s, old, new)
    assert out.dtype == torch.float64 and out.shape == (7, 4, 4)
    rel_old, rel_new = torch.linalg.inv(old[s]) @ W, torch.linalg.inv(new[s]) @ out
    assert float((rel_old - rel_new).abs().max()) < 1e-5
    assert float((pg.rebase(old, torch.arange(3), old, new) - new).abs().max()) < 1e-12
    assert float((pg.rebase(W, s, old, old) - W).abs().max()) < 1e-12
