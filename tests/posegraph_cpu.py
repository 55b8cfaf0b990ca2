"""numpy float64 restatement of the sub-map pose-graph optimisation (upstream: PoseCorrector.pose_graph_optimize,
model/poseGraph.py, run through pypose's LM + Cholesky + TrustRegion + StopOnPlateau).  Closed forms only: no pypose, no
autograd.  csrc/posegraph.hip is held to this file; its linear solve can be swapped (``solve=``) and the order in which the edges
of a block are summed reversed (``reverse_edges=True``) to measure how much the result depends on either.

Conventions: poses are camera-to-world 4x4; a tangent vector is xi = (tau, phi), translation first; Exp(xi) = [Exp(phi), V(phi) tau;
0, 1]; perturbations act on the left, X <- Exp(delta) X."""
import numpy as np

SMALL_ANGLE = 0.05            # below this angle (rad) every coefficient is its Taylor series to theta^6
SMALL_QUAT = 1e-3             # below this |vector part| the quaternion logarithm is its series
STATUS_FACTORISATION_FAILED, STATUS_NAN_QUALITY = 1, 2
MAX_DIAG = 1e32


# ------------------------------------------------------------------------------------------------------------ coefficients
def _coefficients(theta):
    """-> a = sin/t, b = (1-cos)/t^2, c1 = (t-sin)/t^3, c2 = (t^2+2cos-2)/(2t^4), c3 = (2t-3sin+t cos)/(2t^5),
    ci = (1 - (t/2) cot(t/2))/t^2, each with its series below SMALL_ANGLE"""
    theta = np.asarray(theta, np.float64)
    small = theta < SMALL_ANGLE
    t = np.where(small, 1.0, theta)
    t2 = t * t
    s, c = np.sin(t), np.cos(t)
    h = 0.5 * t
    big = (s / t, (1.0 - c) / t2, (t - s) / (t2 * t), (t2 + 2.0 * c - 2.0) / (2.0 * t2 * t2),
           (2.0 * t - 3.0 * s + t * c) / (2.0 * t2 * t2 * t), (1.0 - h * np.cos(h) / np.sin(h)) / t2)
    x = theta * theta
    ser = (1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040))),
           0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320))),
           1.0 / 6 + x * (-1.0 / 120 + x * (1.0 / 5040 + x * (-1.0 / 362880))),
           1.0 / 24 + x * (-1.0 / 720 + x * (1.0 / 40320 + x * (-1.0 / 3628800))),
           1.0 / 120 + x * (-1.0 / 2520 + x * (1.0 / 120960 + x * (-1.0 / 9979200))),
           1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x * (1.0 / 1209600))))
    return tuple(np.where(small, q, p) for p, q in zip(big, ser))


def hat(v):
    v = np.asarray(v, np.float64)
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -v[..., 2], v[..., 1]
    K[..., 1, 0], K[..., 1, 2] = v[..., 2], -v[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -v[..., 1], v[..., 0]
    return K


_I3 = np.eye(3)


# ------------------------------------------------------------------------------------------------------------ rotations
def mat_to_quat(R):
    """unit quaternion (x, y, z, w) of [...,3,3] by the branch rule of the reference's mat2SO3 (convert.py:93-135), normalised"""
    R = np.asarray(R, np.float64)
    m = np.swapaxes(R, -1, -2)
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    d2, d0d1, d0nd1 = m22 < 1e-5, m00 > m11, m00 < -m11
    t0, t1, t2, t3 = 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22, 1 + m00 + m11 + m22
    q0 = np.stack([m12 - m21, t0, m01 + m10, m20 + m02], -1)            # (w, x, y, z)
    q1 = np.stack([m20 - m02, m01 + m10, t1, m12 + m21], -1)
    q2 = np.stack([m01 - m10, m20 + m02, m12 + m21, t2], -1)
    q3 = np.stack([t3, m12 - m21, m20 - m02, m01 - m10], -1)
    c0, c1, c2 = d2 & d0d1, d2 & ~d0d1, ~d2 & d0nd1
    t = np.where(c0, t0, np.where(c1, t1, np.where(c2, t2, t3)))
    q = np.where(c0[..., None], q0, np.where(c1[..., None], q1, np.where(c2[..., None], q2, q3)))
    q = q / (2.0 * np.sqrt(t))[..., None]
    q = q / np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])[..., None]
    return q[..., [1, 2, 3, 0]]


def quat_to_mat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def project(T):
    """mat2SE3 followed by .matrix(): the rotation through its unit quaternion, the translation as it is -> float64 [...,4,4]"""
    T = np.asarray(T, np.float64)
    out = np.zeros(T.shape[:-2] + (4, 4))
    out[..., :3, :3] = quat_to_mat(mat_to_quat(T[..., :3, :3]))
    out[..., :3, 3] = T[..., :3, 3]
    out[..., 3, 3] = 1.0
    return out


def so3_log(R):
    q = mat_to_quat(R)
    q = np.where(q[..., 3:4] < 0, -q, q)
    v, w = q[..., :3], q[..., 3]
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    small = n < SMALL_QUAT
    u = (n / w) ** 2
    f_small = (2.0 / w) * (1.0 + u * (-1.0 / 3 + u * (1.0 / 5 + u * (-1.0 / 7))))
    f_big = 2.0 * np.arctan2(n, w) / np.where(small, 1.0, n)
    return v * np.where(small, f_small, f_big)[..., None]


def so3_exp(phi):
    phi = np.asarray(phi, np.float64)
    theta = np.sqrt((phi[..., 0] * phi[..., 0] + phi[..., 1] * phi[..., 1]) + phi[..., 2] * phi[..., 2])
    a, b, c1 = _coefficients(theta)[:3]
    K = hat(phi)
    K2 = K @ K
    return (_I3 + a[..., None, None] * K + b[..., None, None] * K2, _I3 + b[..., None, None] * K + c1[..., None, None] * K2)


# ------------------------------------------------------------------------------------------------------------ SE(3)
def se3_exp(xi):
    xi = np.asarray(xi, np.float64)
    R, V = so3_exp(xi[..., 3:])
    T = np.zeros(xi.shape[:-1] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = (V @ xi[..., :3, None])[..., 0]
    T[..., 3, 3] = 1.0
    return T


def se3_log(T):
    phi = so3_log(T[..., :3, :3])
    theta = np.sqrt((phi[..., 0] * phi[..., 0] + phi[..., 1] * phi[..., 1]) + phi[..., 2] * phi[..., 2])
    ci = _coefficients(theta)[5]
    K = hat(phi)
    Vinv = _I3 - 0.5 * K + ci[..., None, None] * (K @ K)
    return np.concatenate([(Vinv @ T[..., :3, 3, None])[..., 0], phi], -1)


def rigid_inverse(T):
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3, None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def adjoint(T):
    R, t = T[..., :3, :3], T[..., :3, 3]
    A = np.zeros(T.shape[:-2] + (6, 6))
    A[..., :3, :3] = R
    A[..., :3, 3:] = hat(t) @ R
    A[..., 3:, 3:] = R
    return A


def left_jacobian_inverse(xi):
    """Jl^-1(xi) of SE(3), translation first: [[Ji, -Ji Q Ji], [0, Ji]] with Ji = I - K/2 + ci K^2 and Barfoot's Q(tau, phi)"""
    xi = np.asarray(xi, np.float64)
    tau, phi = xi[..., :3], xi[..., 3:]
    theta = np.sqrt((phi[..., 0] * phi[..., 0] + phi[..., 1] * phi[..., 1]) + phi[..., 2] * phi[..., 2])
    _, _, c1, c2, c3, ci = (c[..., None, None] for c in _coefficients(theta))
    P, T = hat(phi), hat(tau)
    PT, TP, PP = P @ T, T @ P, P @ P
    PTP = PT @ P
    Q = 0.5 * T + c1 * (PT + TP + PTP) + c2 * (PP @ T + T @ PP - 3.0 * PTP) + c3 * (PTP @ P + P @ PTP)
    Ji = _I3 - 0.5 * P + ci * PP
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Ji
    J[..., 3:, 3:] = Ji
    J[..., :3, 3:] = -(Ji @ Q @ Ji)
    return J


# ------------------------------------------------------------------------------------------------------------ the graph
def residuals(X, edges, P, w, jacobian=False):
    """r [E,6] = w * Log(P X_a^-1 X_b); with jacobian=True also G [E,6,6] = d r / d delta_b (d r / d delta_a = -G)"""
    A = P @ rigid_inverse(X[edges[:, 0]])
    xi = se3_log(A @ X[edges[:, 1]])
    r = w[:, None] * xi
    if not jacobian:
        return r
    return r, w[:, None, None] * (left_jacobian_inverse(xi) @ adjoint(A))


def loss_of(r):
    return float(np.sum(np.sum(r * r, 1)))


def dense_jacobian(G, edges, n_nodes):
    """[6E, 6N] with the columns of node 0 zero (the tests' view of the Jacobian)"""
    J = np.zeros((6 * len(edges), 6 * n_nodes))
    for e, (a, b) in enumerate(edges):
        if b > 0:
            J[6 * e:6 * e + 6, 6 * b:6 * b + 6] += G[e]
        if a > 0:
            J[6 * e:6 * e + 6, 6 * a:6 * a + 6] -= G[e]
    return J


def assemble(r, G, edges, n_nodes, reverse_edges=False):
    """A = J^T J and b = -J^T r over nodes 1..N-1, block by block, the edges of a block added in ascending (or descending) index"""
    n = 6 * (n_nodes - 1)
    A, rhs = np.zeros((n, n)), np.zeros(n)
    order = range(len(edges) - 1, -1, -1) if reverse_edges else range(len(edges))
    for e in order:
        a, b = int(edges[e, 0]) - 1, int(edges[e, 1]) - 1
        M, g = G[e].T @ G[e], G[e].T @ r[e]
        if b >= 0:
            A[6 * b:6 * b + 6, 6 * b:6 * b + 6] += M
            rhs[6 * b:6 * b + 6] -= g
        if a >= 0:
            A[6 * a:6 * a + 6, 6 * a:6 * a + 6] += M
            rhs[6 * a:6 * a + 6] += g
        if a >= 0 and b >= 0:
            A[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= M
            A[6 * b:6 * b + 6, 6 * a:6 * a + 6] -= M
    return A, rhs


def solve_lapack(A, b):
    L = np.linalg.cholesky(A)
    y = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, y)


def solve_fixed(A, b):
    """hand-rolled Cholesky and triangular solves, every sum in a fixed ascending order (the kernel's order)"""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k]
        if not s > 0.0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            t = A[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k]
            L[i, j] = t / L[j, j]
    y = b.astype(np.float64).copy()
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def check_graph(n_nodes, edges):
    edges = np.asarray(edges)
    if n_nodes < 2 or n_nodes > 64 or not 1 <= len(edges) <= 1024:
        raise ValueError("graph size")
    if np.any(edges[:, 0] == edges[:, 1]) or edges.min() < 0 or edges.max() >= n_nodes:
        raise ValueError("bad edge")


def optimize(anchors, edges, observations, weights, steps=10, patience=3, decreasing=1e-3, radius=1e4, min_diag=1e-6, max_rejects=16,
             solve=solve_lapack, reverse_edges=False, flip_below=0.0):
    """DESIGN.md 4.15 -> dict: anchors float64 [N,4,4], anchors32, first_loss, loss, steps, solves, rejections, radius, status and
    trace = per step (last, loss, [(last, loss of every try)]).  flip_below: every `last < loss` decision whose relative margin is
    at most this is taken the OTHER way (what rounding may do to a decision on the noise floor; the tests bound its effect)."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(weights, np.float64).reshape(-1)
    X, P = project(anchors), project(observations)
    N = len(X)
    check_graph(N, edges)
    radius, down = np.float64(radius), 0.5
    damping = 1.0 / radius
    done = solves = rejections = plateau = status = 0
    trace = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        loss = first = loss_of(residuals(X, edges, P, w))
        for _ in range(int(steps)):
            last = loss
            r, G = residuals(X, edges, P, w, jacobian=True)
            A, rhs = assemble(r, G, edges, N, reverse_edges)
            d = np.clip(np.diagonal(A).copy(), min_diag, MAX_DIAG)
            rejects, tries = 0, []
            while True:
                d = d + d * damping
                A[np.diag_indices_from(A)] = d
                solves += 1
                try:
                    D = solve(A, rhs)
                    if not np.all(np.isfinite(D)):
                        raise np.linalg.LinAlgError("not finite")
                except np.linalg.LinAlgError:
                    status |= STATUS_FACTORISATION_FAILED
                    break
                saved = X.copy()
                X[1:] = se3_exp(D.reshape(-1, 6)) @ X[1:]
                loss = loss_of(residuals(X, edges, P, w))
                Dn = np.concatenate([np.zeros((1, 6)), D.reshape(-1, 6)])
                u = (G @ (Dn[edges[:, 1]] - Dn[edges[:, 0]])[..., None])[..., 0]
                den = -float(np.sum(np.sum(u * (2.0 * r + u), 1)))
                quality = np.float64(last - loss) / np.float64(den)
                tries.append((last, loss))
                if quality > 0.5:
                    radius, down = radius * 2.0, 0.5
                elif quality > 1e-3:
                    down = 0.5
                else:
                    if np.isnan(quality):
                        status |= STATUS_NAN_QUALITY
                    radius, down = radius * down, down * 0.5
                damping = 1.0 / radius
                reject = last < loss
                if flip_below and abs(loss - last) <= flip_below * abs(last):
                    reject = not reject
                if reject and rejects < max_rejects:
                    X, loss, rejects, rejections = saved, last, rejects + 1, rejections + 1
                    continue
                break
            done += 1
            trace.append((last, loss, tries))
            plateau = plateau + 1 if last - loss < decreasing else 0
            if plateau >= patience:
                break
    return {"anchors": X, "anchors32": X.astype(np.float32), "first_loss": first, "loss": loss, "steps": done, "solves": solves,
            "rejections": rejections, "radius": float(radius), "status": status, "trace": trace}


# ------------------------------------------------------------------------------------------------------------ fixtures
def random_pose(rng, angle, trans):
    """a pose whose rotation has exactly `angle` rad about a random axis and whose translation is uniform in +-trans"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    T = np.eye(4)
    T[:3, :3] = so3_exp(ax * angle)[0]
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def chain_graph(n, loop=(None, 0), drift=0.1, seed=0, step=1.0, weight=0.1, extra=0, as32=True):
    """A walk of n anchors (about `step` metres and 0.3 rad apart), the adjacency edges (i, i+1) of build_edges, and one key edge
    (loop[0], loop[1]) whose observation disagrees with the anchors by a rotation of `drift` rad and `drift` metres.  extra: that
    many further adjacency edges between random pairs (consistent with the anchors).  -> anchors, edges int32, observations, weights"""
    rng = np.random.default_rng(seed)
    X = [np.eye(4)]
    X[0][:3, 3] = rng.uniform(-1, 1, 3)
    for _ in range(n - 1):
        X.append(X[-1] @ random_pose(rng, 0.3, step))
    X = np.stack(X)
    if as32:
        X = X.astype(np.float32)
    Xp = project(X)
    pairs = [(i, i + 1) for i in range(n - 1)]
    while extra > 0:
        i, j = sorted(rng.choice(n, 2, replace=False))
        pairs.append((int(i), int(j)))
        extra -= 1
    a, b = (n - 1 if loop[0] is None else loop[0]), loop[1]
    edges = np.array(pairs + [(a, b)], np.int32)
    obs = [rigid_inverse(Xp[j]) @ Xp[i] for i, j in pairs]
    obs.append(random_pose(rng, drift, drift) @ rigid_inverse(Xp[b]) @ Xp[a])
    obs = np.stack(obs)
    if as32:
        obs = obs.astype(np.float32)
    return X, edges, obs, np.array([1.0] * len(pairs) + [weight])


def exact_graph():
    """zero drift in exact arithmetic: half-turn rotations and dyadic translations, so that every product is exact, every
    residual is exactly zero and the optimisation is a fixed point from its first step (quality 0/0)"""
    rots = [np.diag(d) for d in ([1.0, 1, 1], [1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1], [1.0, 1, 1])]
    X = np.zeros((5, 4, 4), np.float32)
    for i, Rm in enumerate(rots):
        X[i, :3, :3], X[i, :3, 3], X[i, 3, 3] = Rm, [0.5 * i, -1.25 * i, 2.0 + 0.25 * i], 1.0
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]
    Xd = X.astype(np.float64)
    obs = np.stack([rigid_inverse(Xd[j]) @ Xd[i] for i, j in pairs]).astype(np.float32)
    return X, np.array(pairs, np.int32), obs, np.array([1.0, 1.0, 1.0, 1.0, 0.1])


def _without_node(n, loop, **kw):
    """a chain whose last node has no edge"""
    X, e, o, w = chain_graph(n, loop=loop, **kw)
    keep = e.max(1) < n - 1
    return X, e[keep], o[keep], w[keep]


def _duplicates():
    """two conflicting key edges on one pair, and an adjacency edge given twice"""
    X, e, o, w = chain_graph(5, drift=0.3, seed=21, weight=1.0)
    X2, e2, o2, w2 = chain_graph(5, drift=0.5, seed=21, weight=0.5)
    assert np.array_equal(X, X2)
    return X, np.concatenate([e, e[1:2], e2[-1:]]), np.concatenate([o, o[1:2], o2[-1:]]), np.concatenate([w, w[1:2], w2[-1:]])


def _single_edge(**kw):
    """N = 2, E = 1: two anchors and nothing but the key edge (1, 0) with its drifted observation; the smallest accepted graph
    (one 6x6 block, one edge in every loop).  Its minimum is a loss of exactly zero."""
    X, e, o, w = chain_graph(2, **kw)
    assert e.tolist() == [[0, 1], [1, 0]]
    return X, e[1:], o[1:], w[1:]


def _as64(g):
    X, e, o, w = g
    return X.astype(np.float64), e, o.astype(np.float64), w


# the graphs of tests/test_gpu_posegraph.py (float32 inputs unless named *64)
GPU_FIXTURES = {
    "n2_e1": lambda: _single_edge(drift=0.3, seed=1, weight=1.0),
    "n2_e2": lambda: chain_graph(2, drift=0.3, seed=1, weight=1.0),         # the adjacency edge (0, 1) against the key edge (1, 0)
    "chain3": lambda: chain_graph(3, drift=0.2, seed=2),
    "chain8_loop0": lambda: chain_graph(8, drift=0.5, seed=3, weight=1.0),
    "chain8_inner_loop": lambda: chain_graph(8, loop=(6, 2), drift=0.4, seed=4, weight=2.0),
    "duplicates": _duplicates,
    "lonely_node": lambda: _without_node(6, (4, 0), drift=0.3, seed=9, weight=1.0),
    "zero_drift": exact_graph,
    "pi": lambda: chain_graph(4, drift=3.1, seed=8, weight=1.0),
    "lds20": lambda: chain_graph(20, drift=0.3, seed=5, weight=1.0),
    "ws21": lambda: chain_graph(21, drift=0.3, seed=6, weight=1.0),
    "n64_e1024": lambda: chain_graph(64, drift=0.3, seed=7, extra=1024 - 64, weight=1.0),
    "chain12_64": lambda: _as64(chain_graph(12, drift=0.3, seed=12, as32=False)),
    "reject3": lambda: chain_graph(3, drift=2.9, seed=1, step=40.0, weight=1.0),
    "reject6": lambda: chain_graph(6, drift=2.9, seed=1, step=40.0, weight=5.0),
    "reject_w5": lambda: chain_graph(3, drift=2.6, seed=2, step=10.0, weight=5.0),
}


def plateau_margin(out, decreasing=1e-3):
    """smallest relative distance of a step's decrease from the plateau threshold"""
    return min(abs((last - loss) - decreasing) / abs(decreasing) for last, loss, _ in out["trace"])


def decision_margin(out):
    """smallest relative margin of a `last < loss` decision"""
    m = [abs(loss - last) / max(abs(last), 1e-300) for _, _, tries in out["trace"] for last, loss in tries]
    return min(m) if m else float("inf")
