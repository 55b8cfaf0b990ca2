"""Float64 restatement of the mesh evaluation (mipsfusion_amd/evaluate.py, csrc/eval.hip, include/mipsf_eval.h) in numpy, following
the header's rules literally: every floating-point operation below is one IEEE float64 operation (numpy contracts nothing), the
areas are integers, the random numbers an integer hash.  The device's samples and neighbours must EQUAL what this file gives.
It is a checker, not the product.
"""
import math

import numpy as np

from .icp_cpu import knn_exact

UNIT = 2.0 ** -40
CAP = 1 << 63
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------ sampler
def hash_words(seed, k, which):
    """the counter-based hash of include/mipsf_eval.h on uint32 (carried in uint64 and masked) -> uint64 array of 32-bit words"""
    k = np.asarray(k, np.uint64)
    h = (np.uint64((int(seed) & 0xFFFFFFFF) * 0x9E3779B9 & 0xFFFFFFFF) + k * np.uint64(3) + np.uint64(which)) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & M32
    h ^= h >> np.uint64(16)
    return h


def uniforms(seed, k, which):
    return (hash_words(seed, k, which) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def face_units(vertices32, faces):
    """-> python ints: floor(area * 2^40) per face, 0 for an index outside [0, V) or an area that is not finite"""
    v = np.asarray(vertices32, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = np.all((f >= 0) & (f < len(v)), axis=1)
    fs = np.where(ok[:, None], f, 0) if len(v) else np.zeros_like(f)
    if len(v) == 0:
        return [0] * len(f)
    A, B, C = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
    e1, e2 = B - A, C - A
    with np.errstate(all="ignore"):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        t = area * 2.0 ** 40
    out = []
    for okf, a, tf in zip(ok, area, t):
        if not okf or not (a < np.inf):
            out.append(0)
        else:
            out.append(CAP if tf >= 2.0 ** 63 else int(math.floor(tf)))
    return out


class SampleError(ValueError):
    pass


def sample_surface(vertices32, faces, n, seed=0):
    """-> (points fp32 [n,3], face_of int32 [n], area); SampleError for no faces, no area, or 2^63 units and more"""
    units = face_units(vertices32, faces)
    if len(units) == 0:
        raise SampleError("no faces")
    total = sum(units)
    if total >= CAP:
        raise SampleError("area overflow")
    if total == 0:
        raise SampleError("no area")
    cum = np.cumsum(np.array(units, np.uint64))
    assert int(cum[-1]) == total
    v = np.asarray(vertices32, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.arange(n, dtype=np.uint64)
    u0, u1, u2 = (uniforms(seed, k, w) for w in range(3))
    x = ((k.astype(np.float64) + u0) / np.float64(n)) * np.float64(total)
    pos = np.minimum(x.astype(np.uint64), np.uint64(total - 1))
    face_of = np.searchsorted(cum, pos, side="right")              # the first f with cum[f] > pos
    A, B, C = v[f[face_of, 0]], v[f[face_of, 1]], v[f[face_of, 2]]
    r = np.sqrt(u1)
    a, b, c = 1.0 - r, r * (1.0 - u2), r * u2
    p = (a[:, None] * A + b[:, None] * B) + c[:, None] * C
    return p.astype(np.float32), face_of.astype(np.int32), float(total) * UNIT


def mesh_area(vertices, faces):
    """the plain float64 area (no quantisation)"""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    return float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())


# ------------------------------------------------------------------------------------------------------------ nearest
def nearest(source32, target32):
    """-> (index int64 [m], d2 float64 [m]): exact, ties to the lower index; -1 and inf for an empty target"""
    s = np.asarray(source32, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(target32, np.float32).astype(np.float64).reshape(-1, 3)
    if len(t) == 0:
        return np.full(len(s), -1, np.int64), np.full(len(s), np.inf)
    if len(s) == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    idx, d2 = knn_exact(t, s, 1)
    return idx[:, 0], d2[:, 0]


def nearest_brute(source32, target32):
    """all pairs: the argmin of ((dx*dx + dy*dy) + dz*dz), the first among equals"""
    s = np.asarray(source32, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(target32, np.float32).astype(np.float64).reshape(-1, 3)
    d = s[:, None, :] - t[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    j = np.argmin(d2, axis=1)                                       # numpy: the first occurrence of the minimum
    return j.astype(np.int64), d2[np.arange(len(s)), j]


def grid_of(target32, min_edge=0.0, max_cells=1 << 21):
    """the grid mipsf_icp_bin lays over a cloud (icp.hip: bbox_finish_kernel) -> (origin [3], edge, dims [3])"""
    t = np.asarray(target32, np.float32).reshape(-1, 3)
    n = len(t)
    lo, hi = t.min(0).astype(np.float64), t.max(0).astype(np.float64)
    ext = hi - lo
    e = float(min_edge)
    if not e > 0.0:
        area = 2.0 * ((ext[0] * ext[1] + ext[1] * ext[2]) + ext[2] * ext[0])
        longest = float(ext.max())
        e = math.sqrt(8.0 * area / n)
        if not e > longest / 1024.0:
            e = longest / 1024.0
        if not (e > 0.0 and e < math.inf):
            e = 1.0
    for _ in range(4096):
        dims = np.floor(ext / e).astype(np.int64) + 1
        if float(np.prod(dims.astype(np.float64))) <= max_cells:
            return lo, e, dims
        e *= 1.25
    return lo, e, np.ones(3, np.int64)


def walk_cells(source32, target32, d2, min_edge=0.0, max_cells=1 << 21):
    """Cells the device's ring walk visits per source point (eval.hip: eval_nearest_kernel), from the stopping rule: after rings
    0..r the walk stops iff the true nearest distance is within the covered bound (everything unscanned is then farther, so the
    best so far IS the nearest; before that ring it cannot be) or the block is the whole grid.  -> (cells [m], rings [m])"""
    s = np.asarray(source32, np.float32).astype(np.float64).reshape(-1, 3)
    origin, e, dims = grid_of(target32, min_edge, max_cells)
    c = np.clip(np.floor((s - origin) / e), 0, dims - 1).astype(np.int64)
    slack = 16.0 * 2.220446049250313e-16 * float(np.max(np.abs(origin) + dims * e))
    cells, rings = np.zeros(len(s), np.int64), np.zeros(len(s), np.int64)
    todo = np.arange(len(s))
    for r in range(int(dims.max()) + 1):
        lo, hi = np.maximum(c[todo] - r, 0), np.minimum(c[todo] + r, dims - 1)
        low = np.where(lo > 0, np.maximum(s[todo] - (origin + lo * e), 0.0), np.inf)
        high = np.where(hi < dims - 1, np.maximum((origin + (hi + 1) * e) - s[todo], 0.0), np.inf)
        bound = np.minimum(low.min(1), high.min(1))
        covered = np.maximum(bound * (1.0 - 1.0e-6) - slack, 0.0)
        stop = ~(bound < np.inf) | (d2[todo] <= covered * covered)
        cells[todo[stop]], rings[todo[stop]] = np.prod(hi[stop] - lo[stop] + 1, axis=1), r
        todo = todo[~stop]
        if len(todo) == 0:
            break
    assert len(todo) == 0
    return cells, rings


# ------------------------------------------------------------------------------------------------------------ statistics
def stats(d2, threshold):
    """-> dict(sum_d, sum_d2, max_d, within, finite); entries that are not finite (or negative) are counted out"""
    d2 = np.asarray(d2, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (d2 >= 0.0) & (d2 < np.inf)
    v = d2[ok]
    return {"sum_d": math.fsum(np.sqrt(v)), "sum_d2": math.fsum(v), "max_d": math.sqrt(float(v.max())) if len(v) else 0.0,
            "within": int(np.count_nonzero(v <= threshold * threshold)), "finite": int(len(v))}


def reconstruction_metrics(mesh_rec, mesh_gt, n_samples, threshold=0.05, seed=0):
    """mesh = (vertices, faces); the fields of mipsfusion_amd.evaluate.ReconMetrics as a dict, plus the two d2 arrays"""
    p_rec, _, area_rec = sample_surface(np.asarray(mesh_rec[0], np.float32), mesh_rec[1], n_samples, seed)
    p_gt, _, area_gt = sample_surface(np.asarray(mesh_gt[0], np.float32), mesh_gt[1], n_samples, seed + 1)
    d2_acc, d2_comp = nearest(p_rec, p_gt)[1], nearest(p_gt, p_rec)[1]
    acc, comp = stats(d2_acc, threshold), stats(d2_comp, threshold)
    accuracy, completion = acc["sum_d"] / n_samples, comp["sum_d"] / n_samples
    return {"accuracy": accuracy, "completion": completion, "completion_ratio": comp["within"] / n_samples,
            "accuracy_ratio": acc["within"] / n_samples, "chamfer": 0.5 * (accuracy + completion), "accuracy_max": acc["max_d"],
            "completion_max": comp["max_d"], "area_rec": area_rec, "area_gt": area_gt, "within_acc": acc["within"],
            "within_comp": comp["within"], "d2_acc": d2_acc, "d2_comp": d2_comp}


# ------------------------------------------------------------------------------------------------------------ cases
def mesh_square(z=0.0):
    """the unit square in the plane z as 2 faces"""
    v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float64)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def mesh_random(seed=3, n_faces=5000):
    """5 000 small triangles, 50 of them with area 0 (a repeated vertex, or three points on a line), 3 with an index out of range
    (-1, V, 2^31 - 1), one 10^6 times larger in area than the rest -> (vertices fp32, faces int64)"""
    g = np.random.default_rng(seed)
    centres = g.uniform(-2.0, 2.0, (n_faces, 1, 3))
    v = (centres + g.uniform(-0.01, 0.01, (n_faces, 3, 3))).reshape(-1, 3)
    f = np.arange(3 * n_faces, dtype=np.int64).reshape(-1, 3)
    zero = g.choice(n_faces, 50, replace=False)
    f[zero[:25], 2] = f[zero[:25], 1]                                        # a repeated vertex
    v[f[zero[25:], 2]] = 0.5 * (v[f[zero[25:], 0]] + v[f[zero[25:], 1]])       # three points on a line (area 0 or a few units)
    rest = np.setdiff1d(np.arange(n_faces), zero)
    f[rest[0], 0], f[rest[1], 1], f[rest[2], 2] = -1, len(v), 2 ** 31 - 1
    big = rest[3]
    v[f[big]] = v[f[big, 0]] + (v[f[big]] - v[f[big, 0]]) * 1000.0           # edges x 1000: area x 10^6
    return v.astype(np.float32), f


SAMPLE_NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096)
SAMPLE_SEEDS = (0, 12345)
OFFSETS = ((3.0, 0.0, 0.0), (0.0, -10.0, 0.0), (2.0, 2.0, 2.0))
ROOMS = ("room_1000", "room_31", "room_2", "room_1")
FINE = {"min_edge": 1e-6, "max_cells": 1 << 20}

NEAREST_NAMES = tuple(ROOMS) + tuple(f"{r}+{o}" for r in ROOMS for o in OFFSETS) + ("on_box", "wall_ties", "target_1", "target_0",
                                                                                      "one_cell", "fine")

_cases = {}


def tie_wall():
    """a wall on a lattice of pitch 2^-5 (exact in fp32) and the same wall shifted by half a pitch along x and y: every source
    point has four target points at exactly the same distance"""
    from .icp_cpu import wall_points
    wall = wall_points(nx=40, ny=30, pitch=2.0 ** -5)
    return (wall + np.array([2.0 ** -6, 2.0 ** -6, 0.0], np.float32)).astype(np.float32), wall


def nearest_cases():
    """name -> (source fp32, target fp32, keyword arguments of nearest_distance, expected index, expected d2), built once"""
    if _cases:
        return _cases
    from .icp_cpu import room_case
    raw = {}
    for name in ROOMS:
        src, tgt, _ = room_case(name)
        raw[name] = (src, tgt, {})
        for off in OFFSETS:
            raw[f"{name}+{off}"] = ((src + np.array(off, np.float32)).astype(np.float32), tgt, {})
    src, tgt, _ = raw["room_1000"]
    lo, hi = tgt.min(0), tgt.max(0)
    g = np.random.default_rng(5)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    on_faces = (lo + g.random((56, 3)).astype(np.float32) * (hi - lo)).astype(np.float32)
    axis, side = np.arange(56) % 3, (np.arange(56) // 3) % 2
    on_faces[np.arange(56), axis] = np.where(side == 1, hi[axis], lo[axis])
    raw["on_box"] = (np.concatenate([corners, on_faces]), tgt, {})
    raw["wall_ties"] = tie_wall() + ({},)
    raw["target_1"] = (src, tgt[:1].copy(), {})
    raw["target_0"] = (src[:100].copy(), tgt[:0].copy(), {})
    raw["one_cell"] = (src, tgt, {"max_cells": 1})
    raw["fine"] = (src, tgt, dict(FINE))
    assert sorted(raw) == sorted(NEAREST_NAMES)
    for name, (s, t, kw) in raw.items():
        _cases[name] = (s, t, kw) + nearest(s, t)
    return _cases


E2E_SAMPLES = 4096
SHIFT_THRESHOLD = 0.3       # the smallest round threshold at which the shifted pair's ratios are exactly 1 at 4096 samples


def shifted_box_pair():
    """(reconstruction, ground truth): the box room of the reference configuration shifted by 2 cm along x, and itself"""
    from mipsfusion_amd import synth
    v, f = synth.box_room_mesh(synth.config_reference_defaults()["mapping"]["bound"])
    return (v + np.array([0.02, 0.0, 0.0]), f), (v, f)


def tessellated_box(lo, hi, m=12):
    """the six walls of the box lo..hi, each as m x m rectangles of two triangles -> (vertices float64, faces int64)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    tris = []
    for axis in range(3):
        a, b = [d for d in range(3) if d != axis]
        ta, tb = np.linspace(lo[a], hi[a], m + 1), np.linspace(lo[b], hi[b], m + 1)
        for at in (lo[axis], hi[axis]):
            for i in range(m):
                for j in range(m):
                    q = np.zeros((4, 3))
                    q[:, axis] = at
                    q[:, a] = [ta[i], ta[i + 1], ta[i + 1], ta[i]]
                    q[:, b] = [tb[j], tb[j], tb[j + 1], tb[j + 1]]
                    tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
    t = np.asarray(tris).reshape(-1, 3)
    vertices, inverse = np.unique(t, axis=0, return_inverse=True)
    return vertices, inverse.reshape(-1, 3).astype(np.int64)


def cull_case():
    """-> dict(vertices, faces, kf_c2w [2,4,4], kf_max_depth [2], K, W, H): two views of the reference box room"""
    import torch
    from mipsfusion_amd import synth
    cfg = synth.config_reference_defaults()
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(cfg)
    b32 = torch.as_tensor(cfg["mapping"]["bound"], dtype=torch.float32)
    v, f = tessellated_box((b32[:, 0] + 0.3).double().numpy(), (b32[:, 1] - 0.3).double().numpy())
    poses = torch.stack([synth.default_pose(cfg, yaw=0.3, pitch=-0.1), synth.default_pose(cfg, yaw=2.1, pitch=0.25)])
    return {"vertices": v, "faces": f, "kf_c2w": poses, "kf_max_depth": torch.tensor([3.0, 2.5]), "K": (fx, fy, cx, cy), "W": W, "H": H}
