"""numpy restatement of the mesh extractor (include/mipsf_mesh.h): dual means, validity, cases, the
project's own generated tables, interpolation with the snaps, soup order, weld, face filters.  fp32 wherever the extractor
is fp32, the same operations in the same order as the device kernels, so the device result must be bit-identical.
It lives under tests/ because it is a checker, not the product."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mcubes_tables", os.path.join(ROOT, "tools", "gen_mcubes_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


F32 = np.float32
THRESH = F32(10.0)
SNAP = F32(0.00001)
WELD_GRID = F32(0.00001)
# the eight voxels of a dual value in the order they are summed
SUM_ORDER = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = load_generator().tables()
    return _TABLES


def dual_field(vol, truncation):
    """-> value fp32 [X+1,Y+1,Z+1], valid bool: dual vertex a sits at a - 0.5 and averages voxels a-1, a"""
    X, Y, Z = vol.shape
    ok = (vol != -np.inf) & (np.abs(vol) < F32(truncation))
    pv = np.zeros((X + 2, Y + 2, Z + 2), F32)
    pm = np.zeros((X + 2, Y + 2, Z + 2), bool)
    pv[1:-1, 1:-1, 1:-1] = np.where(ok, vol, F32(0))
    pm[1:-1, 1:-1, 1:-1] = ok
    d = np.zeros((X + 1, Y + 1, Z + 1), F32)
    valid = np.ones((X + 1, Y + 1, Z + 1), bool)
    for a, b, c in SUM_ORDER:
        d = d + F32(0.125) * pv[a:a + X + 1, b:b + Y + 1, c:c + Z + 1]
        valid &= pm[a:a + X + 1, b:b + Y + 1, c:c + Z + 1]
    return d, valid


def thresh_rejects(d):
    """d fp32 [n,8] -> bool [n]: the per-cell rejections on thresh = 10, all 64 pairs"""
    rej = np.zeros(len(d), bool)
    for k in range(8):
        for l in range(8):
            a, b = d[:, k], d[:, l]
            rej |= np.where(a * b < 0, np.abs(a) + np.abs(b) > THRESH, np.abs(a - b) > THRESH)
    return rej | (np.abs(d) > THRESH).any(1)


def classify(vol, isovalue, truncation):
    """-> cases uint8 [X,Y,Z] (0 = emits nothing), corner values fp32 [X,Y,Z,8]"""
    X, Y, Z = vol.shape
    d, valid = dual_field(vol, truncation)
    iso = F32(isovalue)
    cv = np.stack([d[(c >> 2) & 1:((c >> 2) & 1) + X, (c >> 1) & 1:((c >> 1) & 1) + Y, (c & 1):(c & 1) + Z] for c in range(8)], -1)
    ok = np.ones((X, Y, Z), bool)
    code = np.zeros((X, Y, Z), np.int32)
    for c in range(8):
        ok &= valid[(c >> 2) & 1:((c >> 2) & 1) + X, (c >> 1) & 1:((c >> 1) & 1) + Y, (c & 1):(c & 1) + Z]
        code |= (cv[..., c] < iso).astype(np.int32) << c
    code[~ok] = 0
    code[tables()[1][code] == 0] = 0          # no crossing, or one of the patterns that emit nothing
    live = np.nonzero(code.reshape(-1))[0]
    rej = thresh_rejects(cv.reshape(-1, 8)[live])
    code.reshape(-1)[live[rej]] = 0
    return code.astype(np.uint8), cv


def edge_vertices(iso, p1, p2, d1, d2):
    """p1, p2 fp32 [n,3], d1, d2 fp32 [n] -> fp32 [n,3]"""
    with np.errstate(all="ignore"):
        mu = (iso - d1) / (d2 - d1)
        r = p1 + mu[:, None] * (p2 - p1)
    r = np.where((np.abs(d1 - d2) < SNAP)[:, None], p1, r)
    r = np.where((np.abs(iso - d2) < SNAP)[:, None], p2, r)
    r = np.where((np.abs(iso - d1) < SNAP)[:, None], p1, r)
    return r.astype(F32)


def soup(vol, isovalue, truncation, x0=0):
    """-> triangles fp32 [T,3,3] in cell order (i, j, k), k fastest, table order within a cell; cell ids int32 [T].
    x0: `vol` is the slab [x0:, :, :] of a larger volume (coordinates and cell ids are the larger volume's)"""
    ends, ntri, tri = tables()
    vol = np.ascontiguousarray(vol, F32)
    X, Y, Z = vol.shape
    code, cv = classify(vol, isovalue, truncation)
    cells = np.nonzero(code.reshape(-1))[0]
    code = code.reshape(-1)[cells].astype(np.int64)
    cv = cv.reshape(-1, 8)[cells]
    ijk = np.stack(np.unravel_index(cells, (X, Y, Z)), -1)
    ijk[:, 0] += x0
    cells = cells + x0 * Y * Z
    ijk = ijk.astype(F32)
    off = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], F32) - F32(0.5)
    iso = F32(isovalue)
    ev = np.zeros((len(cells), 12, 3), F32)
    for e in range(12):
        c1, c2 = int(ends[e, 0]), int(ends[e, 1])
        ev[:, e] = edge_vertices(iso, ijk + off[c1], ijk + off[c2], cv[:, c1], cv[:, c2])
    nt = ntri[code].astype(np.int64)
    owner = np.repeat(np.arange(len(cells)), nt)
    within = np.arange(nt.sum()) - np.repeat(np.cumsum(nt) - nt, nt)
    edges = tri[code[owner][:, None], 3 * within[:, None] + np.arange(3)[None, :]].astype(np.int64)
    return ev[owner[:, None], edges], cells[owner].astype(np.int32)


def weld_cells(v):
    s = (v > 0).astype(F32) - (v < 0).astype(F32)
    return np.trunc(v / WELD_GRID + F32(0.5) * s).astype(np.int64)


def weld(tris):
    """tris fp32 [T,3,3] -> vertices fp32 [V,3], faces int32 [T,3].  Vertices whose quantised cells are equal or adjacent are
    one vertex (connected components of that relation); the first in soup order survives; numbering by first appearance."""
    T = len(tris)
    flat = tris.reshape(-1, 3)
    if T == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    q = weld_cells(flat)
    # per axis, ranks that keep "differs by one" and nothing else, so that a cell and its neighbours become one int64 key
    r = np.zeros_like(q)
    for ax in range(3):
        u = np.unique(q[:, ax])
        rank = np.concatenate([[0], np.cumsum(np.minimum(np.diff(u), 2))]) + 1
        r[:, ax] = rank[np.searchsorted(u, q[:, ax])]
    M = int(r.max()) + 3

    def key(c):
        return (c[:, 0] * M + c[:, 1]) * M + c[:, 2]

    keys, inv = np.unique(key(r), return_inverse=True)
    inv = inv.reshape(-1)
    label = np.full(len(keys), 3 * T, np.int64)
    np.minimum.at(label, inv, np.arange(3 * T))
    first = label.copy()                    # the cell's first soup vertex: stands for the cell
    rc = r[first]
    nb = []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                k = key(rc + np.array([a, b, c]))
                pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
                nb.append(np.where(keys[pos] == k, pos, -1))
    nb = np.stack(nb, 1)
    while True:
        cand = np.where(nb >= 0, label[np.maximum(nb, 0)], 3 * T).min(1)
        new = np.minimum(label, cand)
        if np.array_equal(new, label):
            break
        label = new
    root = label[inv]
    keep = root == np.arange(3 * T)
    new_id = np.cumsum(keep) - 1
    return flat[keep].copy(), new_id[root].reshape(T, 3).astype(np.int32)


def filter_faces(faces, *per_face):
    """drop faces with a repeated index, then repeated faces (same three indices in any order; the first stays)"""
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    idx = np.nonzero(ok)[0]
    if len(idx):
        _, firsts = np.unique(np.sort(faces[idx], 1), axis=0, return_index=True)
        idx = idx[np.sort(firsts)]
    return (faces[idx],) + tuple(p[idx] for p in per_face)


def soup_in_slabs(vol, isovalue, truncation, cells_per_slab=32):
    """soup() of a large volume without its whole corner table in memory: slabs along x that overlap by the one voxel on each
    side a cell reads; a slab's own outermost cells have no valid corners, so every cell emits in exactly one slab"""
    X = vol.shape[0]
    parts = [soup(vol[max(a - 1, 0):min(a + cells_per_slab + 1, X)], isovalue, truncation, max(a - 1, 0))
             for a in range(1, max(X - 1, 2), cells_per_slab)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def marching_cubes(vol, isovalue, truncation, return_cells=False, slabs=False):
    """-> vertices float64 [V,3] (fp32 values), faces int64 [F,3] (, cell id int32 [F])"""
    tris, cells = (soup_in_slabs if slabs else soup)(vol, isovalue, truncation)
    v, f = weld(tris)
    f, cells = filter_faces(f, cells)
    out = (v.astype(np.float64), f.astype(np.int64))
    return out + (cells,) if return_cells else out


def weld_greedy(tris):
    """the upstream's sequential weld (slow; for checking that the parallel one agrees where clusters are cliques): a vertex
    joins the first registered cell among the 27 around its own, else registers its cell"""
    flat = tris.reshape(-1, 3)
    q = weld_cells(flat)
    grid, look, verts = {}, np.zeros(len(flat), np.int64), []
    for v in range(len(flat)):
        x, y, z = (int(t) for t in q[v])
        hit = -1
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                for c in (-1, 0, 1):
                    if hit < 0:
                        hit = grid.get((x + a, y + b, z + c), -1)
        if hit < 0:
            hit = grid[(x, y, z)] = len(verts)
            verts.append(flat[v])
        look[v] = hit
    return np.array(verts, F32).reshape(-1, 3), look.reshape(-1, 3).astype(np.int32)


def vector_area(tris):
    """sum of 0.5 (v1 - v0) x (v2 - v0) over triangles [n,3,3] (float64) -> [3]"""
    t = np.asarray(tris, np.float64)
    return 0.5 * np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).sum(0) if len(t) else np.zeros(3)


# ------------------------------------------------------------------------------- criteria shared by the CPU and GPU tests
MATCH_TOL = 2e-5      # the upstream's own weld reach: it calls two such vertices one
AREA_TOL = 2e-4       # a patch's perimeter is below 7 voxel lengths: moving each vertex by 2e-5 moves its vector area < 1.4e-4
SNAP_CASES = ("plane_snap", "plane_snap2")


def face_cells(vertices, faces, shape):
    c = np.floor(vertices[faces].mean(1) + 0.5).astype(np.int64)
    return (c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2]


def per_cell_area(vertices, faces, shape):
    t = vertices[faces]
    a = 0.5 * np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    out = np.zeros((int(np.prod(shape)), 3))
    np.add.at(out, face_cells(vertices, faces, shape), a)
    return out


def compare_with_reference(name, vertices, faces, g):
    """the criteria of tests/test_mcubes_cpu.py test 2 for fixture `name` of mcubes.npz; prints each figure, then asserts"""
    from scipy.spatial import cKDTree
    rv, rf = g[name + "_v"].astype(np.float64), g[name + "_f"].astype(np.int64)
    shape = g[name + "_vol"].shape
    assert len(vertices) == len(rv), (name, len(vertices), len(rv))
    d_own, to_ref = cKDTree(rv).query(vertices)
    d_ref, to_own = cKDTree(vertices).query(rv)
    print(f"{name}: V {len(vertices)}/{len(rv)} F {len(faces)}/{len(rf)} farthest match {max(d_own.max(), d_ref.max()):.3e}")
    assert d_own.max() <= MATCH_TOL and d_ref.max() <= MATCH_TOL
    assert np.array_equal(to_own[to_ref], np.arange(len(vertices))), "the match is not one-to-one"
    total = np.abs(vector_area(vertices[faces]) - vector_area(rv[rf])).max()
    print(f"{name}: total vector area differs by {total:.3e}")
    if name in SNAP_CASES:
        assert total <= AREA_TOL
        return
    assert len(faces) == len(rf)
    own, ref = per_cell_area(vertices, faces, shape), per_cell_area(rv, rf, shape)
    worst = np.abs(own - ref).max()
    print(f"{name}: worst per-cell vector area difference {worst:.3e} over {int((np.abs(ref).sum(1) > 0).sum())} cells")
    assert worst <= AREA_TOL


def emitting_region(vol, isovalue, truncation):
    """bool [X,Y,Z]: cells that emit whatever their pattern asks for (valid corners, not rejected on thresh, not one of the
    patterns recorded to emit nothing)"""
    X, Y, Z = vol.shape
    d, valid = dual_field(np.ascontiguousarray(vol, F32), truncation)
    ok = np.ones((X, Y, Z), bool)
    code = np.zeros((X, Y, Z), np.int32)
    cv = []
    for c in range(8):
        sl = (slice((c >> 2) & 1, ((c >> 2) & 1) + X), slice((c >> 1) & 1, ((c >> 1) & 1) + Y), slice(c & 1, (c & 1) + Z))
        ok &= valid[sl]
        cv.append(d[sl])
        code |= (d[sl] < F32(isovalue)).astype(np.int32) << c
    crossing = (code != 0) & (code != 255)
    ok &= ~(crossing & (tables()[1][code] == 0))
    ok &= ~thresh_rejects(np.stack(cv, -1).reshape(-1, 8)).reshape(X, Y, Z)
    return ok


def check_manifold(vertices, faces, vol, isovalue, truncation):
    """every edge is used by two faces in opposite directions, or by one if it touches a cell outside the emitting region"""
    if len(faces) == 0:
        return 0
    region = np.pad(emitting_region(vol, isovalue, truncation), 1)
    a = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
    b = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    und, inv, cnt = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True, return_counts=True)
    balance = np.zeros(len(und), np.int64)
    np.add.at(balance, inv.reshape(-1), np.where(a < b, 1, -1))
    assert cnt.max() <= 2, f"{int((cnt > 2).sum())} edges used by more than two faces"
    assert (balance[cnt == 2] == 0).all(), "an edge is used twice in the same direction"
    once = und[cnt == 1]
    mid = 0.5 * (vertices[once[:, 0]] + vertices[once[:, 1]])
    border = np.zeros(len(once), bool)
    for sx in (-1e-6, 1e-6):
        for sy in (-1e-6, 1e-6):
            for sz in (-1e-6, 1e-6):
                c = np.floor(mid + 0.5 + np.array([sx, sy, sz])).astype(np.int64) + 1
                c = np.clip(c, 0, np.array(region.shape) - 1)
                border |= ~region[c[:, 0], c[:, 1], c[:, 2]]
    assert border.all(), f"{int((~border).sum())} open edges inside the emitting region"
    return len(once)
