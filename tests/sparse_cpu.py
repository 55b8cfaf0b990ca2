"""Float64 restatement of the brick-sparse TSDF volume (mipsfusion_amd/sparse_tsdf.py, csrc/sparse.hip, include/mipsf_sparse.h) in
numpy.  A brick-sparse volume is a dense volume in which a voxel is updated only while its brick is allocated, so this file holds
only what is new -- the allocation rule, following the header literally (every pixel, every step of the band, every corner; births
per call, slots in ascending brick order, drops when the pool is full) -- and applies tests/tsdf_cpu.py's `integrate` view by view
under the mask of the bricks that take the view.  The ray cast and the mesh are tests/track_cpu.py's `raycast` and tsdf_cpu's
`extract_mesh` applied to its state ("the masked dense state").  The dense state is kept over a WINDOW of the virtual grid, with
the virtual grid's ticks sliced, so a grid of 2048^3 voxels costs what its room costs.  The device's table, slots, births, counts
and words must EQUAL what this file gives.  It is a checker, not the product.  It also holds the cases the tests share, each
computed once.
"""
import math

import numpy as np

from . import raster_cpu as R
from . import track_cpu as K_
from . import tsdf_cpu as T

BRICK = np.asarray(T.BRICK, np.int64)
UNMARKED = 0xFFFFFFFF
LAST_BITS = 64 * 2.0 ** -52           # of a float64 of magnitude 1


def bricks_of(dims):
    return tuple(int(-(-int(d) // int(b))) for d, b in zip(dims, BRICK))


def new_volume(origin, voxel, dims, trunc, capacity, color=False, max_weight=math.inf, band=None, lo=None, hi=None):
    """an empty sparse volume; the dense state covers the window lo <= voxel index < hi (lo on brick boundaries; the whole grid by
    default)"""
    dims = tuple(int(d) for d in dims)
    lo = (0, 0, 0) if lo is None else tuple(int(x) for x in lo)
    hi = dims if hi is None else tuple(int(x) for x in hi)
    assert all(a % b == 0 and 0 <= a < c <= d for a, b, c, d in zip(lo, BRICK, hi, dims))
    origin = np.asarray(origin, np.float64)
    band = float(trunc) if band is None else float(band)
    ticks = T.make_ticks(origin, voxel, dims)
    nb = bricks_of(dims)
    return {"origin": origin, "voxel": float(voxel), "dims": dims, "trunc": float(trunc), "capacity": int(capacity), "max_weight": float(max_weight),
            "band": band, "steps": int(math.ceil(band / float(voxel))), "bricks": nb, "table": np.full(nb[0] * nb[1] * nb[2], -1, np.int32),
            "slot_brick": [], "lo": lo, "hi": hi, "ticks": [t[a:b] for t, a, b in zip(ticks, lo, hi)],
            "window_origin": origin + float(voxel) * np.asarray(lo, np.float64),
            "state": T.new_state([b - a for a, b in zip(lo, hi)], color), "ambiguous": np.zeros(3, np.int64)}


# ------------------------------------------------------------------------------------------------------------ the allocation rule
def marks(sp, depth, poses, K, depth_max=math.inf):
    """the header's marks of one call -> (mark uint32 [bricks], [z within 1e-12 of 0, i0 coordinates within 1e-9 of an integer, i0
    coordinates within 64 last bits of an integer])"""
    fx, fy, cx, cy = R.intrinsics(K)
    D = np.asarray(depth, np.float32)
    P = R._poses(poses) if len(D) else np.zeros((0, 4, 4))
    nb = sp["bricks"]
    mark = np.full(nb[0] * nb[1] * nb[2], UNMARKED, np.uint32)
    origin, voxel, dims = sp["origin"], sp["voxel"], sp["dims"]
    ambiguous = np.zeros(3, np.int64)
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            H, W = D[k].shape
            row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
            d = D[k].astype(np.float64)
            usable = (d > 0) & (d < np.inf) & (d <= depth_max)
            row, col, d = row[usable], col[usable], d[usable]
            for j in range(-sp["steps"], sp["steps"] + 1):
                z = d + float(j) * voxel
                go = z > 0
                ambiguous[0] += int((np.abs(z) < 1e-12).sum())
                pc = (z * ((col - cx) / fx), -(z * ((row - cy) / fy)), -z)
                i0 = []
                for a in range(3):
                    p = ((pose[a, 0] * pc[0] + pose[a, 1] * pc[1]) + pose[a, 2] * pc[2]) + pose[a, 3]
                    g = (p - origin[a]) / voxel
                    off = np.abs(g - np.round(g))
                    ambiguous[1] += int((go & (off < 1e-9)).sum())
                    ambiguous[2] += int((go & (off <= LAST_BITS * np.maximum(np.abs(g), 1.0))).sum())
                    i0.append(np.floor(g))
                for corner in range(8):
                    c = [i0[a] + 2.0 if corner & (4 >> a) else i0[a] - 1.0 for a in range(3)]
                    ok = go.copy()
                    for a in range(3):
                        ok &= (c[a] >= 0.0) & (c[a] <= float(dims[a]) - 1.0)
                    ci = [np.where(ok, c[a], 0.0).astype(np.int64)[ok] for a in range(3)]
                    b = ((ci[0] // BRICK[0]) * nb[1] + ci[1] // BRICK[1]) * nb[2] + ci[2] // BRICK[2]
                    np.minimum.at(mark, b, np.uint32(k))
    return mark, ambiguous


def allocate(sp, depth, poses, K, depth_max=math.inf):
    """one call of mipsf_sparse_allocate -> dict(marked, new, dropped, in_use, birth int64 [bricks]: the first view of this call a
    brick takes, -1 without a slot)"""
    mark, amb = marks(sp, depth, poses, K, depth_max)
    sp["ambiguous"] += amb
    table = sp["table"]
    birth = np.where(table >= 0, 0, -1).astype(np.int64)
    want = np.flatnonzero((mark != UNMARKED) & (table < 0))                                   # ascending brick index
    room = sp["capacity"] - len(sp["slot_brick"])
    got = want[:room]
    for b in got:
        table[b] = len(sp["slot_brick"])
        sp["slot_brick"].append(int(b))
    birth[got] = mark[got].astype(np.int64)
    return {"marked": int((mark != UNMARKED).sum()), "new": len(got), "dropped": len(want) - len(got), "in_use": len(sp["slot_brick"]), "birth": birth}


def _voxel_mask(sp, brick_mask):
    """bool [bricks] -> bool over the window's voxels"""
    nb, lo, hi = sp["bricks"], sp["lo"], sp["hi"]
    m = brick_mask.reshape(nb)
    first = [a // int(b) for a, b in zip(lo, BRICK)]
    last = [-(-c // int(b)) for c, b in zip(hi, BRICK)]
    m = m[first[0]:last[0], first[1]:last[1], first[2]:last[2]]
    for a in range(3):
        m = np.repeat(m, int(BRICK[a]), axis=a)
    return m[:hi[0] - lo[0], :hi[1] - lo[1], :hi[2] - lo[2]]


def inside_window(sp):
    """whether every allocated brick lies in the window (the counts below are the device's only then)"""
    full = np.zeros(sp["table"].shape, bool)
    full[np.asarray(sp["slot_brick"], np.int64)] = True
    return int(full.sum()) == int(_voxel_mask(sp, full)[::int(BRICK[0]), ::int(BRICK[1]), ::int(BRICK[2])].sum())


def integrate(sp, depth, poses, K, rgb=None, depth_max=math.inf, views_per_call=None):
    """SparseTSDFVolume.integrate -> dict(updates, observed, marked, new, dropped, in_use, births: {brick: view of its call})"""
    D = np.asarray(depth, np.float32)
    D = D[None] if D.ndim == 2 else D
    P = R._poses(poses) if len(D) else np.zeros((0, 4, 4))
    n = len(D)
    per = max(n, 1) if views_per_call is None else int(views_per_call)
    out = {"updates": 0, "observed": 0, "marked": 0, "new": 0, "dropped": 0, "in_use": 0, "births": {}}
    for first in range(0, max(n, 1), per):
        d, p = D[first:first + per], P[first:first + per]
        c3 = None if rgb is None else np.asarray(rgb, np.float32)[first:first + per]
        before = len(sp["slot_brick"])
        a = allocate(sp, d, p, K, depth_max)
        for b in sp["slot_brick"][before:]:
            out["births"][b] = int(a["birth"][b])
        for key in ("marked", "new", "dropped"):
            out[key] += a[key]
        out["in_use"] = a["in_use"]
        st = sp["state"]
        for k in range(len(d)):
            mask = _voxel_mask(sp, (a["birth"] >= 0) & (a["birth"] <= k))
            trial = {key: (None if v is None else v.copy()) for key, v in st.items()}
            _, _, pairs = T.integrate(trial, sp["ticks"], d[k:k + 1], p[k:k + 1], K, sp["trunc"], depth_max, sp["max_weight"],
                                      None if c3 is None else c3[k:k + 1], return_pairs=True)
            out["updates"] += int((pairs[0] & mask).sum())
            st["tsdf"] = np.where(mask, trial["tsdf"], st["tsdf"])
            st["weight"] = np.where(mask, trial["weight"], st["weight"])
            if st["color"] is not None:
                st["color"] = np.where(mask[..., None], trial["color"], st["color"])
        out["observed"] = int((st["weight"] > 0).sum())
    return out


def table_of(sp):
    return sp["table"].reshape(sp["bricks"])


# ------------------------------------------------------------------------------------------------------------ the masked dense state
class Windowed:
    """the masked dense state of the WHOLE virtual grid as track_cpu.field and tsdf_cpu.sample_color read it (`.shape` and an index
    by three integer arrays): the window's words inside the window, zero outside"""

    def __init__(self, a, lo, dims):
        self.a, self.lo, self.shape = a, lo, tuple(dims) + a.shape[3:]

    def __getitem__(self, idx):
        rel = [np.asarray(i, np.int64) - l for i, l in zip(idx, self.lo)]
        ok = np.ones(rel[0].shape, bool)
        for r, s in zip(rel, self.a.shape):
            ok &= (r >= 0) & (r < s)
        got = self.a[tuple(np.where(ok, r, 0) for r in rel)]
        return np.where(ok.reshape(ok.shape + (1,) * (got.ndim - ok.ndim)), got, np.zeros((), self.a.dtype))


def virtual_state(sp):
    st = sp["state"]
    if sp["lo"] == (0, 0, 0) and sp["hi"] == sp["dims"]:
        return st
    return {k: (None if v is None else Windowed(v, sp["lo"], sp["dims"])) for k, v in st.items()}


def raycast(sp, poses, K, H, W, step=None, **kw):
    """track_cpu.raycast over the masked dense state; the box is the virtual grid's"""
    return K_.raycast(virtual_state(sp), sp["origin"], sp["voxel"], poses, K, H, W, 0.5 * sp["trunc"] if step is None else step, **kw)


def window_state(sp, lo=None, hi=None):
    """the window lo .. hi (voxel indices of the virtual grid, inside the state's window; all of it by default) as a dense state"""
    lo = sp["lo"] if lo is None else tuple(lo)
    hi = sp["hi"] if hi is None else tuple(hi)
    sl = tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, sp["lo"]))
    return {k: (None if v is None else np.ascontiguousarray(v[sl])) for k, v in sp["state"].items()}


def extract_mesh(sp, lo=None, hi=None, min_weight=1.0):
    """tsdf_cpu.extract_mesh of window_state(lo, hi) -> (world vertices, faces, index-unit vertices)"""
    first = sp["lo"] if lo is None else tuple(lo)
    return T.extract_mesh(window_state(sp, lo, hi), sp["origin"] + sp["voxel"] * np.asarray(first, np.float64), sp["voxel"], min_weight)


def tight_window(sp):
    nb = sp["bricks"]
    b = np.asarray(sp["slot_brick"], np.int64)
    c = np.stack([b // (nb[1] * nb[2]), (b // nb[2]) % nb[1], b % nb[2]], 1)
    return tuple(int(x) for x in c.min(0) * BRICK), tuple(int(x) for x in np.minimum((c.max(0) + 1) * BRICK, np.asarray(sp["dims"])))


# ------------------------------------------------------------------------------------------------------------ cases
BOX80 = "box/80x112/v0.05/t4"
BOX_CASES = ("box/40x56/v0.15/t4", "box/40x56/v0.10/t4", BOX80)          # the three convex volumes the sparse state is held to the dense one on
VIRTUAL = "virtual_2048"                                                 # the 0.10 room inside 2048^3 voxels, at brick (100, 37, 61)
VIRTUAL_DIMS, VIRTUAL_BRICK = (2048, 2048, 2048), (100, 37, 61)
GPU_CASES = ("box/40x56/v0.10/t4", "two_rooms/v0.20", "bad_pixels", "colour", "max_weight_2", "one_voxel", "1x5x70", "many_views", "nan_pose", VIRTUAL)
_inputs, _cases = {}, {}


def _turn(yaw, pitch):
    cy, sy, cp, sp_ = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    return np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp_], [0.0, sp_, cp]])


def _settled(c, render):
    """The case with every view moved slightly that holds a decision a last-bit difference could flip.  Several of tsdf_cpu's box
    views look straight at a wall from a distance that fp32 holds exactly (the difference of two fp32 coordinates), so every pixel on
    that wall lands ON a lattice plane, step after step of the band, and a floor is decided by the last bit thousands of times.
    Such a view is turned by 0.011 and 0.007 rad about its own axes and its depth image rendered again (render: pose fp32 [4,4]
    tensor -> depth [H,W]); nothing else of the case changes."""
    poses, depth, moved = c["poses"].clone(), c["depth"].copy(), []
    probe = new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], 1)
    for k in range(len(poses)):
        _, amb = marks(probe, depth[k:k + 1], poses[k:k + 1], c["K"], c["depth_max"])
        if amb[0] or amb[2]:
            R3 = poses[k, :3, :3].numpy().astype(np.float64) @ _turn(0.011, 0.007)
            poses[k, :3, :3] = poses.new_tensor(R3.astype(np.float32))
            depth[k] = render(poses[k])
            moved.append(k)
    return dict(c, poses=poses, depth=depth, moved=tuple(moved))


def _render_box(c):
    return lambda pose: T.box_depth(pose[None], c["K"], c["H"], c["W"])[0]


def _render_rooms(c):
    from mipsfusion_amd import synth
    Tr = synth.TWO_ROOMS
    return lambda pose: synth.render_rooms_frame(Tr["room_a"], Tr["room_b"], Tr["door"], pose, c["H"], c["W"], *c["K"], seed=3)["depth"].numpy()


SETTLED = ("box/40x56/v0.15/t4", "box/40x56/v0.10/t4", "max_weight_2", "one_voxel", "1x5x70", "many_views", "two_rooms/v0.20")   # and BOX80


def inputs(name):
    """name -> the inputs of a case: tsdf_cpu's (settled, above), or made here"""
    if name in _inputs:
        return _inputs[name]
    if name == BOX80:
        H, W, K = 80, 112, (80.0, 80.0, 55.5, 39.5)
        poses = T.box_poses20()
        voxel = 0.05
        origin, dims = T.box_grid(voxel)
        c = {"origin": np.asarray(origin, np.float64), "voxel": voxel, "dims": tuple(dims), "trunc": 4 * voxel, "depth": T.box_depth(poses, K, H, W),
             "rgb": None, "poses": poses, "K": K, "H": H, "W": W, "depth_max": math.inf, "max_weight": math.inf}
    elif name == "nan_pose":                                     # view 2 of six has a NaN pose: it marks and updates nothing
        b = T.case("box/33x47/v0.20/t3")
        poses = b["poses"][:6].clone()
        poses[2] = float("nan")
        c = dict(b, poses=poses, depth=b["depth"][:6])
    elif name == VIRTUAL:
        b = inputs("box/40x56/v0.10/t4")
        shift = np.asarray(VIRTUAL_BRICK, np.float64) * BRICK
        c = dict(b, origin=b["origin"] - b["voxel"] * shift, dims=VIRTUAL_DIMS)
    else:
        c = T.case(name)
    if name in SETTLED or name == BOX80:
        c = _settled(c, _render_rooms(c) if name == "two_rooms/v0.20" else _render_box(c))
    c = {k: v for k, v in c.items() if k not in ("state", "updates", "observed", "updated")}      # tsdf_cpu's dense answer is not an input
    _inputs[name] = c
    return c


def window_of(name):
    """the window the restatement keeps its dense state over: the whole grid, or for the virtual grid the room's bricks and one more
    on every side (the band reaches six voxels past a wall, the room's own grid three)"""
    if name != VIRTUAL:
        return None, None
    room = bricks_of(T.case("box/40x56/v0.10/t4")["dims"])
    lo = [(v - 1) * int(b) for v, b in zip(VIRTUAL_BRICK, BRICK)]
    hi = [(v + r + 1) * int(b) for v, r, b in zip(VIRTUAL_BRICK, room, BRICK)]
    return lo, hi


def fuse(name, capacity=None, views_per_call=None, band=None):
    """a fresh sparse volume of the case's inputs, fused -> (volume, counts)"""
    c = inputs(name)
    nb = bricks_of(c["dims"])
    lo, hi = window_of(name)
    sp = new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], min(nb[0] * nb[1] * nb[2], 1024) if capacity is None else capacity,
                    c["rgb"] is not None, c["max_weight"], band, lo, hi)
    counts = integrate(sp, c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], views_per_call)
    return sp, counts


def dense(name):
    """the dense restatement of the case's inputs -> state (tsdf_cpu.integrate over the whole grid); computed once"""
    if ("dense", name) not in _cases:
        c = inputs(name)
        st = T.new_state(c["dims"], c["rgb"] is not None)
        T.integrate(st, T.make_ticks(c["origin"], c["voxel"], c["dims"]), c["depth"], c["poses"], c["K"], c["trunc"], c["depth_max"], c["max_weight"], c["rgb"])
        _cases[("dense", name)] = st
    return _cases[("dense", name)]


def case(name):
    """name -> dict(the inputs, sp: the restatement's volume after one call over all views, counts); computed once"""
    if name not in _cases:
        sp, counts = fuse(name)
        assert inside_window(sp), name
        _cases[name] = dict(inputs(name), sp=sp, counts=counts)
    return _cases[name]
