"""Restatement of the release, the archive and the restore of bricks of the brick-sparse TSDF volume (mipsfusion_amd/sparse_tsdf.py
release / restore / BrickArchive, csrc/sparse_release.hip, include/mipsf_sparse_release.h) in numpy, over the volumes of
tests/sparse_cpu.py (and of tests/sparse_remove_cpu.py, which add `born` per brick).  It follows the header literally: the two
predicates per slot, the candidates' prefix sum and the archive's cap, entry k of the archive = the k-th released slot, the j-th tail
survivor into the j-th hole, the restore's marks (the lowest entry wins) and sparse_cpu's own allocation order behind them.  It keeps
sparse_cpu's dense state: the voxels of a released brick go to zero and come back on restore.

Nothing here is ambiguous.  The predicates are comparisons of STORED words -- float64 ticks against the float64 words of the box,
fp32 weights against zero -- and everything else is a copy, so no result depends on the rounding of an operation and there is no
last bit that could flip a decision: the device's table, slot order, count, born, pool words, archive and records must EQUAL what
this file gives, with no tolerance.  It is a checker, not the product.
"""
import math

import numpy as np

from . import sparse_cpu as S
from . import sparse_remove_cpu as SR
from . import track_cpu as TC
from . import tsdf_cpu as T

OUTSIDE, EMPTY = 1, 2
UNBORN = SR.UNBORN
RELEASE_KEYS = ("candidates", "released", "released_outside", "released_empty", "deferred", "moved", "in_use")
RESTORE_KEYS = ("listed", "invalid", "duplicates", "occupied", "restored", "dropped", "in_use")
# the walk: the views of two_rooms/v0.20 in their order, each fused and followed by a release of the bricks outside 2 m of its camera
WALK, WALK_RADIUS = "two_rooms/v0.20", 2.0


def coords(sp, b):
    nb = sp["bricks"]
    return (int(b) // (nb[1] * nb[2]), (int(b) // nb[2]) % nb[1], int(b) % nb[2])


def brick_box(sp, b):
    """-> (blo [3], bhi [3]): the first and the last tick of brick b on every axis, read from the virtual grid's ticks"""
    ticks = T.make_ticks(sp["origin"], sp["voxel"], sp["dims"]) if "all_ticks" not in sp else sp["all_ticks"]
    sp["all_ticks"] = ticks
    c = coords(sp, b)
    lo = [ticks[a][int(S.BRICK[a]) * c[a]] for a in range(3)]
    hi = [ticks[a][min(int(S.BRICK[a]) * c[a] + int(S.BRICK[a]) - 1, sp["dims"][a] - 1)] for a in range(3)]
    return np.asarray(lo, np.float64), np.asarray(hi, np.float64)


def _slices(sp, b):
    """the voxels of brick b in the window's dense state (the brick lies in the window) -> slices, the brick's extent inside the grid"""
    c = coords(sp, b)
    first = [c[a] * int(S.BRICK[a]) for a in range(3)]
    last = [min(first[a] + int(S.BRICK[a]), sp["dims"][a]) for a in range(3)]
    assert all(sp["lo"][a] <= first[a] and last[a] <= sp["hi"][a] for a in range(3)), "a brick outside the restatement's window"
    return tuple(slice(first[a] - sp["lo"][a], last[a] - sp["lo"][a]) for a in range(3)), [last[a] - first[a] for a in range(3)]


def slot_words(sp, b):
    """the words of brick b as its slot holds them: tsdf, weight fp32 [8,8,16], color fp32 [8,8,16,3] or None; zero outside the grid"""
    sl, n = _slices(sp, b)
    st = sp["state"]
    out = []
    for key in ("tsdf", "weight", "color"):
        if st[key] is None:
            out.append(None)
            continue
        full = np.zeros(tuple(int(x) for x in S.BRICK) + st[key].shape[3:], np.float32)
        full[:n[0], :n[1], :n[2]] = st[key][sl]
        out.append(full)
    return out


def _write_words(sp, b, tsdf, weight, color):
    sl, n = _slices(sp, b)
    st = sp["state"]
    st["tsdf"][sl] = tsdf[:n[0], :n[1], :n[2]]
    st["weight"][sl] = weight[:n[0], :n[1], :n[2]]
    if st["color"] is not None:
        st["color"][sl] = color[:n[0], :n[1], :n[2]]


def pool(sp):
    """the whole pool as the device holds it -> dict(tsdf, weight fp32 [capacity,8,8,16], color or None, born int64 [capacity] with
    UNBORN beyond the count and in a volume without history None)"""
    cap = sp["capacity"]
    st = sp["state"]
    out = {"tsdf": np.zeros((cap,) + tuple(int(x) for x in S.BRICK), np.float32), "weight": np.zeros((cap,) + tuple(int(x) for x in S.BRICK), np.float32),
           "color": None if st["color"] is None else np.zeros((cap,) + tuple(int(x) for x in S.BRICK) + (3,), np.float32),
           "born": np.full(cap, UNBORN, np.int64) if "born" in sp else None}
    for s, b in enumerate(sp["slot_brick"]):
        t, w, c = slot_words(sp, b)
        out["tsdf"][s], out["weight"][s] = t, w
        if c is not None:
            out["color"][s] = c
        if "born" in sp:
            out["born"][s] = sp["born"][b]
    return out


def flags_of(sp, box=None, empty=False):
    """the predicates per slot in use -> int64 [count]: OUTSIDE | EMPTY"""
    f = np.zeros(len(sp["slot_brick"]), np.int64)
    if box is not None:
        box = np.asarray(box, np.float64).reshape(6)
    for s, b in enumerate(sp["slot_brick"]):
        if box is not None:
            blo, bhi = brick_box(sp, b)
            with np.errstate(invalid="ignore"):
                if any(bool(bhi[a] < box[a]) or bool(blo[a] > box[3 + a]) for a in range(3)):
                    f[s] |= OUTSIDE
        if empty and not (slot_words(sp, b)[1] > 0).any():
            f[s] |= EMPTY
    return f


def release(sp, box=None, empty=False, archive_capacity=None):
    """mipsf_sparse_release -> (record dict, archive dict(bricks, born, tsdf, weight, color; the entries written) or None)"""
    assert box is not None or empty
    f = flags_of(sp, box, empty)
    n = len(f)
    r = f != 0
    Rs = np.cumsum(r) - r                                                    # exclusive
    cap = math.inf if archive_capacity is None else int(archive_capacity)
    gone = r & (Rs < cap)
    released = [s for s in range(n) if gone[s]]                              # ascending
    after = n - len(released)
    archive = None
    if archive_capacity is not None:
        words = [slot_words(sp, sp["slot_brick"][s]) for s in released]
        archive = {"bricks": np.asarray([sp["slot_brick"][s] for s in released], np.int64),
                   "born": np.asarray([sp["born"][sp["slot_brick"][s]] for s in released], np.int64) if "born" in sp else None,
                   "tsdf": np.stack([w[0] for w in words]) if words else np.zeros((0,) + tuple(int(x) for x in S.BRICK), np.float32),
                   "weight": np.stack([w[1] for w in words]) if words else np.zeros((0,) + tuple(int(x) for x in S.BRICK), np.float32),
                   "color": None if sp["state"]["color"] is None else
                   (np.stack([w[2] for w in words]) if words else np.zeros((0,) + tuple(int(x) for x in S.BRICK) + (3,), np.float32))}
    holes = [s for s in released if s < after]
    survivors = [s for s in range(after, n) if not gone[s]]
    assert len(holes) == len(survivors)
    slots = list(sp["slot_brick"])
    for s in released:                                                       # the dense state, the table and the history of the released
        b = slots[s]
        zero = np.zeros(tuple(int(x) for x in S.BRICK), np.float32)
        _write_words(sp, b, zero, zero, np.zeros(zero.shape + (3,), np.float32))
        sp["table"][b] = -1
        if "born" in sp:
            sp["born"][b] = UNBORN
    for hole, s in zip(holes, survivors):
        slots[hole] = slots[s]
        sp["table"][slots[s]] = hole
    sp["slot_brick"] = slots[:after]
    rec = {"candidates": int(r.sum()), "released": len(released), "released_outside": int(((f & OUTSIDE) != 0)[gone].sum()),
           "released_empty": int(((f & EMPTY) != 0)[gone].sum()), "deferred": int(r.sum()) - len(released), "moved": len(holes), "in_use": after}
    return rec, archive


def restore(sp, archive, m=None):
    """mipsf_sparse_restore of the first m entries -> record dict"""
    bricks = np.asarray(archive["bricks"], np.int64)
    m = len(bricks) if m is None else int(m)
    if m == 0:
        return dict.fromkeys(RESTORE_KEYS, 0)
    total = int(np.prod(sp["bricks"]))
    mark = np.full(total, S.UNMARKED, np.int64)
    invalid = 0
    for k in range(m):
        b = int(bricks[k])
        if 0 <= b < total:
            mark[b] = min(mark[b], k)
        else:
            invalid += 1
    marked = np.flatnonzero(mark != S.UNMARKED)
    want = [int(b) for b in marked if sp["table"][b] < 0]                    # ascending brick index
    room = sp["capacity"] - len(sp["slot_brick"])
    for b in want[:room]:
        k = int(mark[b])
        sp["table"][b] = len(sp["slot_brick"])
        sp["slot_brick"].append(b)
        _write_words(sp, b, archive["tsdf"][k], archive["weight"][k], None if archive["color"] is None else archive["color"][k])
        if "born" in sp:
            sp["born"][b] = int(archive["born"][k])
    got = min(len(want), room)
    return {"listed": m, "invalid": invalid, "duplicates": m - invalid - len(marked), "occupied": len(marked) - len(want), "restored": got,
            "dropped": len(want) - got, "in_use": len(sp["slot_brick"])}


def cat(archives):
    keys = ("bricks", "born", "tsdf", "weight", "color")
    return {k: None if archives[0][k] is None else np.concatenate([a[k] for a in archives]) for k in keys}


def copy_volume(sp):
    out = dict(sp, table=sp["table"].copy(), slot_brick=list(sp["slot_brick"]), state={k: (None if v is None else v.copy()) for k, v in sp["state"].items()},
               ambiguous=sp["ambiguous"].copy())
    if "born" in sp:
        out["born"] = sp["born"].copy()
    return out


def planted(bricks, slot_order, capacity, color=False, history=False, seed=0, empty=()):
    """A volume made by hand: a virtual grid of `bricks` = (BX, BY, BZ) whole bricks, the bricks `slot_order` (linear indices) in the
    slots 0, 1, .. with seeded words in every voxel (weights 1 .. 4; all zero in the slots listed in `empty`), born = 5 + slot"""
    dims = tuple(int(n) * int(b) for n, b in zip(bricks, S.BRICK))
    sp = (SR.new_volume if history else S.new_volume)(np.zeros(3), 0.125, dims, 0.5, capacity, color)
    rng = np.random.default_rng(seed)
    st = sp["state"]
    mask = np.zeros(int(np.prod(bricks)), bool)
    mask[np.asarray(slot_order, np.int64)] = True
    m = S._voxel_mask(sp, mask)
    st["tsdf"][...] = np.where(m, rng.uniform(-1, 1, dims).astype(np.float32), 0)
    st["weight"][...] = np.where(m, rng.integers(1, 5, dims).astype(np.float32), 0)
    if color:
        st["color"][...] = np.where(m[..., None], rng.uniform(0, 1, dims + (3,)).astype(np.float32), 0)
    for s, b in enumerate(slot_order):
        sp["table"][b] = s
        sp["slot_brick"].append(int(b))
        if history:
            sp["born"][b] = 5 + s
        if s in empty:
            zero = np.zeros(tuple(int(x) for x in S.BRICK), np.float32)
            _write_words(sp, b, zero if s % 2 else -zero - 1.0, zero, np.zeros(zero.shape + (3,), np.float32))
    if history:
        sp["serial"] = 5 + len(slot_order)
    return sp


def keep_box(pose, radius):
    """the box sparse_tsdf_odometry(keep_radius=...) makes on the device: the fp32 position widened, minus and plus the radius"""
    t = np.asarray(pose, np.float32)[:3, 3].astype(np.float64)
    return np.concatenate([t - float(radius), t + float(radius)])


# ------------------------------------------------------------------------------------------------------------ the walk
_walk = {}


def walk_marks():
    """The walk on sparse_cpu.marks alone: per view the bricks it marks, and the live set when every view is followed by a release of
    the bricks outside WALK_RADIUS of its camera -> dict(union: bricks marked by any view, peak: the largest live set, before a
    release, live: per view the live set before its release); computed once"""
    if "marks" not in _walk:
        c = S.inputs(WALK)
        sp = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], 1)
        live, union, sizes = set(), set(), []
        for k in range(len(c["depth"])):
            mark, _ = S.marks(sp, c["depth"][k:k + 1], c["poses"][k:k + 1], c["K"], c["depth_max"])
            got = set(int(b) for b in np.flatnonzero(mark != S.UNMARKED))
            live |= got
            union |= got
            sizes.append(len(live))
            box = keep_box(c["poses"][k].numpy(), WALK_RADIUS)
            live = set(b for b in live if not any(brick_box(sp, b)[1][a] < box[a] or brick_box(sp, b)[0][a] > box[3 + a] for a in range(3)))
        _walk["marks"] = {"union": len(union), "peak": max(sizes), "live": sizes}
    return _walk["marks"]


def walk(capacity, radius=WALK_RADIUS, views=None):
    """the walk with the restatement's volume: every view fused at its pose, then (with a radius) the release around it
    -> (volume, per view dict(dropped, in_use before the release, released))"""
    c = S.inputs(WALK)
    sp = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], capacity)
    out = []
    for k in range(len(c["depth"]) if views is None else views):
        got = S.integrate(sp, c["depth"][k:k + 1], c["poses"][k:k + 1], c["K"], None, c["depth_max"])
        rec = {"dropped": got["dropped"], "in_use": got["in_use"], "released": 0}
        if radius is not None:
            rec["released"] = release(sp, keep_box(c["poses"][k].numpy(), radius))[0]["released"]
        out.append(rec)
    return sp, out


def odometry_step(sp, prev_pose, depth, K, H, W, **kw):
    """one frame of sparse_tsdf_odometry on the host: the ray cast from the previous pose and the registration against it"""
    m = S.raycast(sp, np.asarray(prev_pose, np.float32)[None], K, H, W)
    return TC.register(m["depth"][0], m["normals"][0], prev_pose, depth, prev_pose, K, max_dist=sp["trunc"], **kw)
