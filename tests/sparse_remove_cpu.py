"""Float64 restatement of the removal of fused views from the brick-sparse TSDF volume (mipsfusion_amd/sparse_tsdf.py deintegrate and
reintegrate, csrc/sparse_remove.hip, include/mipsf_sparse_remove.h) in numpy.  It holds only what is new: tests/sparse_cpu.py's
`allocate` with `born` -- the id of the first view a brick took -- kept per brick as mipsf_sparse_stamp keeps it per slot, and,
view by view in the order given, tests/tsdf_cpu.py's `integrate` and tests/tsdf_remove_cpu.py's `remove` on the dense state of the
window under the mask of the bricks with born <= the view's id.  The counts are taken under the same mask: the (voxel, view) pairs
of a view are tsdf_cpu's `updated`, a pair in the mask is removed where the weight was positive and missing where it was not, and
emptied where the weight then is zero.  The device's words, its five counts, `born` and `serial` must EQUAL what this file gives.
It is a checker, not the product.  It also holds the cases the tests share, each computed once.
"""
import math

import numpy as np

from . import raster_cpu as R
from . import sparse_cpu as S
from . import tsdf_cpu as T
from . import tsdf_remove_cpu as RM

UNBORN = -1                            # MIPSF_SPARSE_UNBORN, as the int64 arrays here hold it
REVERSED = "box/40x56/v0.10/t4/reversed"      # the box room's 20 views fused last first: bricks are born late, after views that see them
DRIFT = "box/40x56/v0.10/t4"           # the case of the drift route
GPU_CASES = (REVERSED, "colour", "two_rooms/v0.20", "bad_pixels", "nan_pose", "many_views", "1x5x70", "one_voxel", S.VIRTUAL)
# |tsdf| and |colour| of a removal with history against the fusion that skipped the removed views at the fusion step: four times the
# largest difference this restatement shows in each group of cases (printed by tests/test_sparse_remove_cpu.py, which also holds
# the measured figures to these constants); room for rounding, not a target.  Measured:
#   REVERSED, two_rooms/v0.20, bad_pixels, nan_pose, 1x5x70, one_voxel, virtual_2048 (weights up to 5)   2^-22 at most
#   colour (weights up to 3)                                                                         2^-24, tsdf and colour
#   many_views (257 views, weights up to 65)                                                         10 * 2^-22 = 2.38e-6
MEASURED = {"many_views": 10.0 * 2.0 ** -22, "colour": 2.0 ** -24}
MEASURED_DEFAULT = 2.0 ** -22


def gate(name):
    """the gate of |tsdf| and of |colour| for a case"""
    return 4.0 * MEASURED.get(name, MEASURED_DEFAULT)


_cases = {}


def new_volume(*args, **kw):
    """sparse_cpu.new_volume with the history: born int64 [bricks] (UNBORN: the brick took no view yet), serial"""
    sp = S.new_volume(*args, **kw)
    sp["born"] = np.full(sp["table"].shape, UNBORN, np.int64)
    sp["serial"] = 0
    return sp


def took(sp, view_id, history=True):
    """bool over the window's voxels: the voxels of the bricks that hold view `view_id` (without the history: of every brick with a
    slot, which is what a removal that forgot the births would touch)"""
    born = sp["born"]
    return S._voxel_mask(sp, (sp["table"] >= 0) & ((born != UNBORN) & (born <= view_id) if history else True))


def _step(sp, mask, trial):
    st = sp["state"]
    st["tsdf"] = np.where(mask, trial["tsdf"], st["tsdf"])
    st["weight"] = np.where(mask, trial["weight"], st["weight"])
    if st["color"] is not None:
        st["color"] = np.where(mask[..., None], trial["color"], st["color"])


def integrate(sp, depth, poses, K, rgb=None, depth_max=math.inf, views_per_call=None, skip=()):
    """SparseTSDFVolume.integrate with history=True -> dict(updates, observed, marked, new, dropped, in_use, ids int64 [n]).  The
    views whose id is in `skip` allocate and are stamped like the others and are left out at the fusion step: what the volume should
    hold once they are removed again."""
    D = np.asarray(depth, np.float32)
    D = D[None] if D.ndim == 2 else D
    P = R._poses(poses) if len(D) else np.zeros((0, 4, 4))
    n = len(D)
    per = max(n, 1) if views_per_call is None else int(views_per_call)
    out = {"updates": 0, "observed": 0, "marked": 0, "new": 0, "dropped": 0, "in_use": 0, "ids": sp["serial"] + np.arange(n, dtype=np.int64)}
    skip = set(int(x) for x in skip)
    for first in range(0, max(n, 1), per):
        d, p = D[first:first + per], P[first:first + per]
        c3 = None if rgb is None else np.asarray(rgb, np.float32)[first:first + per]
        a = S.allocate(sp, d, p, K, depth_max)
        for key in ("marked", "new", "dropped"):
            out[key] += a[key]
        out["in_use"] = a["in_use"]
        fresh = (a["birth"] >= 0) & (sp["born"] == UNBORN)                         # mipsf_sparse_stamp
        sp["born"][fresh] = sp["serial"] + a["birth"][fresh]
        for k in range(len(d)):
            view_id = sp["serial"] + k
            if view_id in skip:
                continue
            mask = took(sp, view_id)
            trial = RM.copy_state(sp["state"])
            _, _, pairs = T.integrate(trial, sp["ticks"], d[k:k + 1], p[k:k + 1], K, sp["trunc"], depth_max, sp["max_weight"],
                                      None if c3 is None else c3[k:k + 1], return_pairs=True)
            out["updates"] += int((pairs[0] & mask).sum())
            _step(sp, mask, trial)
        sp["serial"] += len(d)
        out["observed"] = int((sp["state"]["weight"] > 0).sum())
    return out


def bricks_emptied(sp):
    """slots in use without a voxel of positive weight (all of whose bricks lie in the window)"""
    live = np.zeros(sp["table"].shape, bool)
    w = sp["state"]["weight"] > 0
    lo, nb = sp["lo"], sp["bricks"]
    for b in sp["slot_brick"]:
        c = (b // (nb[1] * nb[2]), (b // nb[2]) % nb[1], b % nb[2])
        sl = tuple(slice(int(c[a] * S.BRICK[a]) - lo[a], int((c[a] + 1) * S.BRICK[a]) - lo[a]) for a in range(3))
        live[b] = w[sl].any()
    return len(sp["slot_brick"]) - int(live.sum())


def remove(sp, depth, poses, K, ids, rgb=None, depth_max=math.inf, history=True):
    """SparseTSDFVolume.deintegrate -> (removed, missing, emptied, observed, bricks_emptied, pairs outside the history: (voxel,
    view) pairs the views hit in voxels of bricks with a slot that were born after the view)"""
    D = np.asarray(depth, np.float32)
    D = D[None] if D.ndim == 2 else D
    P = R._poses(poses) if len(D) else np.zeros((0, 4, 4))
    ids = np.asarray(ids, np.int64).reshape(-1)
    assert len(ids) == len(D) == len(P)
    removed = missing = emptied = late = 0
    for k in range(len(D)):
        mask = took(sp, int(ids[k]), history)
        st = sp["state"]
        c3 = None if rgb is None else np.asarray(rgb, np.float32)[k:k + 1]
        trial = RM.copy_state(st)
        RM.remove(trial, sp["ticks"], D[k:k + 1], P[k:k + 1], K, sp["trunc"], depth_max, c3)
        # the pairs of the view: `updated` of the fusion, on a scratch state (the words of a fusion do not decide what is updated)
        scratch = T.new_state(st["tsdf"].shape, st["color"] is not None)
        hit = T.integrate(scratch, sp["ticks"], D[k:k + 1], P[k:k + 1], K, sp["trunc"], depth_max, rgb=c3, return_pairs=True)[2][0]
        have = hit & mask & (st["weight"] > 0)
        removed += int(have.sum())
        missing += int((hit & mask & ~(st["weight"] > 0)).sum())
        emptied += int((have & ~(trial["weight"] > 0)).sum())
        late += int((hit & took(sp, 0, False) & ~took(sp, int(ids[k]))).sum())
        _step(sp, mask, trial)
    return removed, missing, emptied, int((sp["state"]["weight"] > 0).sum()), bricks_emptied(sp), late


# ------------------------------------------------------------------------------------------------------------ cases
def inputs(name):
    """sparse_cpu.inputs; REVERSED is the box room's views in reversed order"""
    if name != REVERSED:
        return S.inputs(name)
    if name not in _cases:
        c = S.inputs(DRIFT)
        import torch
        _cases[name] = dict(c, poses=torch.flip(c["poses"], [0]).contiguous(), depth=np.ascontiguousarray(c["depth"][::-1]))
    return _cases[name]


def fresh(name, capacity=None):
    c = inputs(name)
    nb = S.bricks_of(c["dims"])
    lo, hi = S.window_of(name)
    return new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], min(nb[0] * nb[1] * nb[2], 1024) if capacity is None else capacity,
                      c["rgb"] is not None, math.inf, None, lo, hi)


def fuse(name, poses=None, views_per_call=None, skip=(), capacity=None):
    """a fresh volume with history of the case's inputs, fused (at `poses` when given) -> (volume, counts)"""
    c = inputs(name)
    sp = fresh(name, capacity)
    return sp, integrate(sp, c["depth"], c["poses"] if poses is None else poses, c["K"], c["rgb"], c["depth_max"], views_per_call, skip)


def copy_volume(sp):
    out = dict(sp, table=sp["table"].copy(), slot_brick=list(sp["slot_brick"]), born=sp["born"].copy(), state=RM.copy_state(sp["state"]),
               ambiguous=sp["ambiguous"].copy())
    return out


def _views(c, views, poses=None):
    return (c["depth"][views], (c["poses"] if poses is None else poses)[views], c["K"])


def born_of_slots(sp):
    """born in slot order, as the device holds it: int64 [slots in use]"""
    return sp["born"][np.asarray(sp["slot_brick"], np.int64)] if sp["slot_brick"] else np.zeros(0, np.int64)


def case(name):
    """name -> dict(the inputs, fused: the volume after one call over all views with its counts, even: the same with the views at
    the even positions removed again and the six numbers of `remove`, none: the same with the rest removed too); computed once"""
    if ("case", name) in _cases:
        return _cases[("case", name)]
    c = inputs(name)
    assert c["max_weight"] == math.inf
    sp, counts = fuse(name)
    assert S.inside_window(sp), name
    n = len(c["depth"])
    even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
    rgb = c["rgb"]
    half = copy_volume(sp)
    got_even = remove(half, c["depth"][even], c["poses"][even], c["K"], counts["ids"][even], None if rgb is None else rgb[even], c["depth_max"])
    none = copy_volume(half)
    got_odd = remove(none, c["depth"][odd], c["poses"][odd], c["K"], counts["ids"][odd], None if rgb is None else rgb[odd], c["depth_max"])
    _cases[("case", name)] = dict(c, fused=sp, counts=counts, even=even, odd=odd, half=half, removed_even=got_even, none=none, removed_odd=got_odd)
    return _cases[("case", name)]


def drifted():
    """The drift route on DRIFT: the odd views fused at RM.drifted_poses, removed there under their ids and fused at the true poses
    under fresh ones -> dict(case, poses_drifted, odd, stale: the volume fused at the drifted poses, corrected: after remove and
    fuse, removed: the six numbers of `remove`, fused: the counts of fusing the odd views again (ids: their new ids), ids: the ids of
    all views afterwards, fresh: the volume fused at the true poses); computed once"""
    if "drift" in _cases:
        return _cases["drift"]
    c = inputs(DRIFT)
    wrong = RM.drifted_poses(c["poses"])
    odd = np.arange(1, len(c["poses"]), 2)
    stale, counts = fuse(DRIFT, wrong)
    corrected = copy_volume(stale)
    removed = remove(corrected, c["depth"][odd], wrong[odd], c["K"], counts["ids"][odd], None, c["depth_max"])
    fused = integrate(corrected, c["depth"][odd], c["poses"][odd], c["K"], None, c["depth_max"])
    ids = counts["ids"].copy()
    ids[odd] = fused["ids"]
    fresh_vol, _ = fuse(DRIFT)
    _cases["drift"] = {"case": c, "poses_drifted": wrong, "odd": odd, "stale": stale, "corrected": corrected, "removed": removed, "fused": fused,
                       "ids": ids, "fresh": fresh_vol}
    return _cases["drift"]
