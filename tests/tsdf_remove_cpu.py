"""Float64 restatement of the removal of fused views (mipsfusion_amd/tsdf.py deintegrate and reintegrate, csrc/tsdf_remove.hip,
include/mipsf_deintegrate.h) in numpy, following the header's rule literally over tsdf_cpu._project: every floating-point operation
below is one IEEE float64 operation, EVERY voxel is tested against EVERY view in ascending view order (no bricks, no culling), and
the running values are rounded to fp32 after every view.  The device's words and its four counts must EQUAL what this file gives.
It is a checker, not the product.  It also holds the cases the tests share -- a case of tsdf_cpu with its odd views drifted, as a
trajectory is before a loop closure corrects it -- each computed once.
"""
import math

import numpy as np

from . import raster_cpu as R
from . import tsdf_cpu as T

# the drift of the odd views: the camera turned in place by 0.03 rad about the world's z axis and moved by (6, -4, 5) cm
DRIFT_ANGLE, DRIFT_SHIFT = 0.03, (0.06, -0.04, 0.05)
DRIFTED_CASES = ("box/33x47/v0.20/t3", "colour", "random_poses", "two_rooms/v0.20")
# |tsdf| and |colour| of remove-and-fuse-again against the fresh fusion: four times the largest difference the restatement shows
# on DRIFTED_CASES (2^-23 and 2^-24, printed by tests/test_tsdf_remove_cpu.py), room for rounding and not a target
TSDF_GATE, COLOR_GATE = 2.0 ** -21, 2.0 ** -22
# what the loop-closure route gives reintegrate as min_translation (m) and min_rotation (rad): far above the rounding of a rebase
# (1e-7), far below the drift
MOVED_TRANSLATION, MOVED_ROTATION = 1e-3, 1e-3
_cases = {}


def remove(state, ticks, depth, poses, K, trunc, depth_max=math.inf, rgb=None):
    """takes the views out of `state` in place -> (removed, missing, emptied, observed)"""
    D = np.asarray(depth, np.float32)
    D = D[None] if D.ndim == 2 else D
    P = R._poses(poses)
    C3 = None if rgb is None else np.asarray(rgb, np.float32).reshape(D.shape + (3,))
    assert (C3 is None) == (state["color"] is None) and len(P) == len(D)
    _, H, W = D.shape
    trunc, depth_max = float(trunc), float(depth_max)
    removed = missing = emptied = 0
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            z, inside, ri, ci = T._project(ticks, pose, K, H, W)
            d = D[k][ri, ci].astype(np.float64)
            usable = (d > 0) & (d < np.inf) & (d <= depth_max)
            sdf = d - z
            hit = inside & usable & (sdf >= -trunc)
            val = sdf / trunc
            val = np.where(val > 1.0, 1.0, val)
            w0 = state["weight"].astype(np.float64)
            have = hit & (w0 > 0)
            w1 = w0 - 1.0
            last = have & ~(w1 > 0)
            rest = have & (w1 > 0)
            new = ((state["tsdf"].astype(np.float64) * w0 - val) / w1).astype(np.float32)
            state["tsdf"] = np.where(rest, new, np.where(last, zero, state["tsdf"]))
            if C3 is not None:
                c = C3[k][ri, ci].astype(np.float64)
                newc = ((state["color"].astype(np.float64) * w0[..., None] - c) / w1[..., None]).astype(np.float32)
                state["color"] = np.where(rest[..., None], newc, np.where(last[..., None], zero, state["color"]))
            state["weight"] = np.where(rest, w1.astype(np.float32), np.where(last, zero, state["weight"]))
            removed += int(have.sum())
            missing += int((hit & ~(w0 > 0)).sum())
            emptied += int(last.sum())
    return removed, missing, emptied, int((state["weight"] > 0).sum())


def copy_state(state):
    return {k: None if v is None else v.copy() for k, v in state.items()}


def drift_rotation(angle=DRIFT_ANGLE):
    """float64 [3,3]: the rotation by `angle` about the world's z axis"""
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def drifted_poses(poses, which=None, angle=DRIFT_ANGLE, shift=DRIFT_SHIFT):
    """fp32 poses tensor [n,4,4] -> the same with the views `which` (the odd ones by default) drifted: the camera turned in place
    by the rotation, then moved by `shift`; float64, rounded to fp32"""
    import torch
    P = poses.detach().cpu().numpy().astype(np.float64)
    which = np.arange(1, len(P), 2) if which is None else np.asarray(which)
    P[which, :3, :3] = drift_rotation(angle) @ P[which, :3, :3]
    P[which, :3, 3] += np.asarray(shift, np.float64)
    return torch.from_numpy(P.astype(np.float32))


def _fuse(c, poses, views=slice(None), state=None):
    state = T.new_state(c["dims"], c["rgb"] is not None) if state is None else state
    counts = T.integrate(state, c["ticks"], c["depth"][views], poses[views], c["K"], c["trunc"], c["depth_max"], rgb=None if c["rgb"] is None else c["rgb"][views])
    return state, counts


def _remove(c, poses, views, state):
    return remove(state, c["ticks"], c["depth"][views], poses[views], c["K"], c["trunc"], c["depth_max"], None if c["rgb"] is None else c["rgb"][views])


def odd_removed(name):
    """tsdf_cpu.case(name) with its odd views removed again -> dict(state, counts: the four of the removal); computed once"""
    key = ("odd", name)
    if key not in _cases:
        c = T.case(name)
        state = copy_state(c["state"])
        odd = slice(1, None, 2)
        _cases[key] = {"counts": _remove(c, c["poses"], odd, state), "state": state}
    return _cases[key]


def drifted(name):
    """tsdf_cpu.case(name), whose poses are the true ones, with the odd views fused at drifted poses -> dict(case, poses_drifted,
    odd, stale: that fusion, removed: the four counts of taking the odd views out at the drifted poses, fused: the two counts of
    fusing them at the true ones, corrected: the state after both; the fresh fusion is case["state"]); computed once"""
    if name in _cases:
        return _cases[name]
    c = T.case(name)
    assert c["max_weight"] == math.inf
    wrong = drifted_poses(c["poses"])
    odd = slice(1, None, 2)
    stale, _ = _fuse(c, wrong)
    corrected = copy_state(stale)
    removed = _remove(c, wrong, odd, corrected)
    _, fused = _fuse(c, c["poses"], odd, corrected)
    _cases[name] = {"case": c, "poses_drifted": wrong, "odd": odd, "stale": stale, "removed": removed, "fused": fused, "corrected": corrected}
    return _cases[name]


def loop_closure():
    """The two rooms as two sub-maps before a loop closure: the views of room B (camera beyond the shared wall) belong to sub-map
    1, whose anchor has drifted by DRIFT_ANGLE and DRIFT_SHIFT, and their world poses with it (the pose relative to the anchor is
    kept, as pose_graph.rebase keeps it) -> dict(case, submap_of_pose int64 [n], anchors_true, anchors_drifted float64 [2,4,4],
    poses_drifted fp32 tensor [n,4,4]: what the volume was fused at); computed once"""
    if "loop" in _cases:
        return _cases["loop"]
    import torch
    from mipsfusion_amd import synth
    c = T.case("two_rooms/v0.20")
    P = c["poses"].numpy().astype(np.float64)
    sub = (P[:, 2, 3] > synth.TWO_ROOMS["room_a"][2][1]).astype(np.int64)
    assert 0 < sub.sum() < len(sub)
    true = np.stack([P[np.nonzero(sub == s)[0][0]] for s in (0, 1)])
    wrong = true.copy()
    wrong[1, :3, :3] = drift_rotation() @ true[1, :3, :3]
    wrong[1, :3, 3] += np.asarray(DRIFT_SHIFT)
    world = (wrong @ np.linalg.inv(true))[sub] @ P
    _cases["loop"] = {"case": c, "submap_of_pose": sub, "anchors_true": true, "anchors_drifted": wrong,
                      "poses_drifted": torch.from_numpy(world.astype(np.float32))}
    return _cases["loop"]
