"""CPU: the float64 restatement of the removal of fused views (tests/tsdf_remove_cpu.py) held to what is known without a GPU --
removing every view gives back the empty volume, removing the drifted half of a fusion and fusing it again at the true poses gives
the fresh fusion up to the rounding of the steps and puts the mesh back on the walls, an empty volume has nothing to remove -- and
the C ABI of mipsf_deintegrate_views.  tests/test_gpu_tsdf_remove.py holds the device to the restatement for equality of words."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import raster_cpu as R
from . import tsdf_cpu as T
from . import tsdf_remove_cpu as RM
from .conftest import ROOT

ALL_CASES = ("box/33x47/v0.20/t3", "colour", "random_poses", "two_rooms/v0.20", "one_voxel", "1x5x70", "bad_pixels", "many_views")


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", ALL_CASES)
def test_removing_every_view_gives_back_the_empty_volume(name):
    c = T.case(name)
    state = RM.copy_state(c["state"])
    removed, missing, emptied, observed = RM.remove(state, c["ticks"], c["depth"], c["poses"], c["K"], c["trunc"], c["depth_max"], c["rgb"])
    print(f"{name}: removed {removed} (updates {c['updates']}), missing {missing}, emptied {emptied} (observed before {c['observed']}), observed {observed}")
    for key in ("tsdf", "weight", "color"):
        if state[key] is not None:
            assert not state[key].view(np.uint32).any(), key          # the words: no -0.0 either
    assert (removed, missing, emptied, observed) == (c["updates"], 0, c["observed"], 0)


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", RM.DRIFTED_CASES)
def test_remove_and_fuse_again_gives_the_fresh_fusion(name):
    """Every second view fused RM.DRIFT_ANGLE rad and RM.DRIFT_SHIFT m away from its pose, then removed there and fused where it
    belongs.  The weights are integers and must equal the fresh fusion's; tsdf and colour differ by the rounding of the steps.
    Measured with this restatement (largest |difference| of tsdf, of colour; of the stale tsdf for scale):
        box/33x47/v0.20/t3   1.19e-07   -          1.36
        colour               5.96e-08   5.96e-08   1.00
        random_poses         1.19e-07   -          1.99
        two_rooms/v0.20      1.19e-07   -          1.86
    The gates are four times the largest of these, 2^-21 and 2^-22: room for rounding, not a target."""
    d = RM.drifted(name)
    c = d["case"]
    fresh, got, stale = c["state"], d["corrected"], d["stale"]
    n_odd = len(c["poses"][d["odd"]])
    diff = float(np.abs(got["tsdf"].astype(np.float64) - fresh["tsdf"]).max())
    diff_stale = float(np.abs(stale["tsdf"].astype(np.float64) - fresh["tsdf"]).max())
    diff_c = float(np.abs(got["color"].astype(np.float64) - fresh["color"]).max()) if c["rgb"] is not None else 0.0
    print(f"{name}: {n_odd} of {len(c['poses'])} views moved, removed {d['removed']}, fused {d['fused']}; largest difference to the fresh fusion: "
          f"tsdf {diff:.3g} (stale {diff_stale:.3g}), colour {diff_c:.3g}")
    assert np.array_equal(got["weight"], fresh["weight"])
    assert not np.array_equal(stale["weight"], fresh["weight"]) and diff_stale >= 1.0
    assert diff <= RM.TSDF_GATE and diff_c <= RM.COLOR_GATE
    assert d["removed"][1] == 0 and d["removed"][3] <= c["observed"] and d["fused"][1] == c["observed"]


# ------------------------------------------------------------------------------------------------------------ (c)
def test_the_corrected_box_room_lies_on_its_walls_again():
    """Wall distance of the marched vertices in voxels, measured with this restatement (vertices, faces, mean, max):
        stale       1701   3047   0.203   0.944
        corrected   1707   3110   0.060   0.500
        fresh       1707   3110   0.060   0.500"""
    d = RM.drifted("box/33x47/v0.20/t3")
    c = d["case"]
    _, _, lo, hi = R.box_room()
    got = {}
    for key, state in (("stale", d["stale"]), ("corrected", d["corrected"]), ("fresh", c["state"])):
        v, f, _ = T.extract_mesh(state, c["origin"], c["voxel"])
        w = T.wall_distance(v[np.unique(f)], lo, hi) / c["voxel"]
        got[key] = (len(v), len(f), float(w.mean()), float(w.max()))
        print(f"{key}: {len(v)} vertices, {len(f)} faces, wall distance in voxels: mean {w.mean():.3f}, max {w.max():.3f}")
    assert got["stale"][2] > T.MEAN_GATE
    assert got["corrected"][2] <= T.MEAN_GATE and got["corrected"][3] <= T.MAX_GATE
    assert got["corrected"][:2] == got["fresh"][:2]


def test_the_stale_two_rooms_score_worse_than_the_corrected_ones():
    """The loop-closure route of tests/test_gpu_tsdf_remove.py on the restatement, so that what the GPU test asserts of the stale
    volume rests on a measured number: accuracy (mean distance of 20 000 surface samples to synth.two_rooms_mesh(), metres) of the
    volume fused at the drifted poses 0.0781, corrected 0.0696, fused afresh 0.0696; the drift is RM.DRIFT_ANGLE, RM.DRIFT_SHIFT."""
    from mipsfusion_amd import pose_graph, synth

    from . import eval_cpu as E
    import torch
    loop = RM.loop_closure()
    c, sub = loop["case"], loop["submap_of_pose"]
    new = pose_graph.rebase(loop["poses_drifted"], sub, loop["anchors_drifted"], loop["anchors_true"]).to(torch.float32)
    # the rebased poses of sub-map 0 differ from the old ones by the rounding of X_new X_old^-1 at most: the thresholds of
    # reintegrate leave them where they are, and the volume then holds them at their old poses
    from mipsfusion_amd import tsdf
    moved = np.nonzero(tsdf._moved(loop["poses_drifted"].numpy(), new.numpy(), RM.MOVED_TRANSLATION, RM.MOVED_ROTATION))[0]
    assert np.array_equal(moved, np.nonzero(sub == 1)[0])
    assert float((new - loop["poses_drifted"])[sub == 0].abs().max()) < 1e-6
    held = loop["poses_drifted"].clone()
    held[moved] = new[moved]
    stale, _ = RM._fuse(c, loop["poses_drifted"])
    fresh, _ = RM._fuse(c, held)
    got = RM.copy_state(stale)
    removed = RM._remove(c, loop["poses_drifted"], moved, got)
    RM._fuse(c, new, moved, got)
    assert removed[1] == 0 and np.array_equal(got["weight"], fresh["weight"])
    assert float(np.abs(got["tsdf"].astype(np.float64) - fresh["tsdf"]).max()) <= RM.TSDF_GATE
    acc = {}
    for key, state in (("stale", stale), ("corrected", got), ("fresh", fresh)):
        v, f, _ = T.extract_mesh(state, c["origin"], c["voxel"])
        acc[key] = (len(v), len(f), E.reconstruction_metrics((v, f), synth.two_rooms_mesh(), 20000)["accuracy"])
        print(f"{key}: {len(v)} vertices, {len(f)} faces, accuracy {acc[key][2]:.4f} m")
    assert acc["corrected"][:2] == acc["fresh"][:2] and abs(acc["corrected"][2] - acc["fresh"][2]) <= 0.01 * acc["fresh"][2]
    assert acc["stale"][2] > max(acc["corrected"][2], acc["fresh"][2])


def test_which_views_moved():
    import torch
    from mipsfusion_amd import tsdf
    P = T.box_poses20().numpy()
    assert not tsdf._moved(P, P.copy(), 0.0, 0.0).any()
    Q = P.copy()
    Q[3, 1, 2] = np.nextafter(Q[3, 1, 2], np.float32(2.0))            # one word, one bit
    Q[7, 0, 3] += 0.01
    Q[9] = RM.drifted_poses(torch.from_numpy(P), [9], angle=0.01, shift=(0.0, 0.0, 0.0)).numpy()[9]
    assert np.nonzero(tsdf._moved(P, Q, 0.0, 0.0))[0].tolist() == [3, 7, 9]
    assert np.nonzero(tsdf._moved(P, Q, 0.001, 0.001))[0].tolist() == [7, 9]
    assert np.nonzero(tsdf._moved(P, Q, 0.02, 0.001))[0].tolist() == [9] and np.nonzero(tsdf._moved(P, Q, 0.001, 0.02))[0].tolist() == [7]
    assert not tsdf._moved(P, Q, 1.0, 1.0).any()
    Q[5] = np.nan                                                     # a lost frame that one side has a pose for: moved, either way
    assert tsdf._moved(P, Q, 0.0, 0.0)[5] and tsdf._moved(P, Q, 0.001, 0.001)[5] and tsdf._moved(Q, P, 1.0, 1.0)[5]
    assert not tsdf._moved(Q, Q.copy(), 0.0, 0.0)[5] and not tsdf._moved(Q, Q.copy(), 0.001, 0.001)[5]      # lost before and after
    with pytest.raises(ValueError, match="negative"):
        tsdf._moved(P, Q, -1.0, 0.0)


THRESHOLDS = [(1e-2, 0.0), (0.0, 1e-6), (1e-6, 1e-6), (1e-7, 1e-7), (1e-2, 1e-6), (1e-6, 1e-2)]


@pytest.mark.parametrize("min_translation,min_rotation", THRESHOLDS)
def test_poses_that_did_not_move_are_not_moved(min_translation, min_rotation):
    """The angle between two rotations must be 0 for equal words and of the size of the difference for a rounding: the arc cosine
    of the trace of R_old^T R_new is neither (the trace of an fp32 rotation with itself is 1e-7 off 3, which the arc cosine turns
    into up to 4e-4 rad), and half of 10 000 unmoved views then counted as moved at any threshold below that."""
    import torch
    from mipsfusion_amd import pose_graph, tsdf
    g = np.random.default_rng(17)
    q = g.normal(size=(10000, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    P = np.zeros((len(q), 4, 4))
    P[:, :3, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                             2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    P[:, :3, 3] = g.uniform(-5.0, 5.0, (len(q), 3))
    P[:, 3, 3] = 1.0
    P = P.astype(np.float32)
    assert not tsdf._moved(P, P.copy(), min_translation, min_rotation).any()
    # one rebase by an anchor that stayed: X X^-1 W, the identity up to rounding.  A threshold of 0 means any change, so the
    # rounded poses are held to the thresholds that are above a rounding on both sides
    anchor = P[:1].astype(np.float64)
    again = pose_graph.rebase(torch.from_numpy(P), np.zeros(len(P), np.int64), anchor, anchor.copy()).to(torch.float32).numpy()
    off = np.abs(again.astype(np.float64) - P).max()
    assert 0 < off < 2e-6
    if min_translation >= 1e-6 and min_rotation >= 1e-6:
        assert not tsdf._moved(P, again, min_translation, min_rotation).any()
    # and what did move is still seen: 1e-5 rad and 1e-5 m are moved at 1e-6, each on its own
    Q = RM.drifted_poses(torch.from_numpy(P), [0], angle=1e-5, shift=(0.0, 0.0, 0.0)).numpy()
    Q[1, 0, 3] += np.float32(1e-4)
    assert tsdf._moved(P, Q, 1e-6, 1e-6)[:3].tolist() == [True, True, False]
    assert tsdf._moved(P, Q, 1.0, 1e-6)[:3].tolist() == [True, False, False] and tsdf._moved(P, Q, 1e-6, 1.0)[:3].tolist() == [False, True, False]


# ------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", ["box/33x47/v0.20/t3", "colour", "bad_pixels"])
def test_an_empty_volume_has_nothing_to_remove(name):
    c = T.case(name)
    state = T.new_state(c["dims"], c["rgb"] is not None)
    removed, missing, emptied, observed = RM.remove(state, c["ticks"], c["depth"], c["poses"], c["K"], c["trunc"], c["depth_max"], c["rgb"])
    assert (removed, missing, emptied, observed) == (0, c["updates"], 0, 0) and missing > 0
    assert not any(v.view(np.uint32).any() for v in state.values() if v is not None)
    # a weight that is not a number holds nothing either: its voxel's hits are missing and its words stay
    state = RM.copy_state(c["state"])
    at = tuple(np.argwhere(c["updated"].sum(0) > 1)[0])
    state["weight"][at] = np.nan
    before = RM.copy_state(state)
    counts = RM.remove(state, c["ticks"], c["depth"][:2], c["poses"][:2], c["K"], c["trunc"], c["depth_max"], None if c["rgb"] is None else c["rgb"][:2])
    assert counts[1] == int(c["updated"][:2][(slice(None),) + at].sum())
    assert state["tsdf"][at].tobytes() == before["tsdf"][at].tobytes() and np.isnan(state["weight"][at])


# ------------------------------------------------------------------------------------------------------------ (e) the C ABI
def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_deintegrate.h")).read()
    declared = set(re.findall(r"\b(mipsf_deintegrate_[a-z0-9_]+)\s*\(", header))
    assert declared == {"mipsf_deintegrate_views"} == set(_lib.DEINTEGRATE_SIGNATURES)
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    # 8 words, 6 doubles, 10 pointers: the block of mipsf_tsdf_integrate less max_weight; a record of four uint64
    assert C.sizeof(_lib.DeintegrateArgs) == 32 + 48 + 80 == C.sizeof(_lib.TsdfIntegrateArgs) - 8
    assert [f[0] for f in _lib.DeintegrateArgs._fields_] == [f[0] for f in _lib.TsdfIntegrateArgs._fields_ if f[0] != "max_weight"]
    assert _lib.DEINTEGRATE_RECORD_WORDS == 4 and re.search(r"uint64_t removed;.*\n\s*uint64_t missing;.*\n\s*uint64_t emptied;.*\n\s*uint64_t observed;", header)
    import mipsfusion_amd
    from mipsfusion_amd import tsdf
    for name in ("RemoveCounts", "ReintegrateCounts"):
        assert getattr(mipsfusion_amd, name) is getattr(tsdf, name)
    assert tsdf.RemoveCounts._fields == ("removed", "missing", "emptied", "observed")
    assert tsdf.ReintegrateCounts._fields == ("views_moved", "removed", "fused")


def _good(**kw):
    fake = 0x1000                               # never used: every call below is refused before a pointer is
    a = dict(X=4, Y=5, Z=6, n=2, H=8, W=9, fx=10.0, fy=10.0, cx=4.0, cy=4.0, trunc=0.3, depth_max=math.inf,
             depth=fake, poses=fake, tsdf=fake, weight=fake, record=fake)
    a.update(kw)
    blk = _lib.DeintegrateArgs.new(**a)
    for d in range(3):
        blk.ticks[d] = fake
    return blk


# those of tests/test_tsdf_cpu.py, less the two of max_weight
REFUSALS = [(dict(X=0), "no voxels"), (dict(Y=0), "no voxels"), (dict(Z=0), "no voxels"), (dict(H=0), "no pixels"), (dict(W=0), "no pixels"),
            (dict(X=2048, Y=1024, Z=1024), "at most 2"), (dict(X=1 << 31, Y=1, Z=1), "at most 2"), (dict(X=1 << 28, Y=1, Z=1), "bricks"), (dict(H=8193), "a side"),
            (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=math.inf), "trunc"), (dict(trunc=math.nan), "trunc"),
            (dict(fx=0.0), "intrinsics"), (dict(fy=-3.0), "intrinsics"), (dict(fx=math.inf), "intrinsics"), (dict(fy=math.nan), "intrinsics"),
            (dict(cx=math.inf), "intrinsics"), (dict(cy=math.nan), "intrinsics"), (dict(depth_max=math.nan), "depth_max"), (dict(flags=2), "flags"),
            (dict(rgb=0x1000), "go together"), (dict(color=0x1000), "go together"),
            (dict(depth=None), "null pointer"), (dict(poses=None), "null pointer"), (dict(tsdf=None), "null pointer"),
            (dict(weight=None), "null pointer"), (dict(record=None), "null pointer")]


@pytest.mark.parametrize("change,said", REFUSALS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in REFUSALS])
def test_what_is_out_of_range_is_refused_on_the_host(change, said):
    lib = _lib.lib()
    assert lib.mipsf_deintegrate_views(C.byref(_good(**change)), None) != 0
    message = lib.mipsf_last_error()
    assert said.encode() in message and b"mipsf_deintegrate_views" in message, message


def test_struct_size_null_ticks_and_a_capped_volume_are_refused_too():
    lib = _lib.lib()
    blk = _lib.DeintegrateArgs.new()
    blk.struct_size -= 4
    assert lib.mipsf_deintegrate_views(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
    assert lib.mipsf_deintegrate_views(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
    blk = _good()
    blk.ticks[1] = None
    assert lib.mipsf_deintegrate_views(C.byref(blk), None) != 0 and b"null pointer" in lib.mipsf_last_error()
    # a volume made with a finite max_weight holds a moving average: every route refuses it before it looks at an argument (the
    # object is made without its device state here, which none of them reaches; tests/test_gpu_tsdf_remove.py asks a real one)
    from mipsfusion_amd import tsdf
    vol = object.__new__(tsdf.TSDFVolume)
    vol.max_weight = 2.0
    for call in (lambda: vol.deintegrate(None, None, None), lambda: vol.deintegrate_enqueue(None, None, None),
                 lambda: vol.reintegrate(None, None, None, None), lambda: vol.reintegrate_enqueue(None, None, None, None)):
        with pytest.raises(ValueError, match="max_weight"):
            call()
