"""CPU: the float64 restatement of the TSDF tracker's model side (tests/track_cpu.py) held to what is known without a GPU -- the
closed-form depth of the box room, scipy's trilinear interpolation, the capture of a perturbed pose, the cases that must take a
given path -- and the C ABI of the new entry points.  tests/test_gpu_track.py holds the device to the restatement for equality of
words.  Every gate below is twice what this file measured, with the measurement next to it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import raster_cpu as R
from . import track_cpu as TC
from . import tsdf_cpu as T
from .conftest import ROOT


# ------------------------------------------------------------------------------------------------------------ ray cast
def test_the_ray_cast_of_the_fused_box_room_lies_on_the_closed_form():
    """|depth - box_exit_depth| over the hits, in voxels, on box/40x56/v0.15/t4 at step = trunc/2.  Measured with this restatement
    (view: hit rate, share of hits with a normal, mean, max):
        0    0.912  0.929  0.029  0.250
        7    0.994  0.993  0.039  0.674      (the largest at the room's edges)
        13   1.000  1.000  0.029  0.100
    A half-voxel error in the placement of the voxels would move the mean to 0.5."""
    c = TC.case("box/40x56/v0.15/t4")
    _, _, lo, hi = R.box_room()
    for k, view in enumerate(TC.BOX_VIEWS):
        exact = R.box_exit_depth(lo, hi, c["poses"][k].numpy(), c["K"], c["H"], c["W"])
        d = c["want"]["depth"][k]
        hit = d != 0
        normal = (c["want"]["normals"][k] != 0).any(-1)
        err = np.abs(d[hit] - exact[hit]) / c["voxel"]
        print(f"view {view}: hit rate {hit.mean():.3f}, normals {normal.sum() / hit.sum():.3f}, mean {err.mean():.4f}, max {err.max():.4f} voxels")
        assert hit.mean() >= 0.9 and normal.sum() >= 0.9 * hit.sum() and not (normal & ~hit).any()
        assert err.mean() <= TC.DEPTH_MEAN_GATE and err.max() <= TC.DEPTH_MAX_GATE
        # unit normals that point into the room: along the ray they face the camera
        n = c["want"]["normals"][k][normal].astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
        dw = np.stack(R.pixel_rays(c["poses"][k].numpy().astype(np.float64), c["K"], c["H"], c["W"]), -1).reshape(c["H"], c["W"], 3)[normal]
        assert ((n * dw).sum(1) < 0).mean() > 0.99


def test_the_trilinear_field_is_scipys():
    """order-1 map_coordinates on interior points: the same interpolant, summed in another order.  Measured: 3.3e-16 absolute on
    values in -1 .. 1 (an ulp and a half of 1); the gate is twice that."""
    from scipy import ndimage
    c = T.case("box/33x47/v0.20/t3")
    g = np.random.default_rng(5)
    dims = np.asarray(c["dims"])
    idx = g.uniform(0.0, 1.0, (4000, 3)) * (dims - 1.001)
    state = {"tsdf": c["state"]["tsdf"], "weight": np.ones_like(c["state"]["weight"])}
    known, f = TC.field(state, np.zeros(3), 1.0, [idx[:, 0], idx[:, 1], idx[:, 2]])
    want = ndimage.map_coordinates(c["state"]["tsdf"].astype(np.float64), idx.T, order=1)
    print(f"trilinear against scipy: max |difference| {np.abs(f - want).max():.3e}")
    assert known.all() and np.abs(f - want).max() <= 6.7e-16
    # unknown: outside, on the last lattice plane, below min_weight
    known, _ = TC.field(state, np.zeros(3), 1.0, [np.array([-0.5, dims[0] - 1.0, 1.5]), np.array([1.0, 1.0, 1.5]), np.array([1.0, 1.0, 1.5])])
    assert known.tolist() == [False, False, True]
    assert not TC.field(c["state"], np.zeros(3), 1.0, [np.array([0.5]), np.array([0.5]), np.array([0.5])])[0].any()      # the padding no view saw


def test_the_cases_take_the_paths_they_are_there_for():
    box = TC.case("box/33x47/v0.20/t3")
    assert TC.case("unobserved")["want"]["hits"] == 0 and TC.case("unobserved")["want"]["samples"] > 1000
    assert TC.case("side_1")["want"]["hits"] == 0 and TC.case("one_voxel")["want"]["hits"] == 0 and TC.case("one_voxel")["want"]["samples"] == 0
    assert TC.case("side_2")["dims"][0] == 2 and TC.case("side_2")["want"]["samples"] > 1000
    assert TC.case("no_views")["want"]["depth"].shape == (0, 5, 7)
    assert TC.case("image_1x1")["want"]["hits"] == 3 and TC.case("image_17x33")["want"]["hits"] > 1000
    # from outside the cropped volume: hits, and every ray starts at the face (t_in > near = 0)
    assert TC.case("enter_through_a_face")["want"]["hits"] > 1000
    # behind the wall: the first crossing is from negative to positive, and the walk stops there; without that stop the rays go on
    # to the far wall of the room
    c = TC.case("behind_a_wall")
    free = TC.raycast(c["state"], c["origin"], c["voxel"], c["poses"], c["K"], c["H"], c["W"], c["step"], back_face=False)
    stopped, went_on = (c["want"]["depth"] != 0).sum((1, 2)), (free["depth"] != 0).sum((1, 2))
    print("behind a wall: hits per view", stopped.tolist(), "without the back-face stop", went_on.tolist())
    assert (went_on - stopped > 300).all() and c["want"]["samples"] < free["samples"]
    # fewer voxels are known at min_weight 2, more samples at a finer step; near and far cut the walls off
    assert TC.case("min_weight_2")["want"]["hits"] < box["want"]["hits"]
    assert TC.case("step_trunc")["want"]["samples"] < box["want"]["samples"] < TC.case("step_trunc/4")["want"]["samples"]
    cut = TC.case("near_far")
    d = cut["want"]["depth"]
    assert 0 < cut["want"]["hits"] < box["want"]["hits"] and d[d != 0].min() >= cut["near"] and d[d != 0].max() <= cut["far"] + cut["step"]
    # colour follows the walls' analytic colour as the marched vertices do
    col = TC.case("colour")
    hit = col["want"]["depth"] != 0
    assert col["want"]["color"][hit].min() >= 0.0 and col["want"]["color"][hit].max() <= 1.0 and col["want"]["color"][hit].std() > 0.05
    assert not col["want"]["color"][~hit].any()


def test_the_planted_plane():
    """the principal ray of view 0 runs down a lattice line: d.x = d.y = 0, its samples are lattice points, the tsdf words there are
    k/4 - 1 exactly, and the walk ends on f == 0 with t* = that sample's own t"""
    c = TC.case("plane")
    state, origin, voxel, dims = TC.plane_volume()
    row, col = 4, 5                                              # cy, cx of the case
    top = origin[2] + voxel * (dims[2] - 1)
    want_depth = (top + 0.5) - (origin[2] + voxel * 4)
    assert c["want"]["depth"][0, row, col] == np.float32(want_depth)
    known, f = TC.field(state, origin, voxel, [np.array([origin[0] + 5 * voxel]), np.array([origin[1] + 7 * voxel]), np.array([origin[2] + 4 * voxel])])
    assert known[0] and f[0] == 0.0
    assert c["want"]["normals"][0, row, col].tolist() == [0.0, 0.0, 1.0]
    assert c["want"]["depth"][1, row, col] == 0                  # beside the volume with d.x == 0: a miss
    assert (c["want"]["depth"][2] != 0).sum() > 0
    marks = TC.brick_marks(state)
    assert marks.shape == (3, 3, 5) and marks.sum() == 9 and marks[:, :, 0].all()      # 80 % of the bricks are free space


# ------------------------------------------------------------------------------------------------------------ registration
@pytest.mark.parametrize("name", sorted(TC.REG_OFFSETS))
def test_a_perturbed_pose_is_captured(name):
    """The exact depth of a perturbed camera against the model cast from view 7 of box/40x56/v0.15/t4, 15 iterations, no pyramid.
    Measured with this restatement (start -> end; pairs of 2240 pixels):
        0.64 deg  2.3 cm  ->  0.081 deg  0.47 cm   2198      (stops after 5)
        1.9  deg  5.8 cm  ->  0.051 deg  0.66 cm   2049
        3.8  deg 11.7 cm  ->  0.204 deg  0.56 cm   2073
    This is the capture range the tests vouch for, and nothing more."""
    c, w = TC.reg_case(name), TC.reg_want(name, max_iteration=15)
    deg0, m0 = TC.pose_error(c["pose_init"], c["truth"])
    deg1, m1 = TC.pose_error(w["transformation"], c["truth"])
    print(f"{name}: {deg0:.2f} deg {100 * m0:.1f} cm -> {deg1:.3f} deg {100 * m1:.2f} cm, {w['n']} pairs, {w['iterations']} iterations, "
          f"fitness {w['fitness']:.3f}, rmse {w['rmse']:.4f}, ambiguous {sum(w['ambiguous_per_eval'])}")
    assert abs(deg0 - TC.REG_OFFSETS[name][0]) < 0.01 and abs(100 * m0 - TC.REG_OFFSETS[name][1]) < 0.01
    assert m1 <= 2 * 0.0066 and deg1 <= 2 * 0.204 and w["n"] >= 2000


@pytest.mark.parametrize("name", TC.REG_CASES)
def test_the_committed_cases_have_no_ambiguous_pixel(name):
    """tests/test_gpu_track.py compares pair sets and counts for equality; a pixel within rounding of a decision would make that a
    matter of luck.  A case that trips this gets its pose moved by a millimetre."""
    for kw in ({}, {"max_iteration": 0}):
        w = TC.reg_want(name, **kw)
        assert sum(w["ambiguous_per_eval"]) == 0, (name, w["ambiguous_per_eval"])
    w, c = TC.reg_want(name), TC.reg_case(name)
    usable = (c["live"] > 0) & np.isfinite(c["live"]) & (c["live"] <= c["depth_max"])
    if name == "bad_pixels":
        assert not usable[:c["H"] // 2, :c["W"] // 2].any() and 0.7 < usable.mean() < 0.8
    if name == "depth_max":
        assert 0.45 < usable.mean() < 0.55
    if name == "max_dist":
        assert w["pairs_per_eval"][0] < 0.7 * TC.reg_want("1.9deg_5.8cm")["pairs_per_eval"][0]
    if name == "no_model":
        assert w["n"] == 0 and w["fitness"] == 0.0 and w["iterations"] == 1 and np.array_equal(w["pose"], c["pose_init"])
    assert (w["partner"] >= 0).sum() == w["n"] and not (w["partner"].reshape(c["H"], c["W"])[~usable] >= 0).any()


def test_the_odometry_arc():
    """8 frames, 1 degree and 1.6 cm a frame, voxels of 10 cm, a model that starts from ONE fused frame.  Measured: pose errors of
    0.07 .. 0.23 deg and 0.3 .. 0.6 cm, aligned ATE 1.6 mm, 1195 .. 1312 pairs of 1551 pixels, no ambiguous pixel.  A frame
    without depth is flagged, keeps the pose of the frame before and leaves the volume alone."""
    from mipsfusion_amd.trajectory import trajectory_metrics
    o = TC.odo_case()
    poses, records, state = TC.odometry(o["depth"], o["K"], o["truth"][0], o["origin"], o["voxel"], o["dims"], o["trunc"])
    err = [TC.pose_error(poses[k], o["truth"][k]) for k in range(1, TC.ODO_FRAMES)]
    ate = trajectory_metrics(poses, o["truth"]).rmse
    print("odometry: degrees", [round(e[0], 3) for e in err], "cm", [round(100 * e[1], 2) for e in err], f"ATE {1000 * ate:.2f} mm, pairs",
          [r["n"] for r in records[1:]])
    assert sum(sum(r["ambiguous_per_eval"]) for r in records[1:]) == 0
    assert max(e[1] for e in err) <= 2 * 0.006 and max(e[0] for e in err) <= 2 * 0.23 and ate <= 2 * 0.0016
    depth = o["depth"].copy()
    depth[3] = 0
    poses2, records2, _ = TC.odometry(depth, o["K"], o["truth"][0], o["origin"], o["voxel"], o["dims"], o["trunc"], min_correspondences=100)
    assert [r["lost"] for r in records2[1:]] == [k == 3 for k in range(1, TC.ODO_FRAMES)]
    assert np.array_equal(poses2[3], poses2[2]) and np.array_equal(poses2[:3], poses[:3])


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_track.h")).read()
    declared = set(re.findall(r"\b(mipsf_track_[a-z0-9_]+)\s*\(", header))
    assert declared == {"mipsf_track_workspace_bytes", "mipsf_track_raycast", "mipsf_track_register"} == set(_lib.TRACK_SIGNATURES)
    assert not re.findall(r"\bmipsf_tsdf_[a-z0-9_]+\s*\(", header)      # tests/test_tsdf_cpu.py pins that prefix to mipsf_tsdf.h
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_TRACK_MAX_SAMPLES", _lib.TRACK_MAX_SAMPLES), ("MIPSF_TRACK_TILE", _lib.TRACK_TILE),
                         ("MIPSF_TRACK_RESULT_DOUBLES", _lib.TRACK_RESULT_DOUBLES), ("MIPSF_TRACK_MAX_ITERATION", _lib.TRACK_MAX_ITERATION),
                         ("MIPSF_TRACK_MAX_VIEWS", _lib.TRACK_MAX_VIEWS), ("MIPSF_TRACK_NO_SKIP", _lib.TRACK_NO_SKIP)):
        assert int(re.search(rf"#define {macro} +(0x[0-9a-f]+|\d+)u", header).group(1), 0) == value, macro
    for macro, value in (("MIPSF_TRACK_WS_RAYCAST", _lib.TRACK_WS_RAYCAST), ("MIPSF_TRACK_WS_REGISTER", _lib.TRACK_WS_REGISTER)):
        assert int(re.search(rf"#define {macro} +(\d+)", header).group(1)) == value, macro
    assert (TC.MAX_SAMPLES, TC.BRICK, _lib.TRACK_RESULT_DOUBLES) == (_lib.TRACK_MAX_SAMPLES, _lib.TSDF_BRICK, _lib.ICP_RESULT_DOUBLES)
    # 8 words, 13 doubles, 9 pointers; 4 words, 8 doubles, 9 pointers: what the header's structs come to on this ABI
    assert C.sizeof(_lib.TrackRaycastArgs) == 32 + 104 + 72 and C.sizeof(_lib.TrackRegisterArgs) == 16 + 64 + 72
    lib = _lib.lib()
    ws = lib.mipsf_track_workspace_bytes
    assert ws(_lib.TRACK_WS_RAYCAST, 27, 47, 31) == 48 and ws(_lib.TRACK_WS_RAYCAST, 1, 1, 1) == 16 and ws(_lib.TRACK_WS_RAYCAST, 0, 4, 4) == 0
    assert ws(_lib.TRACK_WS_RAYCAST, 2048, 1024, 1024) == 0 and ws(9, 4, 4, 4) == 0
    assert ws(_lib.TRACK_WS_REGISTER, 40, 56, 0) == 256 + 9 * 32 * 8 and ws(_lib.TRACK_WS_REGISTER, 0, 5, 0) == 0 and ws(_lib.TRACK_WS_REGISTER, 8193, 5, 0) == 0
    import mipsfusion_amd
    from mipsfusion_amd import tsdf
    for name in ("Raycast", "TrackResult", "tsdf_odometry"):
        assert getattr(mipsfusion_amd, name) is getattr(tsdf, name)
    assert "trajectory_metrics" in tsdf.tsdf_odometry.__doc__


FAKE = 0x1000                                   # never used: every call below is refused before a pointer is


def _raycast_block(**kw):
    a = dict(X=4, Y=5, Z=6, n=2, H=8, W=9, voxel=0.1, trunc=0.3, fx=10.0, fy=10.0, cx=4.0, cy=4.0, near=0.0, far=math.inf, step=0.15, min_weight=1.0,
             tsdf=FAKE, weight=FAKE, poses=FAKE, depth=FAKE, record=FAKE, workspace=FAKE)
    origin = kw.pop("origin", (0.0, 0.0, 0.0))
    a.update(kw)
    blk = _lib.TrackRaycastArgs.new(**a)
    for d in range(3):
        blk.origin[d] = origin[d]
    return blk


def _register_block(**kw):
    a = dict(H=8, W=9, max_iteration=3, fx=10.0, fy=10.0, cx=4.0, cy=4.0, depth_max=math.inf, max_dist=0.3, relative_fitness=1e-6, relative_rmse=1e-6,
             model_depth=FAKE, model_normals=FAKE, pose_ref=FAKE, live=FAKE, pose_init=FAKE, result=FAKE, pose_out=FAKE, workspace=FAKE)
    a.update(kw)
    return _lib.TrackRegisterArgs.new(**a)


RAYCAST_REFUSALS = [(dict(X=0), "no voxels"), (dict(Z=0), "no voxels"), (dict(X=2048, Y=1024, Z=1024), "at most 2"), (dict(X=1 << 28, Y=1, Z=1), "bricks"),
                    (dict(H=0), "no pixels"), (dict(W=0), "no pixels"), (dict(W=8193), "a side"), (dict(n=65536), "views"),
                    (dict(voxel=0.0), "voxel"), (dict(voxel=math.nan), "voxel"), (dict(trunc=-1.0), "trunc"), (dict(trunc=math.inf), "trunc"),
                    (dict(step=0.0), "step"), (dict(step=math.nan), "step"), (dict(step=1e-9), "samples a ray"),
                    (dict(fx=0.0), "intrinsics"), (dict(fy=math.inf), "intrinsics"), (dict(cx=math.nan), "intrinsics"), (dict(cy=math.inf), "intrinsics"),
                    (dict(origin=(0.0, math.nan, 0.0)), "origin"), (dict(origin=(math.inf, 0.0, 0.0)), "origin"),
                    (dict(near=math.nan), "near or far"), (dict(far=math.nan), "near or far"), (dict(min_weight=math.nan), "min_weight"),
                    (dict(flags=2), "flags"), (dict(color_out=FAKE), "color_out"),
                    (dict(tsdf=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(poses=None), "null pointer"),
                    (dict(depth=None), "null pointer"), (dict(record=None), "null pointer"), (dict(workspace=None), "null pointer"),
                    (dict(workspace=FAKE + 8), "16-byte")]
REGISTER_REFUSALS = [(dict(H=0), "no pixels"), (dict(W=0), "no pixels"), (dict(H=8193), "a side"), (dict(fx=-1.0), "intrinsics"), (dict(cy=math.nan), "intrinsics"),
                     (dict(depth_max=math.nan), "depth_max"), (dict(max_dist=-0.1), "max_dist"), (dict(max_dist=math.inf), "max_dist"),
                     (dict(max_dist=math.nan), "max_dist"), (dict(max_iteration=1001), "max_iteration"),
                     (dict(model_depth=None), "null pointer"), (dict(model_normals=None), "null pointer"), (dict(pose_ref=None), "null pointer"),
                     (dict(live=None), "null pointer"), (dict(pose_init=None), "null pointer"), (dict(result=None), "null pointer"),
                     (dict(pose_out=None), "null pointer"), (dict(workspace=None), "null pointer"), (dict(workspace=FAKE + 4), "16-byte")]


def _ids(refusals):
    return [f"{list(c)[0]}={list(c.values())[0]}" for c, _ in refusals]


@pytest.mark.parametrize("change,said", RAYCAST_REFUSALS, ids=_ids(RAYCAST_REFUSALS))
def test_the_ray_cast_refuses_what_is_out_of_range(change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_raycast(C.byref(_raycast_block(**change)), None) != 0
    assert b"mipsf_track_raycast" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


@pytest.mark.parametrize("change,said", REGISTER_REFUSALS, ids=_ids(REGISTER_REFUSALS))
def test_the_registration_refuses_what_is_out_of_range(change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_register(C.byref(_register_block(**change)), None) != 0
    assert b"mipsf_track_register" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_struct_sizes_are_checked():
    lib = _lib.lib()
    for cls, fn in ((_lib.TrackRaycastArgs, lib.mipsf_track_raycast), (_lib.TrackRegisterArgs, lib.mipsf_track_register)):
        blk = cls.new()
        blk.struct_size -= 4
        assert fn(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
        assert fn(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
