"""CPU: the float64 restatement of the tracker's colour registration (tests/track_color_cpu.py) held to what is known without a GPU
-- with no weight it IS the depth-only loop, the colour moves the pose where depth cannot, it does no harm where depth can, no
pixel of a committed case lies within rounding of a decision -- and the C ABI of the new entry point.
tests/test_gpu_track_color.py holds the device to the restatement.  The figures in the docstrings were measured with this file."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import track_color_cpu as CC
from . import track_cpu as TC
from .conftest import ROOT

DEFAULT_WEIGHT = 10.0                 # mipsfusion_amd.tsdf.DEFAULT_COLOR_WEIGHT (that module needs torch; the GPU test compares the two)
QUARTER = 0.25                        # a sliding case must end below this share of its start
CORNER_MARGIN = 0.010                 # metres; twice the 0.50 cm the colour costs on `corner` at the default weight (below)


def _metres(T, c):
    return TC.pose_error(T, c["truth"])[1]


# ------------------------------------------------------------------------------------------------------------ 1. zero weight
@pytest.mark.parametrize("name", TC.REG_CASES)
def test_zero_weight_reproduces_the_depth_only_loop(name):
    c, want = TC.reg_case(name), TC.reg_want(name)
    mc, lc = CC.reg_colors(name)
    got = CC.register_color(c["model_depth"], c["model_normals"], mc, c["pose_ref"], c["live"], lc, c["pose_init"], c["K"], c["depth_max"], c["max_dist"],
                            color_weight=0.0, relative_color_rmse=math.inf)
    assert np.array_equal(got["transformation"], want["transformation"]) and np.array_equal(got["partner"], want["partner"])
    assert (got["n"], got["iterations"], got["fitness"], got["rmse"]) == (want["n"], want["iterations"], want["fitness"], want["rmse"])
    assert got["pairs_per_eval"] == want["pairs_per_eval"]
    assert all(r <= p for r, p in zip(got["rows_per_eval"], got["pairs_per_eval"]))
    if name == "no_model":
        assert got["rows_per_eval"] == [0, 0] and got["color_rmse"] == 0.0
    else:
        assert got["n_color"] > 0.9 * got["n"]


def test_cases_without_a_patch_give_no_photometric_row():
    for name in ("image_1x1", "no_model"):
        w = CC.want(name, color_weight=DEFAULT_WEIGHT)
        assert w["rows_per_eval"] == [0, 0] and w["color_rmse"] == 0.0 and w["iterations"] == 1 and not w["color_row"].any(), name
    assert CC.want("image_1x1", color_weight=DEFAULT_WEIGHT)["pairs_per_eval"] == [1, 1]      # the pair is there; a 1 x 1 image has no patch


# ------------------------------------------------------------------------------------------------------------ 2, 3. what it is for
def test_the_colour_moves_the_pose_where_depth_cannot():
    """Against the ray cast of the colour fusion of box/40x56/v0.15/t4 (15 cm voxels), 30 iterations, translation error in cm:

        case        start   depth only   w = 0.01    0.1      1       10
        one_wall    7.08      93.51       0.82      0.74    0.66    0.20
        two_walls   6.93      40.86       4.15      3.70    3.24    0.93
        corner      5.69       0.66       0.65      0.59    0.40    1.16
        worst                              4.15      3.70    3.24    1.16   -> the default weight is 10

    Depth alone does not stay put on this model as it did on the prototype's analytic one: the ray cast's normals carry the noise
    of the voxels, the 6 x 6 system passes the pivot rule, and the pose runs off along the plane until three pairs are left.  Only
    w = 10 brings both sliding cases under a quarter of their start.  On `corner` it costs 0.50 cm against depth alone; the margin
    is twice that."""
    worst = {}
    for name in CC.GEOMETRIC:
        c = CC.case(name)
        start, alone = _metres(c["pose_init"], c), _metres(CC.depth_only(name)["transformation"], c)
        ends = {w: _metres(CC.want(name, color_weight=w)["transformation"], c) for w in CC.WEIGHTS}
        print(f"{name}: start {100 * start:.2f} cm, depth only {100 * alone:.2f} cm, colour", {w: round(100 * e, 2) for w, e in ends.items()})
        for w, e in ends.items():
            worst[w] = max(worst.get(w, 0.0), e)
        if name == "corner":
            assert ends[DEFAULT_WEIGHT] <= alone + CORNER_MARGIN
        else:
            assert alone >= 0.9 * start
            assert ends[DEFAULT_WEIGHT] < QUARTER * start
    print("worst", {w: round(100 * e, 2) for w, e in worst.items()})
    assert min(worst, key=worst.get) == DEFAULT_WEIGHT
    src = open(os.path.join(ROOT, "mipsfusion_amd", "tsdf.py")).read()
    assert float(re.search(r"^DEFAULT_COLOR_WEIGHT = ([0-9.]+)$", src, re.M).group(1)) == DEFAULT_WEIGHT


def test_the_relative_stop_needs_the_colour_too():
    """on a lone wall fitness and inlier rmse stand still while the colour moves the pose along the plane: without the third
    condition the loop would stop while the colour rmse still falls"""
    kept = CC.want("one_wall", color_weight=DEFAULT_WEIGHT)
    loose = CC.want("one_wall", color_weight=DEFAULT_WEIGHT, relative_color_rmse=math.inf)
    assert loose["iterations"] <= kept["iterations"] and kept["color_rmse"] <= loose["color_rmse"]
    first = CC.want("one_wall", color_weight=DEFAULT_WEIGHT, max_iteration=0)
    assert kept["color_rmse"] < 0.2 * first["color_rmse"]                 # 0.0054 from 0.0418


# ------------------------------------------------------------------------------------------------------------ 4. no near-ties
@pytest.mark.parametrize("name", CC.CASES)
def test_the_committed_cases_have_no_ambiguous_pixel(name):
    """tests/test_gpu_track_color.py compares pair and row sets for equality.  Every case starts a millimetre beside the pose its
    model was cast from (track_color_cpu.NUDGE): started on it, floor(u) of the first evaluation is a matter of the last bit."""
    c = CC.case(name)
    kw = {} if "color_weight" in c["kw"] else {"color_weight": DEFAULT_WEIGHT}
    for more in ({}, {"max_iteration": 0}):
        w = CC.want(name, **kw, **more)
        assert sum(w["ambiguous_per_eval"]) == 0, (name, w["ambiguous_per_eval"])
        assert (w["partner"] >= 0).sum() == w["n"] and w["color_row"].sum() == w["n_color"] and not (w["color_row"] & (w["partner"] < 0)).any()
    first = CC.want(name, **kw, max_iteration=0)
    H, W = c["H"], c["W"]
    if name == "bad_pixels":
        # the live depth's pattern drops pixels; the colours' pattern (NaN, inf), one pixel further, drops rows of pixels that stay
        # pairs: the fringe of H/2 + W/2 - 1 = 47 pixels, every other one of them not finite
        bad_live = ~np.isfinite(c["live_color"]).all(-1).reshape(-1)
        pairs = first["partner"] >= 0
        assert (pairs & bad_live).sum() >= 20 and not (first["color_row"] & bad_live).any()
        assert not pairs.reshape(H, W)[:H // 2, :W // 2].any() and first["n_color"] < CC.want("corner", color_weight=DEFAULT_WEIGHT, max_iteration=0)["n_color"]
    if name == "color_cut":
        whole = CC.want("one_wall", color_weight=DEFAULT_WEIGHT, max_iteration=0)
        assert abs(first["n_color"] - 0.5 * whole["n_color"]) <= 1 and first["n"] == whole["n"]
    if name == "image_17x33":
        # 561 pixels; pairs project into the last row and column, where no patch exists
        pr, pc = np.divmod(first["partner"][first["partner"] >= 0], W)
        assert pr.min() == 0 and pr.max() == H - 1 and pc.min() == 0 and pc.max() == W - 1 and 0 < first["n_color"] < first["n"]
    if name == "weight_0":
        alone = CC.depth_only("weight_0")
        got = CC.want(name, relative_color_rmse=math.inf)
        assert np.array_equal(got["transformation"], alone["transformation"]) and got["iterations"] == alone["iterations"]


def test_the_patch_reproduces_a_linear_intensity():
    """weights in [0, 1]; on a model whose intensity is linear in (row, col), Im is that field at (v, u) and Iu, Iv its slopes"""
    c = CC.case("corner")
    H, W = c["H"], c["W"]
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b, k = 1.0 / 128, -1.0 / 256, 0.25                                # exact in fp32 at every pixel
    field = (a * col + b * row + k).astype(np.float32)
    assert np.array_equal(field.astype(np.float64), a * col + b * row + k)
    ev = CC.evaluate_color(c["pose_init"].astype(np.float64), c["model_depth"], c["model_normals"], np.repeat(field[..., None], 3, -1), c["pose_ref"],
                           c["live"], c["live_color"], c["K"], math.inf, c["max_dist"], 1.0, math.inf)
    p = ev["patch"]
    assert len(p["u"]) > 2000 and p["fu"].min() >= 0 and p["fu"].max() < 1 and p["fv"].min() >= 0 and p["fv"].max() < 1
    err = np.abs(p["Im"] - (a * p["u"] + b * p["v"] + k)).max()
    print(f"bilinear patch against the linear field: max |difference| {err:.3e}")
    assert err <= 8 * np.finfo(np.float64).eps                          # values below 1, four products and three sums
    assert np.abs(p["Iu"] - a).max() <= 4 * np.finfo(np.float64).eps and np.abs(p["Iv"] - b).max() <= 4 * np.finfo(np.float64).eps


def test_the_closed_form_colour_is_the_renderers():
    import torch
    from mipsfusion_amd import synth
    from . import raster_cpu as R
    v = CC.color_volume()
    H, W, K = R.SIZES["40x56"]
    _, _, lo, hi = R.box_room()
    pose = v["poses"][3]
    f = synth.render_box_frame(synth.config_reference_defaults()["mapping"]["bound"], pose, H, W, *K, drop=0)
    got = CC.box_color(lo, hi, pose.numpy(), K, H, W)
    err = np.abs(got - f["rgb"].numpy()).max()
    print(f"closed-form colour against render_box_frame (fp32): max |difference| {err:.2e}")
    assert err < 1e-5 and got.min() >= 0 and got.max() <= 1              # the renderer works in fp32: 4 x 4 m x 2^-24 in the sine's argument
    assert torch.is_tensor(f["rgb"])


# ------------------------------------------------------------------------------------------------------------ odometry
def test_the_odometry_arc_along_a_wall():
    """8 frames at 33 x 47, K = (100, 100, 23.2, 16.4), facing one wall and sliding 1.5 cm a frame along it, voxels of 10 cm, a
    model that starts from ONE fused frame.  Measured: with the colour (w = 10) 0.63 .. 0.78 cm and 0.21 .. 0.39 degrees a frame,
    aligned ATE 2.2 mm (6.6 mm unaligned); depth alone never moves (its system is refused, every frame keeps the pose before), the
    error grows by 1.5 cm a frame to 10.5 cm, aligned ATE 34.4 mm (62.7 mm unaligned)."""
    from mipsfusion_amd.trajectory import trajectory_metrics
    o = CC.odo_case()
    walk = lambda cw: CC.odometry_color(o["depth"], o["rgb"], o["K"], o["truth"][0], o["origin"], o["voxel"], o["dims"], o["trunc"], color_weight=cw)  # noqa: E731
    (poses, records, _), (alone, _, _) = walk(DEFAULT_WEIGHT), walk(None)
    err = [TC.pose_error(poses[k], o["truth"][k]) for k in range(1, CC.ODO_FRAMES)]
    ate, ate_alone = trajectory_metrics(poses, o["truth"]).rmse, trajectory_metrics(alone, o["truth"]).rmse
    print("odometry: cm", [round(100 * e[1], 2) for e in err], "degrees", [round(e[0], 3) for e in err], f"ATE {1000 * ate:.2f} mm, depth alone {1000 * ate_alone:.2f} mm")
    assert all(np.array_equal(p, o["truth"][0]) for p in alone)
    assert max(e[1] for e in err) <= 2 * 0.0078 and max(e[0] for e in err) <= 2 * 0.39 and ate <= 2 * 0.0022 and ate_alone >= 10 * ate
    assert all(r["n_color"] > 0.8 * r["n"] for r in records[1:])


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_track_color.h")).read()
    declared = set(re.findall(r"\b(mipsf_track_[a-z0-9_]+)\s*\(const", header))
    assert declared == {"mipsf_track_register_color"} == set(_lib.TRACK_COLOR_SIGNATURES)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mipsf_track_register_color")
    assert int(re.search(r"#define MIPSF_TRACK_COLOR_RESULT_DOUBLES +(\d+)u", header).group(1)) == _lib.TRACK_COLOR_RESULT_DOUBLES == CC.RESULT_DOUBLES
    assert _lib.TRACK_COLOR_RESULT_DOUBLES == _lib.TRACK_RESULT_DOUBLES + 2
    assert int(re.search(r"#define MIPSF_TRACK_WS_REGISTER_COLOR +(\d+)", header).group(1)) == _lib.TRACK_WS_REGISTER_COLOR
    # 4 words, 11 doubles, 12 pointers; the block begins as mipsf_track_register_args does
    assert C.sizeof(_lib.TrackRegisterColorArgs) == 16 + 88 + 96
    for field in ("H", "W", "max_iteration", "fx", "relative_rmse"):
        assert getattr(_lib.TrackRegisterColorArgs, field).offset == getattr(_lib.TrackRegisterArgs, field).offset
    ws = _lib.lib().mipsf_track_workspace_bytes
    for H, W in ((40, 56), (17, 33), (1, 1), (0, 5), (8193, 5), (460, 620)):
        assert ws(_lib.TRACK_WS_REGISTER_COLOR, H, W, 0) == ws(_lib.TRACK_WS_REGISTER, H, W, 0)
    assert ws(_lib.TRACK_WS_REGISTER_COLOR, 40, 56, 0) == 256 + 9 * 32 * 8
    import mipsfusion_amd
    from mipsfusion_amd import tsdf
    assert mipsfusion_amd.ColorTrackResult is tsdf.ColorTrackResult and tsdf.ColorTrackResult._fields[:6] == tsdf.TrackResult._fields
    assert len(tsdf.TrackResult._fields) == 6


FAKE = 0x1000                                   # never used: every call below is refused before a pointer is


def _register_color_block(**kw):
    a = dict(H=8, W=9, max_iteration=3, fx=10.0, fy=10.0, cx=4.0, cy=4.0, depth_max=math.inf, max_dist=0.3, relative_fitness=1e-6, relative_rmse=1e-6,
             color_weight=1.0, max_color_diff=math.inf, relative_color_rmse=1e-6, model_depth=FAKE, model_normals=FAKE, model_color=FAKE, pose_ref=FAKE,
             live=FAKE, live_color=FAKE, pose_init=FAKE, result=FAKE, pose_out=FAKE, workspace=FAKE)
    a.update(kw)
    return _lib.TrackRegisterColorArgs.new(**a)


REGISTER_COLOR_REFUSALS = [(dict(H=0), "no pixels"), (dict(W=0), "no pixels"), (dict(H=8193), "a side"), (dict(fx=-1.0), "intrinsics"), (dict(cy=math.nan), "intrinsics"),
                           (dict(depth_max=math.nan), "depth_max"), (dict(max_dist=-0.1), "max_dist"), (dict(max_dist=math.inf), "max_dist"),
                           (dict(max_dist=math.nan), "max_dist"), (dict(max_iteration=1001), "max_iteration"),
                           (dict(color_weight=-1.0), "color_weight"), (dict(color_weight=math.inf), "color_weight"), (dict(color_weight=math.nan), "color_weight"),
                           (dict(max_color_diff=-0.5), "max_color_diff"), (dict(max_color_diff=math.nan), "max_color_diff"),
                           (dict(relative_color_rmse=math.nan), "relative_color_rmse"),
                           (dict(model_color=None), "colour pointer"), (dict(live_color=None), "colour pointer"),
                           (dict(model_depth=None), "null pointer"), (dict(model_normals=None), "null pointer"), (dict(pose_ref=None), "null pointer"),
                           (dict(live=None), "null pointer"), (dict(pose_init=None), "null pointer"), (dict(result=None), "null pointer"),
                           (dict(pose_out=None), "null pointer"), (dict(workspace=None), "null pointer"), (dict(workspace=FAKE + 4), "16-byte")]


def _ids(refusals):
    return [f"{list(c)[0]}={list(c.values())[0]}" for c, _ in refusals]


@pytest.mark.parametrize("change,said", REGISTER_COLOR_REFUSALS, ids=_ids(REGISTER_COLOR_REFUSALS))
def test_the_colour_registration_refuses_what_is_out_of_range(change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_register_color(C.byref(_register_color_block(**change)), None) != 0
    assert b"mipsf_track_register_color" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_struct_size_is_checked():
    lib = _lib.lib()
    blk = _lib.TrackRegisterColorArgs.new()
    blk.struct_size -= 4
    assert lib.mipsf_track_register_color(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
    assert lib.mipsf_track_register_color(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
