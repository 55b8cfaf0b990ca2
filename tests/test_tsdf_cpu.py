"""CPU: the float64 restatement of the TSDF fusion (tests/tsdf_cpu.py) held to what is known without a GPU -- the walls of the box
room, the invariance to the cut into calls, occlusion and carving in the two rooms, the inputs that must update nothing -- the
restated brick culling of csrc/tsdf.hip held to `never leaves out a pair the rule updates`, and the C ABI of the new entry points.
tests/test_gpu_tsdf.py holds the device to the restatement for equality of words."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import raster_cpu as R
from . import tsdf_cpu as T
from .conftest import ROOT

MEAN_GATE, MAX_GATE = T.MEAN_GATE, T.MAX_GATE


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(T.BOX_CASES))
def test_the_fused_box_room_lies_on_its_walls(name):
    """Distance of every used vertex of the marched fused volume to the nearest wall plane, in voxels.  Measured with this
    restatement (mean, 95th percentile, max; faces):
        box/40x56/v0.15/t4   27x47x31   0.052  0.205  0.500    6 421
        box/33x47/v0.20/t3   22x37x25   0.060  0.250  0.500    3 110
        box/40x56/v0.10/t4   37x67x43   0.041  0.193  0.500   17 176
    A half-voxel error in the index-to-world convention would move the mean to 0.5."""
    c = T.case(name)
    _, _, lo, hi = R.box_room()
    v, f, _ = T.extract_mesh(c["state"], c["origin"], c["voxel"])
    used = np.unique(f)
    d = T.wall_distance(v[used], lo, hi) / c["voxel"]
    print(f"{name}: dims {c['dims']}, faces {len(f)}, wall distance in voxels: mean {d.mean():.3f}, p95 {np.percentile(d, 95):.3f}, max {d.max():.3f}; "
          f"updates {c['updates']}, observed {c['observed']}")
    assert len(f) > 1000 and d.mean() <= MEAN_GATE and d.max() <= MAX_GATE


def test_the_cut_into_calls_does_not_reach_the_bytes():
    c = T.case("box/33x47/v0.20/t3")
    state = T.new_state(c["dims"])
    updates = 0
    for k in range(0, len(c["poses"]), 3):
        u, observed = T.integrate(state, c["ticks"], c["depth"][k:k + 3], c["poses"][k:k + 3], c["K"], c["trunc"])
        updates += u
    assert state["tsdf"].tobytes() == c["state"]["tsdf"].tobytes() and state["weight"].tobytes() == c["state"]["weight"].tobytes()
    assert (updates, observed) == (c["updates"], c["observed"])


def test_occlusion_and_carving_in_the_two_rooms():
    from mipsfusion_amd import synth
    c = T.case("two_rooms/v0.20")
    P = R._poses(c["poses"])
    hidden = np.ones(c["dims"], bool)           # more than trunc behind the surface along every view that sees the voxel's pixel
    seen_by_some = np.zeros(c["dims"], bool)
    for k, pose in enumerate(P):
        z, inside, ri, ci = T._project(c["ticks"], pose, c["K"], c["H"], c["W"])
        d = c["depth"][k][ri, ci].astype(np.float64)
        measured = inside & (d > 0)
        hidden &= ~measured | (z > d + c["trunc"] + 1e-9)
        seen_by_some |= measured
    behind = hidden & seen_by_some
    print(f"two rooms: {int(behind.sum())} voxels behind a surface in every view that has their pixel, {int((c['state']['weight'] > 0).sum())} observed")
    assert behind.sum() > 1000 and not c["state"]["weight"][behind].any() and not c["state"]["tsdf"][behind].any()
    # the door opening, 30 cm clear of its frame, within a voxel of the shared wall's plane: the views through the door carve it
    door, zw = synth.TWO_ROOMS["door"], synth.TWO_ROOMS["room_a"][2][1]
    x, y, z = np.meshgrid(*c["ticks"], indexing="ij")
    opening = (x > door[0][0] + 0.3) & (x < door[0][1] - 0.3) & (y > door[1][0] + 0.3) & (y < door[1][1] - 0.3) & (np.abs(z - zw) < 0.2)
    w, t = c["state"]["weight"][opening], c["state"]["tsdf"][opening]
    seen = w > 0
    print(f"door opening: {int(opening.sum())} voxels, {int(seen.sum())} seen, weights up to {w.max()}, tsdf of the seen {t[seen].min()} .. {t[seen].max()}")
    assert seen.sum() >= 20 and (t[seen] == 1.0).all()


def test_inputs_that_update_nothing():
    c = T.case("bad_pixels")
    H, W = c["H"], c["W"]
    bad = ~((c["depth"] > 0) & np.isfinite(c["depth"]) & (c["depth"] <= c["depth_max"]))
    assert bad[:, :H // 2, :W // 2].all() and bad[:, H // 2:, :W // 2][:, ::3].all() and 0.2 < bad.mean() < 0.9
    P = R._poses(c["poses"])
    for k, pose in enumerate(P):                # no updated pair lands on a bad pixel
        _, inside, ri, ci = T._project(c["ticks"], pose, c["K"], H, W)
        assert not (c["updated"][k] & bad[k][ri, ci]).any() and not (c["updated"][k] & ~inside).any()
    assert 0 < c["updates"] < T.case("box/33x47/v0.20/t3")["updates"]
    # a camera at a voxel, looking along -z: the voxels of its plane z == 0 and those behind it update nothing
    ticks = T.make_ticks((0.0, 0.0, 0.0), 0.25, (5, 5, 9))
    import torch
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.5, 0.5, 1.0])
    depth = np.full((1, 33, 47), 0.45, np.float32)
    state = T.new_state((5, 5, 9))
    updates, observed, updated = T.integrate(state, ticks, depth, pose[None], R.SIZES["33x47"][2], 0.5, return_pairs=True)
    assert updates == observed > 0 and not updated[0][:, :, 4:].any() and not state["weight"][:, :, 4:].any()
    assert updated[0][2, 2, 3] and state["weight"][2, 2, 3] == 1.0
    # behind the surface by more than trunc: nothing either
    assert not updated[0][:, :, 0].any()


def test_max_weight_and_odd_shapes():
    free, capped = T.case("box/33x47/v0.20/t3"), T.case("max_weight_2")
    count = free["updated"].sum(0)
    assert np.array_equal(free["state"]["weight"], count.astype(np.float32)) and count.max() > 2
    assert np.array_equal(capped["state"]["weight"], np.minimum(count, 2).astype(np.float32)) and capped["updates"] == free["updates"]
    one, thin = T.case("one_voxel"), T.case("1x5x70")
    assert one["state"]["tsdf"].shape == (1, 1, 1) and one["state"]["weight"][0, 0, 0] == one["updates"] >= 1 and 0.0 < one["state"]["tsdf"][0, 0, 0] <= 1.0
    assert thin["state"]["tsdf"].shape == (1, 5, 70) and 0 < thin["observed"] < 350
    assert thin["state"]["tsdf"].min() < 0 < thin["state"]["tsdf"].max() == 1.0            # the column crosses the wall
    out = T.case("outside")
    assert out["updates"] == 0 and out["observed"] == 0 and not out["state"]["tsdf"].any()
    assert len(T.case("many_views")["poses"]) == _lib.TSDF_VIEW_CHUNK + 1 and T.case("many_views")["updated"][-1].any()


@pytest.mark.parametrize("name", T.EQUALITY_CASES)
def test_the_brick_culling_leaves_out_no_pair(name):
    """csrc/tsdf.hip gives a brick only the views its bounding sphere can be updated by; the restatement tests every pair.  The
    culling's arithmetic, restated in numpy (tsdf_cpu.brick_keeps), keeps every (brick, view) with an updated voxel, on every
    case the GPU test fuses; and it does cull."""
    c = T.case(name)
    keeps = T.brick_keeps(c["ticks"], c["poses"], c["K"], c["H"], c["W"], c["trunc"], c["depth_max"])
    needed = T.pairs_by_brick(c["updated"])
    assert keeps.shape == needed.shape
    print(f"{name}: {needed.size} (brick, view) pairs, {int(needed.sum())} with an update, {int(keeps.sum())} kept")
    assert not (needed & ~keeps).any()
    if name == "outside":
        assert not keeps.any()
    if name in T.BOX_CASES:
        assert keeps.sum() < 0.6 * keeps.size


def test_colour_follows_the_same_mean():
    c = T.case("colour")
    s = c["state"]
    seen = s["weight"] > 0
    assert seen.any() and not s["color"][~seen].any() and s["color"][seen].min() >= 0.0 and s["color"][seen].max() <= 1.0
    v, f, vi = T.extract_mesh(s, c["origin"], c["voxel"])
    col = T.sample_color(vi, s["weight"], s["color"])
    used = np.unique(f)
    want = 0.5 + 0.5 * np.sin(4.0 * v[used])                 # the colour of the wall point next to the vertex; smooth, so close
    print(f"colour: {len(used)} vertices, largest difference to the analytic colour {np.abs(col[used] - want).max():.3f}, mean {np.abs(col[used] - want).mean():.3f}")
    assert np.abs(col[used] - want).mean() < 0.1
    assert not T.sample_color(np.array([[np.nan, 1.0, 1.0], [1e9, -5.0, 2.0]]), np.zeros((3, 3, 3), np.float32), np.ones((3, 3, 3, 3), np.float32)).any()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_tsdf.h")).read()
    declared = set(re.findall(r"\b(mipsf_tsdf_[a-z0-9_]+)\s*\(", header))
    assert declared == {"mipsf_tsdf_integrate", "mipsf_tsdf_sample"} == set(_lib.TSDF_SIGNATURES)
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_TSDF_MAX_VOXELS", _lib.TSDF_MAX_VOXELS), ("MIPSF_TSDF_MAX_SIDE", _lib.TSDF_MAX_SIDE),
                         ("MIPSF_TSDF_VIEW_CHUNK", _lib.TSDF_VIEW_CHUNK), ("MIPSF_TSDF_MAX_BRICKS", _lib.TSDF_MAX_BRICKS), ("MIPSF_TSDF_NO_CULL", _lib.TSDF_NO_CULL),
                         ("MIPSF_TSDF_BRICK_X", _lib.TSDF_BRICK[0]), ("MIPSF_TSDF_BRICK_Y", _lib.TSDF_BRICK[1]), ("MIPSF_TSDF_BRICK_Z", _lib.TSDF_BRICK[2])):
        assert int(re.search(rf"#define {macro} (0x[0-9a-f]+|\d+)u", header).group(1), 0) == value, macro
    assert (T.VIEW_CHUNK, T.BRICK) == (_lib.TSDF_VIEW_CHUNK, _lib.TSDF_BRICK)
    # 8 words, 7 doubles, 10 pointers; 6 words, 4 pointers: what the header's structs come to on this ABI
    assert C.sizeof(_lib.TsdfIntegrateArgs) == 32 + 56 + 80 and C.sizeof(_lib.TsdfSampleArgs) == 24 + 32
    import mipsfusion_amd
    from mipsfusion_amd import tsdf
    for name in ("TSDFVolume", "tsdf_mesh_from_frames", "mesh_from_rendered_depth"):
        assert getattr(mipsfusion_amd, name) is getattr(tsdf, name)


def _good(**kw):
    fake = 0x1000                               # never used: every call below is refused before a pointer is
    a = dict(X=4, Y=5, Z=6, n=2, H=8, W=9, fx=10.0, fy=10.0, cx=4.0, cy=4.0, trunc=0.3, depth_max=math.inf, max_weight=math.inf,
             depth=fake, poses=fake, tsdf=fake, weight=fake, record=fake)
    a.update(kw)
    blk = _lib.TsdfIntegrateArgs.new(**a)
    for d in range(3):
        blk.ticks[d] = fake
    return blk


REFUSALS = [(dict(X=0), "no voxels"), (dict(Y=0), "no voxels"), (dict(Z=0), "no voxels"), (dict(H=0), "no pixels"), (dict(W=0), "no pixels"),
            (dict(X=2048, Y=1024, Z=1024), "at most 2"), (dict(X=1 << 31, Y=1, Z=1), "at most 2"), (dict(X=1 << 28, Y=1, Z=1), "bricks"), (dict(H=8193), "a side"),
            (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=math.inf), "trunc"), (dict(trunc=math.nan), "trunc"),
            (dict(fx=0.0), "intrinsics"), (dict(fy=-3.0), "intrinsics"), (dict(fx=math.inf), "intrinsics"), (dict(fy=math.nan), "intrinsics"),
            (dict(cx=math.inf), "intrinsics"), (dict(cy=math.nan), "intrinsics"), (dict(depth_max=math.nan), "depth_max"),
            (dict(max_weight=0.5), "max_weight"), (dict(max_weight=math.nan), "max_weight"), (dict(flags=2), "flags"),
            (dict(rgb=0x1000), "go together"), (dict(color=0x1000), "go together"),
            (dict(depth=None), "null pointer"), (dict(poses=None), "null pointer"), (dict(tsdf=None), "null pointer"),
            (dict(weight=None), "null pointer"), (dict(record=None), "null pointer")]


@pytest.mark.parametrize("change,said", REFUSALS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in REFUSALS])
def test_what_is_out_of_range_is_refused_on_the_host(change, said):
    lib = _lib.lib()
    assert lib.mipsf_tsdf_integrate(C.byref(_good(**change)), None) != 0
    assert said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_struct_sizes_null_ticks_and_the_sampler_are_refused_too():
    lib = _lib.lib()
    for cls, fn in ((_lib.TsdfIntegrateArgs, lib.mipsf_tsdf_integrate), (_lib.TsdfSampleArgs, lib.mipsf_tsdf_sample)):
        blk = cls.new()
        blk.struct_size -= 4
        assert fn(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
        assert fn(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
    blk = _good()
    blk.ticks[1] = None
    assert lib.mipsf_tsdf_integrate(C.byref(blk), None) != 0 and b"null pointer" in lib.mipsf_last_error()
    assert lib.mipsf_tsdf_sample(C.byref(_lib.TsdfSampleArgs.new(X=0, Y=3, Z=3, m=1)), None) != 0 and b"no voxels" in lib.mipsf_last_error()
    assert lib.mipsf_tsdf_sample(C.byref(_lib.TsdfSampleArgs.new(X=3, Y=3, Z=3, m=1)), None) != 0 and b"null pointer" in lib.mipsf_last_error()
    assert lib.mipsf_tsdf_sample(C.byref(_lib.TsdfSampleArgs.new(X=3, Y=3, Z=3, m=0)), None) == 0
    from mipsfusion_amd import tsdf
    with pytest.raises(ValueError, match="voxel size 0.001"):
        tsdf.TSDFVolume((0, 0, 0), 0.001, (2048, 1024, 1024), 0.004, device="cuda")
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            tsdf.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4)
