"""The restatement of the brick-sparse TSDF volume (tests/sparse_cpu.py) held to its conditions, without a GPU: on the convex box
room the masked dense state gives what the dense state gives; on the two rooms it need not, and how far apart they are is printed;
the cut into calls does not reach a word while nothing is dropped; a pool that is too small takes the first bricks in order; and the
shared cases hold no decision that a last-bit difference could flip.  Then the C ABI: header, library and package agree, and the
host refuses what the header says it refuses.

On the last-bit count.  An i0 coordinate within 1e-9 of an integer cannot be avoided in these cases: the walls of the box room lie ON
lattice planes (the grid starts three voxels outside them), a depth pixel puts a point on a wall to the rounding of its fp32 depth,
about 1e-6 voxel, so about one wall pixel in a thousand lands within 1e-9 of the plane, whatever the pose.  Those are printed.  What
is asserted to be zero is what a last-bit difference can reach: a coordinate within 64 last bits of an integer, and z within 1e-12
of 0; tsdf_cpu's views that had thousands of those (they look straight at a wall from a distance fp32 holds exactly) are turned by
a hundredth of a radian in sparse_cpu."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import sparse_cpu as S
from . import track_cpu as K_
from . import tsdf_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ masked = dense, convex
BORN_LATE = {"box/40x56/v0.15/t4": (48, 48, 37), "box/40x56/v0.10/t4": (129, 135, 106), S.BOX80: (523, 720, 458)}   # allocated, bricks, born after view 0
# (the last with views 13 and 14 turned, see above; 521 and 456 with tsdf_cpu's poses as they are)


@pytest.mark.parametrize("name", S.BOX_CASES)
def test_on_the_box_room_the_masked_state_gives_what_the_dense_state_gives(name):
    c = S.case(name)
    sp, dense = c["sp"], S.dense(name)
    nb = sp["bricks"]
    late = sum(1 for v in c["counts"]["births"].values() if v > 0)
    print(f"{name}: dims {c['dims']}, {c['counts']['in_use']} of {nb[0] * nb[1] * nb[2]} bricks, {late} born after view 0, views moved {c.get('moved')}")
    assert (c["counts"]["in_use"], nb[0] * nb[1] * nb[2], late) == BORN_LATE[name] and c["counts"]["dropped"] == 0
    observed = sp["state"]["weight"] > 0
    assert observed.sum() == c["counts"]["observed"] > 0
    assert np.array_equal(_words(sp["state"]["tsdf"])[observed], _words(dense["tsdf"])[observed])
    got, want = S.extract_mesh(sp), T.extract_mesh(dense, c["origin"], c["voxel"])
    assert len(want[1]) > 1000 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _, _, lo, hi = S.R.box_room()
    dist = T.wall_distance(got[0], lo, hi) / c["voxel"]
    print(f"  wall distance in voxels: mean {dist.mean():.3f}, max {dist.max():.3f}")
    assert dist.mean() < T.MEAN_GATE and dist.max() < T.MAX_GATE
    poses = c["poses"][list(K_.BOX_VIEWS)]
    a = S.raycast(sp, poses, c["K"], c["H"], c["W"])
    b = K_.raycast(dense, c["origin"], c["voxel"], poses, c["K"], c["H"], c["W"], 0.5 * c["trunc"])
    print(f"  ray cast from views {K_.BOX_VIEWS}: hits {a['hits']} of {3 * c['H'] * c['W']}")
    assert a["hits"] == b["hits"] > 0.9 * 3 * c["H"] * c["W"] and np.array_equal(_words(a["depth"]), _words(b["depth"]))


def test_on_the_two_rooms_the_two_states_may_differ_and_this_is_how_far():
    """Not convex: a view through the door can fuse free space in a brick of the far room that it does not mark (its depth pixels
    end elsewhere), and a brick born later has then missed a view the dense voxel took.  Measured here: it does not happen at this
    voxel size -- all 45 bricks of the grid get a slot, 15 of them after view 0, and no word, face or hit differs."""
    name = "two_rooms/v0.20"
    c = S.case(name)
    sp, dense = c["sp"], S.dense(name)
    observed = sp["state"]["weight"] > 0
    differing = int((_words(sp["state"]["tsdf"])[observed] != _words(dense["tsdf"])[observed]).sum())
    got, want = S.extract_mesh(sp), T.extract_mesh(dense, c["origin"], c["voxel"])
    a = S.raycast(sp, c["poses"], c["K"], c["H"], c["W"])
    b = K_.raycast(dense, c["origin"], c["voxel"], c["poses"], c["K"], c["H"], c["W"], 0.5 * c["trunc"])
    print(f"{name}: {differing} of {int(observed.sum())} observed tsdf words differ ({differing / observed.sum():.4f}); dense observes "
          f"{int((dense['weight'] > 0).sum())}; faces {len(got[1])} against {len(want[1])}; hits {a['hits']} against {b['hits']}; "
          f"depth words differing {int((_words(a['depth']) != _words(b['depth'])).sum())}")
    assert (differing, int(observed.sum()), len(got[1]), len(want[1]), a["hits"], b["hits"]) == TWO_ROOMS_MEASURED


TWO_ROOMS_MEASURED = (0, 18433, 2896, 2896, 11147, 11147)          # measured with this restatement: differing words, observed, faces masked / dense, hits masked / dense


# ------------------------------------------------------------------------------------------------------------ cuts and drops
@pytest.mark.parametrize("name", ["box/40x56/v0.15/t4", "colour"])
def test_the_cut_into_calls_does_not_reach_a_word_while_nothing_is_dropped(name):
    want = S.case(name)
    for per in (1, 3):
        sp, counts = S.fuse(name, views_per_call=per)
        assert counts["dropped"] == 0 and sorted(sp["slot_brick"]) == sorted(want["sp"]["slot_brick"])
        assert (counts["updates"], counts["observed"], counts["in_use"]) == tuple(want["counts"][k] for k in ("updates", "observed", "in_use"))
        for key in ("tsdf", "weight") + (("color",) if want["rgb"] is not None else ()):
            assert np.array_equal(_words(sp["state"][key]), _words(want["sp"]["state"][key])), (per, key)
        if per == 1:                                             # only the numbering of the slots depends on the cut
            assert sp["slot_brick"] != want["sp"]["slot_brick"]


def test_a_pool_that_is_too_small_takes_the_first_bricks_in_order():
    name = "box/40x56/v0.10/t4"
    full = S.case(name)
    need = full["counts"]["in_use"]
    sp, counts = S.fuse(name, capacity=need // 2)
    assert sp["slot_brick"] == sorted(full["sp"]["slot_brick"])[:need // 2] == full["sp"]["slot_brick"][:need // 2]
    assert (counts["new"], counts["dropped"], counts["in_use"], counts["marked"]) == (need // 2, need - need // 2, need // 2, need)
    table = S.table_of(sp).reshape(-1)
    assert (table >= 0).sum() == need // 2 and np.array_equal(np.flatnonzero(table >= 0), np.asarray(sp["slot_brick"]))
    # the bricks that have a slot hold what they hold in the full volume; the others hold nothing
    mask = S._voxel_mask(sp, table >= 0)
    assert np.array_equal(_words(sp["state"]["tsdf"])[mask], _words(full["sp"]["state"]["tsdf"])[mask]) and not sp["state"]["weight"][~mask].any()
    # a second call finds the pool full: everything marked and unallocated is dropped again, nothing moves
    c = S.inputs(name)
    again = S.allocate(sp, c["depth"][:3], c["poses"][:3], c["K"])
    assert again["new"] == 0 and again["dropped"] > 0 and again["in_use"] == need // 2 and len(sp["slot_brick"]) == need // 2


def test_a_nan_pose_marks_and_updates_nothing():
    c = S.inputs("nan_pose")
    sp = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], 64)
    counts = S.integrate(sp, c["depth"][2:3], c["poses"][2:3], c["K"])
    assert not np.isfinite(c["poses"][2].numpy()).any()
    assert (counts["marked"], counts["in_use"], counts["updates"], counts["observed"]) == (0, 0, 0, 0) and not sp["state"]["weight"].any()


@pytest.mark.parametrize("name", S.GPU_CASES + tuple(n for n in S.BOX_CASES if n not in S.GPU_CASES))
def test_the_shared_cases_hold_no_decision_a_last_bit_could_flip(name):
    c = S.case(name)
    z0, near, last_bits = (int(x) for x in c["sp"]["ambiguous"])
    print(f"{name}: z within 1e-12 of 0: {z0}; i0 coordinates within 1e-9 of an integer: {near}; within 64 last bits: {last_bits}; views moved {c.get('moved')}")
    assert z0 == 0 and last_bits == 0
    assert S.inside_window(c["sp"]) and c["counts"]["dropped"] == 0


def test_the_virtual_grid_is_past_the_dense_limit_and_costs_what_its_room_costs():
    c = S.case(S.VIRTUAL)
    room = S.case("box/40x56/v0.10/t4")
    assert c["dims"][0] * c["dims"][1] * c["dims"][2] > _lib.TSDF_MAX_VOXELS and c["sp"]["state"]["tsdf"].size < 400000
    assert c["counts"]["in_use"] > room["counts"]["in_use"]                 # the band reaches past the room's own grid
    first = tuple(int(x) for x in np.asarray(c["sp"]["slot_brick"][:1]) // (c["sp"]["bricks"][1] * c["sp"]["bricks"][2]))
    assert first[0] == S.VIRTUAL_BRICK[0] - 1
    from mipsfusion_amd import tsdf
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], device="cuda")


# ------------------------------------------------------------------------------------------------------------ the C ABI
NAMES = {"mipsf_sparse_scan_words", "mipsf_sparse_allocate", "mipsf_sparse_integrate", "mipsf_sparse_gather", "mipsf_sparse_raycast"}


def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_sparse.h")).read()
    declared = set(re.findall(r"\b(mipsf_sparse_[a-z0-9_]+)\s*\(", header))
    assert declared == NAMES == set(_lib.SPARSE_SIGNATURES)
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_SPARSE_BRICK_VOXELS", _lib.SPARSE_BRICK_VOXELS), ("MIPSF_SPARSE_MAX_BRICKS", _lib.SPARSE_MAX_BRICKS),
                         ("MIPSF_SPARSE_MAX_CAPACITY", _lib.SPARSE_MAX_CAPACITY), ("MIPSF_SPARSE_MAX_STEPS", _lib.SPARSE_MAX_STEPS),
                         ("MIPSF_SPARSE_MAX_VIEWS", _lib.SPARSE_MAX_VIEWS), ("MIPSF_SPARSE_SCAN_TILE", _lib.SPARSE_SCAN_TILE),
                         ("MIPSF_SPARSE_NO_SKIP", _lib.SPARSE_NO_SKIP)):
        assert int(re.search(rf"#define {macro} (0x[0-9a-f]+|\d+)u", header).group(1), 0) == value, macro
    assert _lib.SPARSE_BRICK_VOXELS == int(np.prod(T.BRICK)) and _lib.SPARSE_MAX_CAPACITY == (1 << 31) // 2048
    # the volume: 4 words, 4 doubles, 10 pointers; then 6 words, 6 doubles, 5 pointers; 6, 7, 4; 8 words, 3 pointers; 6, 9, 5
    assert C.sizeof(_lib.SparseVolume) == 128
    assert [C.sizeof(x) for x in (_lib.SparseAllocateArgs, _lib.SparseIntegrateArgs, _lib.SparseGatherArgs, _lib.SparseRaycastArgs)] == [240, 240, 184, 264]
    lib = _lib.lib()
    assert lib.mipsf_sparse_scan_words(2048, 2048, 2048) == 256 * 256 * 128 // 1024 + 1 and lib.mipsf_sparse_scan_words(0, 4, 4) == 0
    assert lib.mipsf_sparse_scan_words(1 << 31, 1 << 31, 16) == 0
    import mipsfusion_amd
    from mipsfusion_amd import sparse_tsdf
    for name in ("SparseTSDFVolume", "SparseTSDFCounts", "sparse_tsdf_mesh_from_frames", "sparse_tsdf_odometry"):
        assert getattr(mipsfusion_amd, name) is getattr(sparse_tsdf, name)


def _volume(**kw):
    fake = 0x1000                               # never used: every call below is refused before a pointer is
    g = _lib.SparseVolume()
    a = dict(X=40, Y=50, Z=60, capacity=16, voxel=0.1, table=fake, slot_brick=fake, birth=fake, count=fake, tsdf=fake, weight=fake)
    a.update(kw)
    ticks = a.pop("ticks", (fake, fake, fake))
    origin = a.pop("origin", (0.0, 0.0, 0.0))
    for k, v in a.items():
        setattr(g, k, v)
    for d in range(3):
        g.ticks[d], g.origin[d] = ticks[d], origin[d]
    return g


def _block(which, vol=None, **kw):
    fake = 0x1000
    vol = {} if vol is None else vol
    image = dict(n=2, H=8, W=9, fx=10.0, fy=10.0, cx=4.0, cy=4.0)
    if which == "allocate":
        a = dict(image, steps=4, band=0.4, depth_max=math.inf, depth=fake, poses=fake, mark=fake, scan=fake, record=fake)
        cls, fn = _lib.SparseAllocateArgs, "mipsf_sparse_allocate"
    elif which == "integrate":
        a = dict(image, trunc=0.4, depth_max=math.inf, max_weight=math.inf, depth=fake, poses=fake, record=fake)
        cls, fn = _lib.SparseIntegrateArgs, "mipsf_sparse_integrate"
    elif which == "raycast":
        a = dict(image, trunc=0.4, near=0.0, far=math.inf, step=0.2, min_weight=1.0, poses=fake, depth=fake, record=fake)
        cls, fn = _lib.SparseRaycastArgs, "mipsf_sparse_raycast"
    else:
        a = dict(tsdf=fake, weight=fake)
        cls, fn = _lib.SparseGatherArgs, "mipsf_sparse_gather"
    lo, hi = kw.pop("lo", (0, 0, 0)), kw.pop("hi", (8, 8, 8))
    a.update(kw)
    blk = cls.new(vol=_volume(**vol), **a)
    if which == "gather":
        for d in range(3):
            blk.lo[d], blk.hi[d] = lo[d], hi[d]
    return blk, fn


EVERYWHERE = [(dict(X=0), "no voxels"), (dict(Z=0), "no voxels"), (dict(X=1 << 31, Y=1 << 10, Z=1 << 10), "2^31 bricks"),
              (dict(X=(1 << 14) * 8, Y=(1 << 14) * 8, Z=8 * 16), "2^31 bricks"), (dict(capacity=0), "capacity"), (dict(capacity=(1 << 20) + 1), "capacity"),
              (dict(voxel=0.0), "voxel"), (dict(voxel=math.nan), "voxel"), (dict(origin=(0.0, math.inf, 0.0)), "origin"), (dict(table=None), "null pointer"),
              (dict(count=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(ticks=(0x1000, None, 0x1000)), "null pointer")]
REFUSALS = [(w, v, {}, said) for w in ("allocate", "integrate", "gather", "raycast") for v, said in EVERYWHERE] + [
    ("allocate", {}, dict(band=-0.1), "band"), ("allocate", {}, dict(band=math.nan), "band"), ("allocate", {}, dict(band=math.inf), "band"),
    ("allocate", {}, dict(steps=4097), "steps"), ("allocate", {}, dict(H=0), "no pixels"), ("allocate", {}, dict(W=8193), "a side"),
    ("allocate", {}, dict(n=65536), "views"), ("allocate", {}, dict(fx=0.0), "intrinsics"), ("allocate", {}, dict(cy=math.nan), "intrinsics"),
    ("allocate", {}, dict(depth_max=math.nan), "depth_max"), ("allocate", {}, dict(mark=None), "null pointer"), ("allocate", {}, dict(scan=None), "null pointer"),
    ("allocate", {}, dict(depth=None), "null pointer"), ("allocate", {}, dict(record=None), "null pointer"),
    ("integrate", {}, dict(trunc=0.0), "trunc"), ("integrate", {}, dict(trunc=math.nan), "trunc"), ("integrate", {}, dict(max_weight=0.5), "max_weight"),
    ("integrate", {}, dict(flags=2), "flags"), ("integrate", {}, dict(rgb=0x1000), "go together"), ("integrate", dict(color=0x1000), {}, "go together"),
    ("integrate", {}, dict(depth_max=math.nan), "depth_max"), ("integrate", {}, dict(poses=None), "null pointer"), ("integrate", {}, dict(W=0), "no pixels"),
    ("gather", {}, dict(lo=(8, 0, 0)), "window"), ("gather", {}, dict(hi=(41, 8, 8)), "window"), ("gather", {}, dict(tsdf=None), "null pointer"),
    ("gather", {}, dict(color=0x1000), "needs a volume with color"),
    ("gather", dict(X=2048, Y=2048, Z=2048), dict(hi=(2048, 1024, 1024)), "at most 2^31 - 1"),
    ("raycast", {}, dict(step=0.0), "step"), ("raycast", {}, dict(step=1e-6), "samples a ray"), ("raycast", {}, dict(near=math.nan), "near or far"),
    ("raycast", {}, dict(min_weight=math.nan), "min_weight"), ("raycast", {}, dict(flags=2), "flags"), ("raycast", {}, dict(color_out=0x1000), "color_out"),
    ("raycast", {}, dict(trunc=-1.0), "trunc"), ("raycast", {}, dict(depth=None), "null pointer"), ("raycast", {}, dict(n=65536), "views")]


@pytest.mark.parametrize("which,vol,change,said", REFUSALS, ids=[f"{w}:{list(v or c)[0]}={list((v or c).values())[0]}" for w, v, c, _ in REFUSALS])
def test_what_is_out_of_range_is_refused_on_the_host(which, vol, change, said):
    lib = _lib.lib()
    blk, fn = _block(which, vol, **change)
    assert getattr(lib, fn)(C.byref(blk), None) != 0
    assert said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_struct_sizes_and_the_python_side_are_refused_too():
    lib = _lib.lib()
    for which in ("allocate", "integrate", "gather", "raycast"):
        blk, fn = _block(which)
        blk.struct_size -= 4
        assert getattr(lib, fn)(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
        assert getattr(lib, fn)(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
    from mipsfusion_amd import sparse_tsdf
    for kw, said in ((dict(dims=(1 << 20, 1 << 20, 1 << 20)), "2\\^31 bricks"), (dict(capacity_bricks=0), "capacity_bricks"),
                     (dict(capacity_bricks=(1 << 20) + 1), "capacity_bricks"), (dict(band=-1.0), "band"), (dict(band=math.nan), "band"),
                     (dict(voxel_size=0.0), "voxel_size"), (dict(dims=(4, 0, 4)), "dims")):
        a = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(64, 64, 64), trunc=0.4, capacity_bricks=8, device="cuda")
        a.update(kw)
        with pytest.raises(ValueError, match=said):
            sparse_tsdf.SparseTSDFVolume(**a)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            sparse_tsdf.SparseTSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, 8)
