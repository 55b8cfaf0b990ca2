"""CPU: the float64 restatement of the removal of fused views from the brick-sparse volume (tests/sparse_remove_cpu.py) held to what
is known without a GPU -- removing every view gives back all-zero words, removing half the views gives the fusion that skipped
them, the history is what makes that so, `born` does not depend on the cut into calls, the drift route puts the mesh back on the
walls, no input has a floor decided by a last bit -- and the C ABI of include/mipsf_sparse_remove.h.
tests/test_gpu_sparse_remove.py holds the device to the restatement for equality of words."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import raster_cpu as R
from . import sparse_cpu as S
from . import sparse_remove_cpu as SR
from . import tsdf_cpu as T
from . import tsdf_remove_cpu as RM
from .conftest import ROOT


def _zero(state):
    return all(not v.view(np.uint32).any() for v in state.values() if v is not None)          # the words: no -0.0 either


# ------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", SR.GPU_CASES)
def test_removing_every_view_gives_back_all_zero_words(name):
    c = SR.case(name)
    ev, od, counts = c["removed_even"], c["removed_odd"], c["counts"]
    print(f"{name}: fused {counts['updates']} pairs into {counts['observed']} voxels of {counts['in_use']} bricks; even positions removed "
          f"{ev[:5]}, then the rest {od[:5]}")
    assert _zero(c["none"]["state"])
    assert ev[0] + od[0] == counts["updates"] and ev[2] + od[2] == counts["observed"]
    assert ev[1] == od[1] == 0 and od[3] == 0 and od[4] == counts["in_use"] and ev[5] >= 0 and od[5] == 0
    # nothing is freed, and the history stays
    for key in ("table", "born"):
        assert np.array_equal(c["none"][key], c["fused"][key])
    assert c["none"]["slot_brick"] == c["fused"]["slot_brick"]
    # with every brick taking every view the restatement is tsdf_remove_cpu's, count for count: the mask is the only thing added
    if name == "colour":
        sp = SR.copy_volume(c["fused"])
        dense = RM.copy_state(sp["state"])
        want = RM.remove(dense, sp["ticks"], c["depth"][:1], c["poses"][:1], c["K"], sp["trunc"], c["depth_max"], c["rgb"][:1])
        sp["born"][sp["table"] >= 0] = 0
        got = SR.remove(sp, c["depth"][:1], c["poses"][:1], c["K"], [0], c["rgb"][:1], c["depth_max"])
        # (a hit outside the allocated bricks is missing to the dense rule and nothing to the sparse one)
        assert (got[0], got[2], got[3]) == (want[0], want[2], want[3]) and got[1] <= want[1] and all(np.array_equal(sp["state"][k], dense[k]) for k in dense)


# ------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", SR.GPU_CASES)
def test_removing_half_the_views_gives_the_fusion_that_skipped_them(name):
    """The views at the even positions removed again, against a fusion with the same allocation and the same `born` that left them
    out at the fusion step.  The weights are integers and must be equal; tsdf and colour differ by the rounding of the steps.
    Largest |difference| measured with this restatement (tsdf, colour), and the largest weight:
        box/40x56/v0.10/t4/reversed   2.38e-07   -          5
        colour                        5.96e-08   5.96e-08   3
        two_rooms/v0.20               1.79e-07   -          5
        bad_pixels                    5.96e-08   -          2
        nan_pose                      5.96e-08   -          2
        many_views                    2.38e-06   -          65
        1x5x70                        5.96e-08   -          2
        one_voxel                     0          -          2
        virtual_2048                  2.38e-07   -          5
    sparse_remove_cpu.MEASURED holds the largest of each group and the gate is four times that; the figures are asserted to be
    no larger than MEASURED, so a gate cannot go stale."""
    c = SR.case(name)
    want, _ = SR.fuse(name, skip=c["counts"]["ids"][c["even"]])
    got, ref = c["half"]["state"], want["state"]
    assert np.array_equal(want["born"], c["fused"]["born"]) and want["slot_brick"] == c["fused"]["slot_brick"]
    diff = float(np.abs(got["tsdf"].astype(np.float64) - ref["tsdf"]).max())
    diff_c = float(np.abs(got["color"].astype(np.float64) - ref["color"]).max()) if got["color"] is not None else 0.0
    print(f"{name}: {len(c['even'])} of {len(c['depth'])} views removed: largest difference to the fusion without them: tsdf {diff:.3g}, colour {diff_c:.3g}; "
          f"largest weight {float(c['fused']['state']['weight'].max()):.0f}; gate {SR.gate(name):.3g}")
    assert np.array_equal(got["weight"], ref["weight"])
    assert diff <= SR.gate(name) and diff_c <= SR.gate(name)
    assert max(diff, diff_c) <= SR.MEASURED.get(name, SR.MEASURED_DEFAULT)


# ------------------------------------------------------------------------------------------------------------ (c)
def test_without_the_history_a_removal_reaches_bricks_that_never_held_the_view():
    """The box room's views fused last first: measured 4106 (voxel, view) pairs of the even positions in voxels of bricks born after
    the view; a removal that takes every allocated brick for every view leaves 1462 weight words and 1046 tsdf words different
    (71 pairs in the given order; none on colour, two_rooms/v0.20, nan_pose and bad_pixels)."""
    c = SR.case(SR.REVERSED)
    late = c["removed_even"][5]
    blind = SR.copy_volume(c["fused"])
    ev = c["even"]
    got = SR.remove(blind, c["depth"][ev], c["poses"][ev], c["K"], c["counts"]["ids"][ev], None, c["depth_max"], history=False)
    words = {k: int((blind["state"][k].view(np.uint32) != c["half"]["state"][k].view(np.uint32)).sum()) for k in ("weight", "tsdf")}
    print(f"{SR.REVERSED}: {late} pairs of the removed views lie in bricks born after them; without the history {words['weight']} weight words and "
          f"{words['tsdf']} tsdf words differ, removed {got[0]} against {c['removed_even'][0]}")
    assert late > 0 and words["weight"] > 0 and got[0] > c["removed_even"][0]


# ------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", [SR.REVERSED, "colour", "nan_pose"])
def test_born_does_not_depend_on_the_cut_into_calls(name):
    c = SR.case(name)
    want = c["fused"]
    for per in (1, 7):
        sp, counts = SR.fuse(name, views_per_call=per)
        assert np.array_equal(sp["born"], want["born"]) and sp["serial"] == want["serial"] == len(c["depth"]), per
        assert np.array_equal(counts["ids"], c["counts"]["ids"]) and counts["updates"] == c["counts"]["updates"]
        assert all(np.array_equal(sp["state"][k], want["state"][k]) for k in ("tsdf", "weight"))
    assert ((want["born"] != SR.UNBORN) == (want["table"] >= 0)).all()
    if name == "nan_pose":                                        # the lost view has an id, and no brick is born at it
        assert want["serial"] == 6 and 2 not in set(want["born"].tolist())


# ------------------------------------------------------------------------------------------------------------ (e)
def test_the_drift_route_puts_the_box_room_back_on_its_walls():
    """Wall distance of the marched vertices in voxels, measured with this restatement (vertices, faces, mean, max):
        stale       8914   17061   0.350   1.961
        corrected   8963   17176   0.041   0.500
        fresh       8963   17176   0.041   0.500"""
    d = SR.drifted()
    c = d["case"]
    _, _, lo, hi = R.box_room()
    got = {}
    for key in ("stale", "corrected", "fresh"):
        v, f, _ = S.extract_mesh(d[key])
        w = T.wall_distance(v[np.unique(f)], lo, hi) / c["voxel"]
        got[key] = (len(v), len(f), float(w.mean()), float(w.max()))
        print(f"{key}: {len(v)} vertices, {len(f)} faces, wall distance in voxels: mean {w.mean():.4f}, max {w.max():.3f}")
    assert got["stale"][2] > T.MEAN_GATE
    assert got["corrected"][2] <= T.MEAN_GATE and got["corrected"][3] <= T.MAX_GATE
    assert got["corrected"][:2] == got["fresh"][:2]
    assert d["removed"][1] == 0 and np.array_equal(d["ids"][d["odd"]], 20 + np.arange(10)) and np.array_equal(d["ids"][::2], np.arange(0, 20, 2))


# ------------------------------------------------------------------------------------------------------------ (f)
def test_no_floor_of_an_input_is_decided_by_a_last_bit():
    """sparse_cpu.marks counts, per volume, the band samples with z within 1e-12 of 0, the lattice coordinates within 1e-9 of an
    integer and those within 64 last bits of one: the first and the last must be 0 on everything the GPU test fuses, or a device
    that rounds one operation differently allocates another brick.  Measured [0, 38, 0] at most; the drift route [0, 17, 0] for the
    stale volume and [0, 38, 0] once the odd views are fused again at the true poses."""
    for name in SR.GPU_CASES:
        amb = SR.case(name)["fused"]["ambiguous"]
        print(f"{name}: {amb.tolist()}")
        assert amb[0] == 0 and amb[2] == 0, name
    d = SR.drifted()
    for key in ("stale", "corrected"):
        amb = d[key]["ambiguous"]
        print(f"drift route, {key}: {amb.tolist()}")
        assert amb[0] == 0 and amb[2] == 0, key


# ------------------------------------------------------------------------------------------------------------ (g) the C ABI
NAMES = {"mipsf_sparse_stamp", "mipsf_sparse_deintegrate"}


def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_sparse_remove.h")).read()
    declared = set(re.findall(r"\b(mipsf_sparse_[a-z0-9_]+)\s*\(", header))
    assert declared == NAMES == set(_lib.SPARSE_REMOVE_SIGNATURES)
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_SPARSE_UNBORN", _lib.SPARSE_UNBORN), ("MIPSF_SPARSE_MAX_VIEW_ID", _lib.SPARSE_MAX_VIEW_ID)):
        assert int(re.search(rf"#define {macro} (0x[0-9a-f]+|\d+)u", header).group(1), 0) == value, macro
    # two words, the volume, two pointers; the block of mipsf_sparse_integrate less max_weight plus two pointers; five uint64
    assert C.sizeof(_lib.SparseStampArgs) == 8 + 128 + 16
    assert C.sizeof(_lib.SparseDeintegrateArgs) == C.sizeof(_lib.SparseIntegrateArgs) - 8 + 16 == 248
    mine, theirs = [f[0] for f in _lib.SparseDeintegrateArgs._fields_], [f[0] for f in _lib.SparseIntegrateArgs._fields_ if f[0] != "max_weight"]
    assert mine == theirs[:-1] + ["view_ids", "born", "record"]
    assert _lib.SPARSE_REMOVE_RECORD_WORDS == 5
    assert re.search(r"uint64_t removed;.*\n\s*uint64_t missing;.*\n\s*uint64_t emptied;.*\n\s*uint64_t observed;.*\n\s*uint64_t bricks_emptied;", header)
    for unit_list in (open(os.path.join(ROOT, "mipsfusion_amd", "csrc", "Makefile")).read(), open(os.path.join(ROOT, "tools", "audit_packed.py")).read()):
        assert "sparse_remove" in unit_list
    import mipsfusion_amd
    from mipsfusion_amd import sparse_tsdf
    for name in ("SparseRemoveCounts", "SparseReintegrateCounts"):
        assert getattr(mipsfusion_amd, name) is getattr(sparse_tsdf, name)
    assert sparse_tsdf.SparseRemoveCounts._fields == ("removed", "missing", "emptied", "observed", "bricks_emptied")
    assert sparse_tsdf.SparseReintegrateCounts._fields == ("views_moved", "removed", "fused", "view_ids")


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
    if which == "stamp":
        a = dict(n=2, born=fake, serial=fake)
        cls, fn = _lib.SparseStampArgs, "mipsf_sparse_stamp"
    else:
        a = dict(n=2, H=8, W=9, fx=10.0, fy=10.0, cx=4.0, cy=4.0, trunc=0.4, depth_max=math.inf, depth=fake, poses=fake, view_ids=fake, born=fake,
                 record=fake)
        cls, fn = _lib.SparseDeintegrateArgs, "mipsf_sparse_deintegrate"
    a.update(kw)
    return cls.new(vol=_volume(**({} if vol is None else vol)), **a), fn


# of the volume: those of tests/test_sparse_cpu.py; of the views: those of mipsf_sparse_integrate less max_weight, and the two new pointers
EVERYWHERE = [(dict(X=0), "no voxels"), (dict(Z=0), "no voxels"), (dict(X=1 << 31, Y=1 << 10, Z=1 << 10), "2^31 bricks"),
              (dict(X=(1 << 14) * 8, Y=(1 << 14) * 8, Z=8 * 16), "2^31 bricks"), (dict(capacity=0), "capacity"), (dict(capacity=(1 << 20) + 1), "capacity"),
              (dict(voxel=0.0), "voxel"), (dict(voxel=math.nan), "voxel"), (dict(origin=(0.0, math.inf, 0.0)), "origin"), (dict(table=None), "null pointer"),
              (dict(count=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(birth=None), "null pointer"),
              (dict(ticks=(0x1000, None, 0x1000)), "null pointer")]
REFUSALS = [(w, v, {}, said) for w in ("stamp", "deintegrate") for v, said in EVERYWHERE] + [
    ("stamp", {}, dict(n=65536), "views"), ("stamp", {}, dict(born=None), "null pointer"), ("stamp", {}, dict(serial=None), "null pointer"),
    ("deintegrate", {}, dict(H=0), "no pixels"), ("deintegrate", {}, dict(W=0), "no pixels"), ("deintegrate", {}, dict(W=8193), "a side"),
    ("deintegrate", {}, dict(n=65536), "views"), ("deintegrate", {}, dict(fx=0.0), "intrinsics"), ("deintegrate", {}, dict(fy=math.inf), "intrinsics"),
    ("deintegrate", {}, dict(cy=math.nan), "intrinsics"), ("deintegrate", {}, dict(trunc=0.0), "trunc"), ("deintegrate", {}, dict(trunc=math.nan), "trunc"),
    ("deintegrate", {}, dict(trunc=math.inf), "trunc"), ("deintegrate", {}, dict(depth_max=math.nan), "depth_max"), ("deintegrate", {}, dict(flags=2), "flags"),
    ("deintegrate", {}, dict(rgb=0x1000), "go together"), ("deintegrate", dict(color=0x1000), {}, "go together"),
    ("deintegrate", {}, dict(depth=None), "null pointer"), ("deintegrate", {}, dict(poses=None), "null pointer"),
    ("deintegrate", {}, dict(view_ids=None), "null pointer"), ("deintegrate", {}, dict(born=None), "null pointer"),
    ("deintegrate", {}, dict(record=None), "null pointer")]


@pytest.mark.parametrize("which,vol,change,said", REFUSALS, ids=[f"{w}:{list(v or c)[0]}={list((v or c).values())[0]}" for w, v, c, _ in REFUSALS])
def test_what_is_out_of_range_is_refused_on_the_host(which, vol, change, said):
    lib = _lib.lib()
    blk, fn = _block(which, vol, **change)
    assert getattr(lib, fn)(C.byref(blk), None) != 0
    message = lib.mipsf_last_error()
    assert said.encode() in message and fn.encode() in message, message


def test_struct_sizes_and_the_python_side_are_refused_too():
    lib = _lib.lib()
    for which in ("stamp", "deintegrate"):
        blk, fn = _block(which)
        blk.struct_size -= 4
        assert getattr(lib, fn)(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
        assert getattr(lib, fn)(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
    # a volume without history, or with a finite max_weight, is refused by every route before it looks at an argument (the object
    # is made without its device state here, which none of them reaches; tests/test_gpu_sparse_remove.py asks real ones)
    from mipsfusion_amd import sparse_tsdf
    vol = object.__new__(sparse_tsdf.SparseTSDFVolume)
    vol.history, vol.max_weight = False, math.inf
    calls = (lambda: vol.deintegrate(None, None, None, None), lambda: vol.deintegrate_enqueue(None, None, None, None),
             lambda: vol.reintegrate(None, None, None, None, None), lambda: vol.reintegrate_enqueue(None, None, None, None, None))
    for call in calls + (lambda: vol.sync_views(), lambda: vol.stamp_enqueue(1)):
        with pytest.raises(ValueError, match="history"):
            call()
    vol.history, vol.max_weight = True, 2.0
    for call in calls:
        with pytest.raises(ValueError, match="max_weight"):
            call()
    # the ids: one a view, integers, of views that were fused
    vol.max_weight, vol.views_fused = math.inf, 5
    assert vol._ids([0, 4, 2], 3).tolist() == [0, 4, 2] and vol._ids(np.array([], np.int64), 0).tolist() == []
    for bad, n in (([0, 1], 3), ([0, 5, 1], 3), ([-1], 1), ([0.5], 1)):
        with pytest.raises(ValueError, match="view_ids"):
            vol._ids(bad, n)
