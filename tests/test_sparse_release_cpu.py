"""Holds the restatement of the release, the archive and the restore of bricks (tests/sparse_release_cpu.py) to its purpose, on the
cases of tests/sparse_cpu.py: a release is the dense state with the released bricks' voxels zeroed, an archive brings every word
back, a round trip does not reach a later fusion, release(empty=True) frees what deintegrate emptied, a pool smaller than the scene
survives a walk only when the bricks behind the camera are released, and a brick whose tick EQUALS a bound of the box stays.  The
GPU tests (tests/test_gpu_sparse_release.py) hold the device to this restatement word for word."""
import math

import numpy as np
import pytest

from . import sparse_cpu as S
from . import sparse_release_cpu as RL
from . import sparse_remove_cpu as SR

CASES = ("box/40x56/v0.10/t4", "two_rooms/v0.20", "colour", "1x5x70", "one_voxel", S.VIRTUAL)


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_state(a, b):
    return all((x is None and y is None) or np.array_equal(_words(x), _words(y)) for x, y in ((a[k], b[k]) for k in ("tsdf", "weight", "color")))


def _snapshot(sp):
    """a copy of the dense state (window_state may hand out the state's own arrays)"""
    return {k: (None if v is None else v.copy()) for k, v in S.window_state(sp).items()}


def _middle_box(sp):
    """a box that cuts the allocated bricks in two: everything up to the middle of their extent along the longest axis"""
    boxes = np.array([np.concatenate(RL.brick_box(sp, b)) for b in sp["slot_brick"]])
    lo, hi = boxes[:, :3].min(0), boxes[:, 3:].max(0)
    a = int(np.argmax(hi - lo))
    box = np.concatenate([lo - 1.0, hi + 1.0])
    box[3 + a] = 0.5 * (lo[a] + hi[a])
    return box


def _consistent(sp):
    """the invariant: slots 0 .. count-1, the table their inverse and -1 elsewhere"""
    t = sp["table"]
    assert len(set(sp["slot_brick"])) == len(sp["slot_brick"]) <= sp["capacity"]
    assert int((t >= 0).sum()) == len(sp["slot_brick"]) and all(t[b] == s for s, b in enumerate(sp["slot_brick"]))


# ------------------------------------------------------------------------------------------------------------ 1. a release is a mask
@pytest.mark.parametrize("name", CASES)
def test_a_release_zeroes_the_released_bricks_and_nothing_else(name):
    c = S.case(name)
    sp = RL.copy_volume(c["sp"])
    before = _snapshot(sp)
    box = _middle_box(sp)
    flags = RL.flags_of(sp, box)
    gone = [b for b, f in zip(sp["slot_brick"], flags) if f]
    kept = [b for b, f in zip(sp["slot_brick"], flags) if not f]
    rec, arch = RL.release(sp, box)
    print(f"{name}: {rec}")
    assert arch is None and rec["released"] == rec["candidates"] == len(gone) and rec["deferred"] == 0 and rec["in_use"] == len(kept)
    assert rec["released_outside"] == rec["released"] and rec["released_empty"] == 0 and rec["moved"] <= min(len(gone), len(kept))
    if name not in ("one_voxel",):
        assert 0 < len(gone) < len(gone) + len(kept), "the box must cut the bricks in two"
    _consistent(sp)
    assert sorted(sp["slot_brick"]) == sorted(kept) and all(sp["table"][b] == -1 for b in gone)
    mask = np.zeros(sp["table"].shape, bool)
    mask[np.asarray(gone, np.int64)] = True
    m = S._voxel_mask(sp, mask)
    want = {k: (None if v is None else np.where(m.reshape(m.shape + (1,) * (v.ndim - 3)), np.zeros((), v.dtype), v)) for k, v in before.items()}
    assert _same_state(S.window_state(sp), want)
    if name in ("two_rooms/v0.20", "colour"):                     # the ray cast and the mesh are sparse_cpu's over that state
        other = dict(sp, state=want)
        poses = c["poses"][:1]
        a, b = S.raycast(sp, poses, c["K"], c["H"], c["W"], color=c["rgb"] is not None), S.raycast(other, poses, c["K"], c["H"], c["W"], color=c["rgb"] is not None)
        assert np.array_equal(_words(a["depth"]), _words(b["depth"])) and np.array_equal(_words(a["normals"]), _words(b["normals"])) and a["hits"] == b["hits"]
        full = S.raycast(c["sp"], poses, c["K"], c["H"], c["W"])
        assert full["hits"] >= a["hits"]
        va, fa, _ = S.extract_mesh(sp)
        vb, fb, _ = S.extract_mesh(other)
        assert np.array_equal(va, vb) and np.array_equal(fa, fb)


# ------------------------------------------------------------------------------------------------------------ 2. the archive brings it back
@pytest.mark.parametrize("name", ("two_rooms/v0.20", "colour", "1x5x70", S.VIRTUAL))
def test_an_archive_restored_gives_back_every_word(name):
    c = S.case(name)
    sp = RL.copy_volume(c["sp"])
    before, bricks = _snapshot(sp), sorted(sp["slot_brick"])
    box = _middle_box(sp)
    rec, arch = RL.release(sp, box, archive_capacity=len(sp["slot_brick"]))
    assert rec["released"] == len(arch["bricks"]) > 0 and (arch["color"] is None) == (c["rgb"] is None) and arch["born"] is None
    assert not _same_state(S.window_state(sp), before)
    got = RL.restore(sp, arch)
    print(f"{name}: released {rec}, restored {got}")
    assert got == {"listed": rec["released"], "invalid": 0, "duplicates": 0, "occupied": 0, "restored": rec["released"], "dropped": 0, "in_use": len(bricks)}
    _consistent(sp)
    assert sorted(sp["slot_brick"]) == bricks and _same_state(S.window_state(sp), before)
    # restored again: every brick has a slot and keeps its words
    again = RL.restore(sp, arch)
    assert again["occupied"] == rec["released"] and again["restored"] == 0 and _same_state(S.window_state(sp), before)


def test_the_history_travels_with_the_archive():
    c = SR.case("two_rooms/v0.20")
    sp = SR.copy_volume(c["fused"])
    sp["state"] = {k: (None if v is None else v.copy()) for k, v in sp["state"].items()}
    born, before = sp["born"].copy(), _snapshot(sp)
    rec, arch = RL.release(sp, _middle_box(sp), archive_capacity=len(sp["slot_brick"]))
    assert rec["released"] > 0 and arch["born"] is not None and (sp["born"][arch["bricks"]] == RL.UNBORN).all() and (arch["born"] == born[arch["bricks"]]).all()
    RL.restore(sp, arch)
    assert np.array_equal(sp["born"], born) and _same_state(S.window_state(sp), before)


# ------------------------------------------------------------------------------------------------------------ 3. a round trip and later views
@pytest.mark.parametrize("name", ("two_rooms/v0.20", "colour"))
def test_fusing_on_after_a_round_trip_equals_fusing_on_without(name):
    c = S.inputs(name)
    n = len(c["depth"])
    half = n // 2
    rgb = c["rgb"]
    cap = S.case(name)["sp"]["capacity"]

    def fuse(sp, views):
        return S.integrate(sp, c["depth"][views], c["poses"][views], c["K"], None if rgb is None else rgb[views], c["depth_max"])
    lo, hi = S.window_of(name)
    plain = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], cap, rgb is not None, c["max_weight"], None, lo, hi)
    fuse(plain, slice(0, half))
    trip = RL.copy_volume(plain)
    rec, arch = RL.release(trip, _middle_box(trip), archive_capacity=cap)
    back = RL.restore(trip, arch)
    assert rec["released"] > 0 and back["restored"] == rec["released"]
    a, b = fuse(plain, slice(half, n)), fuse(trip, slice(half, n))
    assert {k: a[k] for k in ("updates", "observed", "marked", "new", "dropped", "in_use")} == {k: b[k] for k in ("updates", "observed", "marked", "new", "dropped", "in_use")}
    assert _same_state(S.window_state(plain), S.window_state(trip)) and sorted(plain["slot_brick"]) == sorted(trip["slot_brick"])
    _consistent(trip)


# ------------------------------------------------------------------------------------------------------------ 4. what deintegrate emptied
def test_release_empty_frees_exactly_the_emptied_bricks_and_they_are_born_afresh():
    name = "two_rooms/v0.20"
    c = SR.case(name)
    sp = SR.copy_volume(c["fused"])
    ids = c["counts"]["ids"]
    views = np.array([1, 3])                                      # the two views from room B: the bricks only they saw lose every view
    got = SR.remove(sp, c["depth"][views], c["poses"][views], c["K"], ids[views], None, c["depth_max"])
    emptied, in_use = got[4], len(sp["slot_brick"])
    assert 0 < emptied < in_use
    idle = [b for b in sp["slot_brick"] if not (RL.slot_words(sp, b)[1] > 0).any()]
    state = _snapshot(sp)
    rec, _ = RL.release(sp, empty=True)
    print(f"{name}: views {views.tolist()} removed, bricks_emptied {emptied} of {in_use}, release {rec}")
    assert rec["candidates"] == rec["released"] == rec["released_empty"] == emptied == len(idle) and rec["released_outside"] == 0 and rec["in_use"] == in_use - emptied
    _consistent(sp)
    assert all(sp["table"][b] == -1 and sp["born"][b] == RL.UNBORN for b in idle) and SR.bricks_emptied(sp) == 0
    assert _same_state(S.window_state(sp), state)                 # the emptied bricks held zeros already
    again = SR.integrate(sp, c["depth"][views], c["poses"][views], c["K"], None, c["depth_max"])
    assert again["new"] >= emptied and all(sp["born"][b] >= len(ids) for b in idle if sp["table"][b] >= 0)
    assert any(sp["table"][b] >= 0 for b in idle) and np.array_equal(again["ids"], len(ids) + np.arange(2))


# ------------------------------------------------------------------------------------------------------------ 5. the walk
def test_a_pool_smaller_than_the_scene_survives_the_walk_only_with_a_keep_radius():
    w = RL.walk_marks()
    print(f"{RL.WALK}, radius {RL.WALK_RADIUS} m: {w}")
    assert w["union"] == 45 and w["peak"] == 31 and w["live"] == [30, 24, 25, 31, 18, 21]
    for cap in (32, 44):                                          # peak live set <= C < union
        sp, recs = RL.walk(cap)
        assert all(r["dropped"] == 0 for r in recs) and [r["in_use"] for r in recs] == w["live"] and all(r["released"] > 0 for r in recs), (cap, recs)
        _consistent(sp)
        _, recs = RL.walk(cap, radius=None)
        assert sum(r["dropped"] for r in recs) > 0 and recs[-1]["in_use"] == cap, (cap, recs)
    assert [r["dropped"] for r in RL.walk(45, radius=None)[1]] == [0] * 6


def test_the_walk_at_a_finer_voxel():
    """the same rooms and views at 10 cm voxels: eight times the bricks per volume, the same property"""
    c = S.inputs(RL.WALK)
    voxel = 0.1
    origin = c["origin"] + 3 * c["voxel"] - 3 * voxel
    dims = [int(math.ceil((d - 1) * c["voxel"] / voxel)) + 1 for d in c["dims"]]
    probe = S.new_volume(origin, voxel, dims, 4 * voxel, 1)
    live, union, sizes = set(), set(), []
    for k in range(len(c["depth"])):
        mark, _ = S.marks(probe, c["depth"][k:k + 1], c["poses"][k:k + 1], c["K"])
        got = set(int(b) for b in np.flatnonzero(mark != S.UNMARKED))
        live |= got
        union |= got
        sizes.append(len(live))
        box = RL.keep_box(c["poses"][k].numpy(), RL.WALK_RADIUS)
        flags = RL.flags_of(dict(probe, slot_brick=sorted(live)), box)
        live = set(b for b, f in zip(sorted(live), flags) if not f)
    print(f"{RL.WALK} at {voxel} m: bricks {S.bricks_of(dims)}, union {len(union)}, live before each release {sizes}")
    assert max(sizes) < len(union)


# ------------------------------------------------------------------------------------------------------------ 6. planted ties
def test_a_bound_on_a_tick_keeps_the_brick_and_the_next_float_releases_it():
    sp0 = RL.planted((3, 3, 2), [4, 9, 13, 0, 17], 8)
    b = 9                                                         # brick (1, 1, 1)
    blo, bhi = RL.brick_box(sp0, b)
    far = np.array([-100.0, -100.0, -100.0, 100.0, 100.0, 100.0])
    for a in range(3):
        for bound, value, past in ((a, bhi[a], math.inf), (3 + a, blo[a], -math.inf)):
            box = far.copy()
            box[bound] = value                                    # lo == bhi, or hi == blo: the brick's last centre is ON the bound
            sp = RL.copy_volume(sp0)
            RL.release(sp, box)
            assert sp["table"][b] >= 0, (a, bound)
            box[bound] = np.nextafter(value, past)
            sp = RL.copy_volume(sp0)
            rec, _ = RL.release(sp, box)
            assert sp["table"][b] == -1 and rec["released"] >= 1, (a, bound)
    for k in range(6):                                            # a NaN anywhere in the box releases nothing through that bound
        box = far.copy()
        box[k] = math.nan
        sp = RL.copy_volume(sp0)
        assert RL.release(sp, box)[0]["released"] == 0
    sp = RL.copy_volume(sp0)
    assert RL.release(sp, np.full(6, math.nan))[0] == dict.fromkeys(RL.RELEASE_KEYS, 0) | {"in_use": 5}


# ------------------------------------------------------------------------------------------------------------ 7. the rule, literally
def test_the_swap_fill_the_cap_and_the_restore_s_marks():
    order = [7, 3, 11, 0, 5, 9, 2, 10]
    sp0 = RL.planted((2, 3, 2), order, 10, color=True, history=True, empty=(1, 6, 7))
    # EMPTY alone: slots 1, 6, 7 go; n' = 5; hole 1 takes the one tail survivor, slot 5
    sp = RL.copy_volume(sp0)
    rec, arch = RL.release(sp, empty=True, archive_capacity=8)
    assert rec == {"candidates": 3, "released": 3, "released_outside": 0, "released_empty": 3, "deferred": 0, "moved": 1, "in_use": 5}
    assert sp["slot_brick"] == [7, 9, 11, 0, 5] and arch["bricks"].tolist() == [3, 2, 10] and arch["born"].tolist() == [6, 11, 12]
    assert (arch["tsdf"][1] == -1.0).all() and (arch["tsdf"][0] == 0.0).all() and (arch["weight"] == 0).all()
    _consistent(sp)
    # the cap: one entry only, the first candidate in slot order; the others are deferred
    sp = RL.copy_volume(sp0)
    rec, arch = RL.release(sp, empty=True, archive_capacity=1)
    assert (rec["released"], rec["deferred"], rec["moved"]) == (1, 2, 1) and sp["slot_brick"] == [7, 10, 11, 0, 5, 9, 2] and arch["bricks"].tolist() == [3]
    sp = RL.copy_volume(sp0)
    rec, arch = RL.release(sp, empty=True, archive_capacity=0)
    assert (rec["released"], rec["deferred"]) == (0, 3) and sp["slot_brick"] == order and len(arch["bricks"]) == 0
    # restore: the lowest entry wins a duplicate, an entry out of range is invalid, an occupied brick keeps its words, the pool ends
    sp = RL.copy_volume(sp0)
    rec, arch = RL.release(sp, np.array([-9.0, -9.0, -9.0, 9.0, 9.0, 9.0]), empty=True, archive_capacity=8)
    twice = RL.cat([arch, arch])
    twice["tsdf"][3:] += 1.0
    twice["bricks"][4] = 12                                       # beyond the 12 bricks of the grid
    twice["bricks"] = np.concatenate([twice["bricks"], [7]])      # a brick that has a slot
    for k in ("born", "tsdf", "weight", "color"):
        twice[k] = np.concatenate([twice[k], twice[k][:1]])
    got = RL.restore(sp, twice)
    assert got == {"listed": 7, "invalid": 1, "duplicates": 2, "occupied": 1, "restored": 3, "dropped": 0, "in_use": 8}
    assert sp["slot_brick"][5:] == [2, 3, 10] and (RL.slot_words(sp, 3)[0] == 0.0).all() and (RL.slot_words(sp, 2)[0] == -1.0).all()
    small = RL.copy_volume(sp0)
    small["capacity"] = 6
    RL.release(small, empty=True)
    got = RL.restore(small, arch)
    assert (got["restored"], got["dropped"], got["in_use"]) == (1, 2, 6) and small["slot_brick"][5] == 2
    assert RL.restore(sp, arch, 0) == dict.fromkeys(RL.RESTORE_KEYS, 0)


def test_the_module_says_why_nothing_is_ambiguous_and_the_package_has_the_names():
    assert "no tolerance" in RL.__doc__ and "last bit" in RL.__doc__
    import mipsfusion_amd
    for name in ("ReleaseCounts", "RestoreCounts", "BrickArchive"):
        assert hasattr(mipsfusion_amd, name)
    from mipsfusion_amd import sparse_tsdf
    assert tuple(sparse_tsdf.ReleaseCounts._fields[:6]) == RL.RELEASE_KEYS[:6] and tuple(sparse_tsdf.RestoreCounts._fields[:6]) == RL.RESTORE_KEYS[:6]
    for name in ("release", "release_enqueue", "restore", "restore_enqueue"):
        assert callable(getattr(sparse_tsdf.SparseTSDFVolume, name))
    assert "keep_radius" in sparse_tsdf.sparse_tsdf_odometry.__doc__
