"""GPU tests of the release, the archive and the restore of bricks of the brick-sparse volume (mipsfusion_amd/sparse_tsdf.py release,
restore, BrickArchive, sparse_tsdf_odometry(keep_radius=...); csrc/sparse_release.hip) against the restatement of
tests/sparse_release_cpu.py.  Nothing is computed on either side -- stored words are compared and copied -- so the table, the slot
order, the count, born, every word of all `capacity` slots of the pool (the zeroed tail too), the archive's entries and both
records are compared for EQUALITY, with no tolerance.  The pool, the per-slot arrays, the archive and the records sit between guard
words.  tests/test_sparse_release_cpu.py holds the restatement to its purpose."""
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, sparse_tsdf

from . import sparse_cpu as S
from . import sparse_mesh_cpu as B
from . import sparse_release_cpu as RL
from . import sparse_remove_cpu as SR

pytestmark = pytest.mark.gpu

FAR = np.array([-1e3, -1e3, -1e3, 1e3, 1e3, 1e3])                # a box that holds every brick
AWAY = np.array([1e3, 1e3, 1e3, 2e3, 2e3, 2e3])                  # a box that holds none
GUARD = 2                                                         # guard slots behind the pool, guard entries around the archive


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _u32(a):
    return np.asarray(a.cpu().numpy() if torch.is_tensor(a) else a).astype(np.int64) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------- guards
_FILLS = (("tsdf", 7.0), ("weight", 7.0), ("color", 7.0), ("slot_brick", -77), ("_birth", -77), ("born", -77))


def _guard(vol):
    """the pool and the per-slot arrays GUARD slots longer, the guard slots full of a sentinel -> the long tensors"""
    long = {}
    for key, fill in _FILLS:
        old = getattr(vol, key)
        if old is None:
            continue
        new = torch.full((vol.capacity + GUARD,) + tuple(old.shape[1:]), fill, dtype=old.dtype, device=old.device)
        new[:vol.capacity] = old
        long[key] = new
        setattr(vol, key, new[:vol.capacity])
    vol._bind()
    return long


def _guards_hold(vol, long):
    return [key for key, fill in _FILLS if key in long and not bool((long[key][vol.capacity:] == fill).all())]


class _Archive:
    """a BrickArchive of `cap` entries of the test's own, GUARD sentinel entries on either side"""

    def __init__(self, vol, cap):
        self.cap = cap
        n = cap + 2 * GUARD
        dev = vol.device
        self.long = {"bricks": torch.full((n,), -77, dtype=torch.int32, device=dev),
                     "born": torch.full((n,), -77, dtype=torch.int32, device=dev) if vol.history else None,
                     "tsdf": torch.full((n,) + sparse_tsdf.BRICK, 7.0, device=dev), "weight": torch.full((n,) + sparse_tsdf.BRICK, 7.0, device=dev),
                     "color": torch.full((n,) + sparse_tsdf.BRICK + (3,), 7.0, device=dev) if vol.color is not None else None}
        cut = {k: (None if v is None else v[GUARD:GUARD + cap]) for k, v in self.long.items()}
        self.archive = sparse_tsdf.BrickArchive(cut["bricks"], cut["born"], cut["tsdf"], cut["weight"], cut["color"])

    def differs(self, want):
        """the entries written against the restatement's; everything else still the sentinel -> what differs"""
        out, n = [], len(want["bricks"])
        a = self.archive
        if not np.array_equal(a.bricks[:n].cpu().numpy(), want["bricks"]):
            out.append("archive bricks")
        if a.born is not None and not np.array_equal(_u32(a.born[:n]), _u32(want["born"])):
            out.append("archive born")
        for key in ("tsdf", "weight", "color"):
            if getattr(a, key) is not None and not np.array_equal(_words(getattr(a, key)[:n]), _words(want[key])):
                out.append(f"archive {key}")
        for key, v in self.long.items():
            if v is None:
                continue
            rest = torch.cat([v[:GUARD], v[GUARD + n:]])
            if not bool((rest == (-77 if v.dtype == torch.int32 else 7.0)).all()):
                out.append(f"archive {key} beyond the entries written")
        return out


def _record(dev, words=7):
    long = torch.full((words + 2,), -77, dtype=torch.int64, device=dev)
    return long, long[1:1 + words]


# ------------------------------------------------------------------------------------------------------------- device <-> restatement
def _to_device(sp, dev):
    """the restatement's volume written into a SparseTSDFVolume, guarded -> (vol, guards)"""
    st = sp["state"]
    vol = sparse_tsdf.SparseTSDFVolume(sp["origin"], sp["voxel"], sp["dims"], sp["trunc"], sp["capacity"], color=st["color"] is not None,
                                       max_weight=sp["max_weight"], device=dev, history="born" in sp)
    p = RL.pool(sp)
    n = len(sp["slot_brick"])
    vol.table.copy_(torch.from_numpy(S.table_of(sp)))
    vol.slot_brick[:n] = torch.tensor(sp["slot_brick"], dtype=torch.int32)
    vol.count.fill_(n)
    vol.tsdf.copy_(torch.from_numpy(p["tsdf"]))
    vol.weight.copy_(torch.from_numpy(p["weight"]))
    if vol.color is not None:
        vol.color.copy_(torch.from_numpy(p["color"]))
    if vol.history:
        vol.born.copy_(torch.from_numpy(p["born"].astype(np.int32)))
        vol.serial.fill_(sp["serial"])
        vol.views_fused = sp["serial"]
    vol.bricks_in_use = n
    return vol, _guard(vol)


def _differs(vol, sp):
    """table, slot order, count, born and EVERY word of all `capacity` slots against the restatement's -> what differs"""
    out = []
    n = int(vol.count.item())
    if n != len(sp["slot_brick"]):
        out.append(f"count {n} != {len(sp['slot_brick'])}")
    if vol.slot_brick[:len(sp["slot_brick"])].cpu().tolist() != sp["slot_brick"]:
        out.append("slot order")
    if not np.array_equal(vol.table.cpu().numpy(), S.table_of(sp)):
        out.append("table")
    p = RL.pool(sp)
    if vol.history and not np.array_equal(_u32(vol.born), _u32(p["born"])):
        out.append("born")
    for key in ("tsdf", "weight", "color"):
        if getattr(vol, key) is not None:
            bad = int((_words(getattr(vol, key)) != _words(p[key])).sum())
            if bad:
                out.append(f"{key}: {bad} words")
    return out


def _box(box, dev):
    return None if box is None else torch.from_numpy(np.asarray(box, np.float64).reshape(6)).to(dev)


def _release_both(vol, sp, dev, box=None, empty=False, cap=None, guards=None):
    """release_enqueue on the device and the restatement's release, with a guarded record and archive; asserts the record, the archive,
    the state and the guards -> (record dict, the test's archive or None, the restatement's archive)"""
    long_rec, rec = _record(dev)
    mine = None if cap is None else _Archive(vol, cap)
    got = vol.release_enqueue(_box(box, dev), empty, None, rec, None if mine is None else mine.archive)
    want, want_arch = RL.release(sp, box, empty, cap)
    rec_got = dict(zip(RL.RELEASE_KEYS, rec.tolist()))
    assert (got is rec) if mine is None else (got[0] is rec and got[1] is mine.archive)
    assert rec_got == want, (rec_got, want)
    assert long_rec[0].item() == -77 and long_rec[-1].item() == -77
    assert _differs(vol, sp) == []
    if mine is not None:
        assert mine.differs(want_arch) == []
    if guards is not None:
        assert _guards_hold(vol, guards) == []
    return want, mine, want_arch


def _restore_both(vol, sp, dev, archive, want_arch, m=None, guards=None):
    long_rec, rec = _record(dev)
    got = vol.restore_enqueue(archive if m is None else archive.first(m), rec)
    want = RL.restore(sp, want_arch, m)
    rec_got = dict(zip(RL.RESTORE_KEYS, rec.tolist()))
    assert got is rec and rec_got == want, (rec_got, want)
    assert long_rec[0].item() == -77 and long_rec[-1].item() == -77
    assert _differs(vol, sp) == []
    if guards is not None:
        assert _guards_hold(vol, guards) == []
    return want


def _from_cpu(want_arch, dev):
    """the restatement's archive as a BrickArchive on the device"""
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)      # noqa: E731
    return sparse_tsdf.BrickArchive(t(want_arch["bricks"], np.int32), t(want_arch["born"], np.int32), t(want_arch["tsdf"], np.float32),
                                    t(want_arch["weight"], np.float32), t(want_arch["color"], np.float32), n=len(want_arch["bricks"]))


# ------------------------------------------------------------------------------------------------------------- 1. the shapes of a release
ORDER = [7, 3, 11, 0, 5, 9, 2, 10, 17, 20]                        # ten bricks of a grid of 4 x 3 x 2, in slot order
SHAPES = {                                                        # name: (capacity, slots without an observed voxel, box, empty, archive entries)
    "nothing released": (12, (), FAR, True, None),
    "everything released": (12, (), AWAY, False, None),
    "everything released into an archive": (12, (), AWAY, True, 10),
    "the tail only, no move": (12, (7, 8, 9), None, True, None),
    "below n' only, every tail slot survives": (12, (0, 1, 2), None, True, 3),
    "one hole and one tail survivor": (12, (2, 9), None, True, None),
    "count == capacity": (10, (0, 4, 9), None, True, 10),
    "an archive of no entries": (12, (1, 6, 7), None, True, 0),
    "an archive of one entry": (12, (1, 6, 7), None, True, 1),
    "an archive of candidates - 1 entries": (12, (1, 3, 6, 7), None, True, 3),
    "both predicates, a slot in both": (12, (1, 2), np.array([-1e3, -1e3, -1e3, 1e3, 1.5, 1e3]), True, 10),
    "a NaN box": (12, (1,), np.full(6, math.nan), False, 4),
    "a NaN in one bound": (12, (1,), np.array([-1e3, math.nan, -1e3, 1e3, 1e3, 1e3]), False, None),
}


@pytest.mark.parametrize("color,history", [(False, False), (True, False), (False, True), (True, True)])
def test_the_shapes_of_a_release_equal_the_restatement(dev, color, history):
    for name, (capacity, idle, box, empty, cap) in SHAPES.items():
        sp = RL.planted((4, 3, 2), ORDER, capacity, color, history, seed=len(name), empty=idle)
        vol, guards = _to_device(sp, dev)
        assert _differs(vol, sp) == [], name
        want, mine, want_arch = _release_both(vol, sp, dev, box, empty, cap, guards)
        print(f"colour {color}, history {history}, {name}: {want}")
        if name == "both predicates, a slot in both":
            assert want["released_outside"] + want["released_empty"] > want["released"] > 0
        if name == "an archive of candidates - 1 entries":
            assert want["deferred"] == 1 and want["released"] == 3
        if "NaN" in name:
            assert want["released"] == 0
        if name.startswith("everything"):
            assert want["in_use"] == 0 and not vol.weight.any() and bool((vol.table == -1).all())
        if mine is not None and want["released"]:                 # and back again: the archive restored into the same volume
            back = _restore_both(vol, sp, dev, mine.archive, want_arch, want["released"], guards)
            assert back["restored"] == want["released"] and back["dropped"] == 0, name
            assert mine.differs(want_arch) == [], name            # a restore only reads the archive
    # count = 0: a fresh volume
    sp = RL.planted((4, 3, 2), [], 4, color, history)
    vol, guards = _to_device(sp, dev)
    for box, empty, cap in ((AWAY, True, None), (FAR, False, 2)):
        want, _, _ = _release_both(vol, sp, dev, box, empty, cap, guards)
        assert want == dict.fromkeys(RL.RELEASE_KEYS, 0)


# ------------------------------------------------------------------------------------------------------------- 2. the shapes of a restore
@pytest.mark.parametrize("color,history", [(False, False), (True, True)])
def test_the_shapes_of_a_restore_equal_the_restatement(dev, color, history):
    sp0 = RL.planted((4, 3, 2), ORDER, 12, color, history, seed=3, empty=(1, 6))
    sp = RL.copy_volume(sp0)
    vol, guards = _to_device(sp, dev)
    box = np.array([-1e3, -1e3, -1e3, 1e3, 1.5, 1e3])
    want, mine, arch = _release_both(vol, sp, dev, box, True, 10, guards)
    n = want["released"]
    assert n >= 4
    arch = {k: (None if v is None else v.copy()) for k, v in arch.items()}
    # m = 0: a zero record and nothing moves
    assert _restore_both(vol, sp, dev, mine.archive, arch, 0, guards) == dict.fromkeys(RL.RESTORE_KEYS, 0)
    # duplicates with other words (the lowest entry wins), a brick out of range on either side, an occupied brick, descending bricks
    twice = RL.cat([arch, arch])
    twice["tsdf"][n:] += 1.0
    twice["weight"][n:] += 1.0
    twice["bricks"][n + 1] = 24                                   # the grid has 24 bricks
    twice["bricks"][n + 2] = -5
    extra = {k: (None if v is None else v[:1].copy()) for k, v in arch.items()}
    extra["bricks"][0] = sp["slot_brick"][0]                      # a brick that has a slot
    extra["tsdf"] += 3.0
    twice = RL.cat([twice, extra])
    order = np.argsort(-twice["bricks"], kind="stable")           # descending brick order; duplicates keep their order
    twice = {k: (None if v is None else v[order]) for k, v in twice.items()}
    got = _restore_both(vol, sp, dev, _from_cpu(twice, dev), twice, None, guards)
    print(f"colour {color}, history {history}: restore {got}")
    assert (got["listed"], got["invalid"], got["duplicates"], got["occupied"], got["restored"], got["dropped"]) == (2 * n + 1, 2, n - 2, 1, n, 0)
    assert sorted(sp["slot_brick"]) == sorted(sp0["slot_brick"])
    # a pool that fills half way through: the first bricks in brick order get the slots that are left
    small = RL.copy_volume(sp0)
    small["capacity"] = len(ORDER) - n + 2
    RL.release(small, box, True)
    vol, guards = _to_device(small, dev)
    got = _restore_both(vol, small, dev, _from_cpu(arch, dev), arch, None, guards)
    assert (got["restored"], got["dropped"], got["in_use"]) == (2, n - 2, small["capacity"])
    # every call repeats: the same archive again finds every brick it restored occupied and changes no word
    again = _restore_both(vol, small, dev, _from_cpu(arch, dev), arch, None, guards)
    assert (again["occupied"], again["restored"], again["dropped"]) == (2, 0, n - 2)


# ------------------------------------------------------------------------------------------------------------- 3. pools past a tile
@pytest.mark.parametrize("in_use,capacity", [(1100, 1100), (2100, 2304)])
def test_a_pool_past_the_scan_s_tile_and_its_top_level(dev, in_use, capacity):
    """more than 1024 and more than 2048 slots in use: the candidates' prefix sum crosses its tile and sums several tiles"""
    assert in_use > (1 if in_use < 2048 else 2) * _lib.SPARSE_SCAN_TILE
    grid = (13, 13, 13)
    rng = np.random.default_rng(in_use)
    order = rng.permutation(13 ** 3)[:in_use].tolist()
    idle = tuple(int(s) for s in rng.choice(in_use, in_use // 5, replace=False))
    sp = RL.planted(grid, order, capacity, history=True, seed=1, empty=idle)
    vol, guards = _to_device(sp, dev)
    box = np.array([-1e3, -1e3, -1e3, 7.9, 1e3, 1e3])             # bricks 0 .. 7 of 13 along x stay (a brick is 1 m wide there)
    candidates = int((RL.flags_of(sp, box, True) != 0).sum())
    want, mine, arch = _release_both(vol, sp, dev, box, True, candidates - 1, guards)
    print(f"{in_use} slots of {capacity}: {want}")
    assert want["candidates"] == candidates > _lib.SPARSE_SCAN_TILE // 2 and want["deferred"] == 1 and want["moved"] > 0
    assert want["released_outside"] > 0 and want["released_empty"] > 0
    back = _restore_both(vol, sp, dev, mine.archive, arch, want["released"], guards)
    assert back["restored"] == want["released"] and back["in_use"] == in_use
    rest, _, _ = _release_both(vol, sp, dev, AWAY, False, None, guards)          # and everything goes
    assert rest["released"] == in_use and rest["in_use"] == 0 and not vol.weight.any() and not vol.tsdf.any() and bool((vol.born == -1).all())


# ------------------------------------------------------------------------------------------------------------- 4. fused volumes
def _fused(name, dev, views, history):
    c = (SR if history else S).inputs(name)
    lo, hi = S.window_of(name)
    cap = S.case(name)["sp"]["capacity"]
    make = SR.new_volume if history else S.new_volume
    sp = make(c["origin"], c["voxel"], c["dims"], c["trunc"], cap, c["rgb"] is not None, c["max_weight"], None, lo, hi)
    vol = sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], cap, color=c["rgb"] is not None, max_weight=c["max_weight"], device=dev,
                                       history=history)
    guards = _guard(vol)
    return c, sp, vol, guards


def _fuse_both(c, sp, vol, views, history):
    rgb = None if c["rgb"] is None else c["rgb"][views]
    got = vol.integrate(c["depth"][views], c["poses"][views], c["K"], rgb, c["depth_max"])
    want = (SR if history else S).integrate(sp, c["depth"][views], c["poses"][views], c["K"], rgb, c["depth_max"])
    assert tuple(got) == tuple(want[k] for k in ("updates", "observed", "marked", "new", "dropped", "in_use")), (tuple(got), want)
    assert vol.bricks_in_use == len(sp["slot_brick"])
    return got


def _middle_box(sp):
    boxes = np.array([np.concatenate(RL.brick_box(sp, b)) for b in sp["slot_brick"]])
    lo, hi = boxes[:, :3].min(0), boxes[:, 3:].max(0)
    a = int(np.argmax(hi - lo))
    box = np.concatenate([lo - 1.0, hi + 1.0])
    box[3 + a] = 0.5 * (lo[a] + hi[a])
    return box


def _consumers_equal(name, c, sp, vol, mesh=True):
    """to_dense, the ray cast and the mesh marched brick by brick against the restatement's, word for word"""
    d = vol.to_dense(sp["lo"], sp["hi"])
    st = sp["state"]
    assert np.array_equal(_words(d.tsdf), _words(st["tsdf"])) and np.array_equal(_words(d.weight), _words(st["weight"])), name
    assert st["color"] is None or np.array_equal(_words(d.color), _words(st["color"])), name
    pose = c["poses"][:1]
    far = 10.0 if c["dims"] == S.VIRTUAL_DIMS else math.inf
    color = c["rgb"] is not None
    ref = S.raycast(sp, pose, c["K"], c["H"], c["W"], far=far, color=color)
    got = vol.raycast_enqueue(pose.to(vol.device).contiguous(), c["K"], c["H"], c["W"], far=far, color=color)
    assert np.array_equal(_words(got.depth), _words(ref["depth"])) and np.array_equal(_words(got.normals), _words(ref["normals"])), name
    assert got.hits.tolist() == [ref["hits"], 0] and (not color or np.array_equal(_words(got.color), _words(ref["color"]))), name
    if mesh:
        want = B.mesh(sp)
        m = vol.extract_mesh_bricks()
        assert np.array_equal(m.faces, want["faces"]) and np.array_equal(np.ascontiguousarray(m.vertices).view(np.uint64), np.ascontiguousarray(want["vertices"]).view(np.uint64)), name
        assert (want["colors"] is None and m.vertex_colors is None) or np.array_equal(_words(m.vertex_colors), _words(want["colors"])), name
    assert sorted(map(tuple, vol.allocated_bricks().tolist())) == sorted(RL.coords(sp, b) for b in sp["slot_brick"])
    if sp["slot_brick"]:
        assert vol.tight_window() == S.tight_window(sp), name
    else:
        assert vol.tight_window() is None


@pytest.mark.parametrize("name,history", [("two_rooms/v0.20", True), ("colour", True), ("1x5x70", False), ("one_voxel", False), (S.VIRTUAL, False),
                                          ("max_weight_2", False)])
def test_fused_volumes_released_and_restored_equal_the_restatement(dev, name, history):
    """half the views fused, the bricks beyond the middle released into an archive (public release: one read-back, the host's
    mirrors), the consumers, the other half fused on top (released bricks are born afresh), the archive restored (the bricks that
    came back meanwhile keep their words), with a history the second half removed again -- the restatement's words at every step"""
    n = len((SR if history else S).inputs(name)["depth"])
    first, second = slice(0, n // 2), slice(n // 2, n)
    c, sp, vol, guards = _fused(name, dev, first, history)
    _fuse_both(c, sp, vol, first, history)
    assert _differs(vol, sp) == [], name
    box = _middle_box(sp)
    in_use = len(sp["slot_brick"])
    counts, arch = vol.release(np.stack([box[:3], box[3:]], 1), archive=True)
    want, want_arch = RL.release(sp, box, archive_capacity=in_use)
    print(f"{name}: {in_use} bricks, release {tuple(counts)}")
    assert isinstance(counts, sparse_tsdf.ReleaseCounts) and isinstance(arch, sparse_tsdf.BrickArchive) and tuple(counts) == tuple(want[k] for k in RL.RELEASE_KEYS)
    assert arch.n == len(arch) == want["released"] and vol.bricks_in_use == want["in_use"] and (name == "one_voxel" or want["released"] > 0)
    assert _differs(vol, sp) == [] and _guards_hold(vol, guards) == [], name
    assert np.array_equal(arch.bricks.cpu().numpy(), want_arch["bricks"]) and np.array_equal(_words(arch.tsdf), _words(want_arch["tsdf"]))
    assert np.array_equal(_words(arch.weight), _words(want_arch["weight"])) and (arch.color is None or np.array_equal(_words(arch.color), _words(want_arch["color"])))
    assert arch.born is None or np.array_equal(_u32(arch.born), _u32(want_arch["born"]))
    _consumers_equal(name, c, sp, vol, mesh=name in B.CASES)
    _fuse_both(c, sp, vol, second, history)
    assert _differs(vol, sp) == [], name
    host = sparse_tsdf.BrickArchive.cat([arch.cpu()])             # by way of the host, and through cat
    got = vol.restore(host)
    back = RL.restore(sp, want_arch)
    print(f"{name}: restore {tuple(got)}")
    assert isinstance(got, sparse_tsdf.RestoreCounts) and tuple(got) == tuple(back[k] for k in RL.RESTORE_KEYS) and vol.bricks_in_use == len(sp["slot_brick"])
    assert got.restored + got.occupied == want["released"] and _differs(vol, sp) == [] and _guards_hold(vol, guards) == [], name
    _consumers_equal(name, c, sp, vol, mesh=name in B.CASES and name != S.VIRTUAL)
    if history:
        ids = vol.last_view_ids
        rgb = None if c["rgb"] is None else c["rgb"][second]
        gone = vol.deintegrate(c["depth"][second], c["poses"][second], c["K"], ids, rgb, c["depth_max"])
        ref = SR.remove(sp, c["depth"][second], c["poses"][second], c["K"], ids, rgb, c["depth_max"])
        assert tuple(gone) == ref[:5] and _differs(vol, sp) == [], name
        idle, _ = RL.release(sp, empty=True)
        freed = vol.release(empty=True)
        assert tuple(freed) == tuple(idle[k] for k in RL.RELEASE_KEYS) and freed.released == gone.bricks_emptied and _differs(vol, sp) == [], name
        _fuse_both(c, sp, vol, second, history)                   # and they are born afresh
        assert _differs(vol, sp) == [] and _guards_hold(vol, guards) == [], name


# ------------------------------------------------------------------------------------------------------------- 5. repeats, graphs
def test_every_call_repeats_bit_for_bit_and_replays_from_a_graph(dev):
    """the same release and the same restore on the same state give the same bytes, eagerly and replayed from a captured graph
    (GPU_MAX_HW_QUEUES as the machine sets it)"""
    sp0 = RL.planted((13, 13, 13), np.random.default_rng(5).permutation(13 ** 3)[:1500].tolist(), 1600, color=True, history=True, seed=2, empty=tuple(range(0, 1500, 7)))
    box = _box(np.array([-1e3, -1e3, -1e3, 1e3, 6.9, 1e3]), dev)
    vol, guards = _to_device(RL.copy_volume(sp0), dev)
    keep = [t.clone() for t in (vol.table, vol.slot_brick, vol.count, vol.born, vol.tsdf, vol.weight, vol.color)]

    def reset():
        for t, k in zip((vol.table, vol.slot_brick, vol.count, vol.born, vol.tsdf, vol.weight, vol.color), keep):
            t.copy_(k)

    def snap(extra):
        return [t.clone() for t in (vol.table, vol.slot_brick, vol.count, vol.born, vol.tsdf, vol.weight, vol.color) + tuple(extra)]

    def same(a, b):
        return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
    mine = _Archive(vol, 1000)
    rec, rec2 = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(7, dtype=torch.int64, device=dev)
    arch = mine.archive

    def round_trip():
        vol.release_enqueue(box, True, None, rec, arch)
        vol.restore_enqueue(arch, rec2)
    round_trip()
    torch.cuda.synchronize()
    first = snap((rec, rec2, arch.bricks, arch.born, arch.tsdf, arch.weight, arch.color))
    sp = RL.copy_volume(sp0)
    want, want_arch = RL.release(sp, box.cpu().numpy(), True, 1000)
    back = RL.restore(sp, {k: (None if v is None else np.concatenate([v, np.zeros((1000 - len(v),) + v.shape[1:], v.dtype) - (1 if k == "bricks" else 0)]))
                           for k, v in want_arch.items()})
    assert rec.tolist() == [want[k] for k in RL.RELEASE_KEYS] and rec2.tolist() == [back[k] for k in RL.RESTORE_KEYS] and want["deferred"] == 0
    assert _differs(vol, sp) == [] and back["invalid"] == 1000 - want["released"] and back["restored"] == want["released"] > 0
    for _ in range(2):
        reset()
        round_trip()
        torch.cuda.synchronize()
        assert same(first, snap((rec, rec2, arch.bricks, arch.born, arch.tsdf, arch.weight, arch.color)))
    reset()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        round_trip()
    for _ in range(2):
        reset()
        rec.zero_(), rec2.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same(first, snap((rec, rec2, arch.bricks, arch.born, arch.tsdf, arch.weight, arch.color)))
    assert _guards_hold(vol, guards) == []


# ------------------------------------------------------------------------------------------------------------- 6. the walk
def test_a_pool_smaller_than_the_scene_survives_the_walk_with_a_keep_radius(dev):
    """the walk of tests/test_sparse_release_cpu.py at its poses: 32 slots for a scene of 45 bricks"""
    c = S.inputs(RL.WALK)
    cap = 32
    w = RL.walk_marks()
    assert w["peak"] <= cap < w["union"]
    for radius in (RL.WALK_RADIUS, None):
        sp, want = RL.walk(cap, radius)
        vol = sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], cap, device=dev)
        guards = _guard(vol)
        got = []
        for k in range(len(c["depth"])):
            counts = vol.integrate(c["depth"][k:k + 1], c["poses"][k:k + 1], c["K"], None, c["depth_max"])
            rec = {"dropped": counts.dropped, "in_use": counts.bricks_in_use, "released": 0}
            if radius is not None:
                t = c["poses"][k][:3, 3].to(torch.float64).numpy()
                rec["released"] = vol.release(np.stack([t - radius, t + radius], 1)).released
            got.append(rec)
        print(f"radius {radius}: {got}")
        assert got == want and _differs(vol, sp) == [] and _guards_hold(vol, guards) == []
        assert (sum(r["dropped"] for r in got) == 0) == (radius is not None)


def test_odometry_with_a_keep_radius_equals_the_restatement_fed_with_the_device_s_poses(dev):
    """sparse_tsdf_odometry(keep_radius=...) over the walk's six frames in 32 slots: no call drops a brick, and frame by frame the
    pose is the restatement's registration against the restatement's volume -- fused and released at the device's poses -- and the
    volume at the end is the restatement's.  (The six views lie metres apart, so the registration finds few pairs and the poses
    wander; what is held here is the sequence fuse, release around the pose found, on the device, not the tracking.)  With a
    threshold on the pairs the frames that fall below it are lost: they are fused at a NaN pose, and the NaN box releases nothing."""
    c = S.inputs(RL.WALK)
    K, H, W, n, cap, r = c["K"], c["H"], c["W"], len(c["depth"]), 32, RL.WALK_RADIUS
    bounds = np.stack([c["origin"], c["origin"] + c["voxel"] * (np.asarray(c["dims"]) - 1.5)], 1)
    for least in (0, 50):
        poses, records, vol = sparse_tsdf.sparse_tsdf_odometry(torch.from_numpy(c["depth"]).to(dev), K, c["poses"][0], c["voxel"], bounds, cap, c["trunc"],
                                                               min_correspondences=least, keep_radius=r)
        assert vol.dims == tuple(c["dims"]) and np.array_equal(vol.origin, c["origin"])
        poses = poses.numpy()
        sp = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], cap)
        released = []
        for k in range(n):
            lost = False
            if k:
                want = RL.odometry_step(sp, poses[k - 1], c["depth"][k], K, H, W)
                got, amb = records[k], sum(want["ambiguous_per_eval"])
                Tg = got["transformation"].numpy()
                print(f"least {least}, frame {k}: pairs {got['n_correspondences']} {want['n']}, iterations {got['iterations']} {want['iterations']}, ambiguous {amb}, "
                      f"lost {got['lost']}, dropped {got['dropped']}, released {got['released']}")
                assert abs(got["n_correspondences"] - want["n"]) <= amb
                if amb == 0:
                    assert got["iterations"] == want["iterations"] and np.abs(Tg - want["transformation"]).max() < 1e-9
                lost = got["lost"]
                assert lost == (got["n_correspondences"] < least) and np.array_equal(poses[k], poses[k - 1] if lost else Tg.astype(np.float32))
            if not lost:
                assert S.integrate(sp, c["depth"][k:k + 1], poses[k:k + 1], K)["dropped"] == 0
                released.append(RL.release(sp, RL.keep_box(poses[k], r))[0]["released"])
            else:
                released.append(0)
            assert records[k]["dropped"] == 0 and records[k]["released"] == released[-1], k
        assert records[-1]["released_total"] == sum(released) > 0 and records[-1]["bricks_in_use"] == len(sp["slot_brick"]) == vol.bricks_in_use
        assert _differs(vol, sp) == []
        if least:
            assert any(rec["lost"] for rec in records)
    # without the argument: the launches and the records of before
    plain = sparse_tsdf.sparse_tsdf_odometry(c["depth"][:2], K, c["poses"][0], c["voxel"], bounds, cap, c["trunc"], device=dev)[1]
    assert "released" not in plain[-1] and "dropped" in plain[-1] and "dropped" not in plain[0]


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_carry_their_messages_and_change_no_word(dev):
    sp = RL.planted((4, 3, 2), ORDER, 12, True, True, seed=9, empty=(1,))
    vol, guards = _to_device(sp, dev)
    box = _box(FAR, dev)
    with pytest.raises(ValueError, match="box"):
        vol.release()
    with pytest.raises(ValueError, match="box"):
        vol.release_enqueue(box.float())
    with pytest.raises(ValueError, match="keep_box"):
        vol.release(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="archive_capacity"):
        vol.release_enqueue(box, archive_capacity=-1)
    plain_arch = sparse_tsdf.BrickArchive.empty(4, False, False, dev)
    with pytest.raises(ValueError, match="into"):
        vol.release_enqueue(box, into=plain_arch)
    with pytest.raises(ValueError, match="born"):
        vol.restore(sparse_tsdf.BrickArchive.empty(4, True, False, dev))
    with pytest.raises(ValueError, match="color"):
        vol.restore(sparse_tsdf.BrickArchive.empty(4, False, True, dev))
    with pytest.raises(ValueError, match="BrickArchive"):
        vol.restore([1, 2])
    with pytest.raises(ValueError, match="cat"):
        sparse_tsdf.BrickArchive.cat([plain_arch, sparse_tsdf.BrickArchive.empty(4, True, True, dev)])
    # the C ABI: flags, the box, the archive's arrays, the scratch
    import ctypes as C
    lib = _lib.lib()
    rec = torch.zeros(7, dtype=torch.int64, device=dev)
    scratch = torch.zeros(int(lib.mipsf_sparse_release_scratch_words(vol.capacity)) // 2 + 2, dtype=torch.int64, device=dev)
    arch = sparse_tsdf.BrickArchive.empty(4, True, True, dev)

    def call(**kw):
        a = dict(flags=_lib.SPARSE_RELEASE_OUTSIDE | _lib.SPARSE_RELEASE_ARCHIVE, archive_capacity=4, vol=vol._vol, born=vol.born.data_ptr(), box=box.data_ptr(),
                 arch_brick=arch.bricks.data_ptr(), arch_born=arch.born.data_ptr(), arch_tsdf=arch.tsdf.data_ptr(), arch_weight=arch.weight.data_ptr(),
                 arch_color=arch.color.data_ptr(), scratch=scratch.data_ptr(), record=rec.data_ptr())
        a.update(kw)
        with torch.cuda.device(dev):
            args = _lib.SparseReleaseArgs.new(**a)
            rc = lib.mipsf_sparse_release(C.byref(args), _lib.stream_ptr())
        return rc, lib.mipsf_last_error().decode()
    for kw, said in ((dict(flags=8 | 1), "flags"), (dict(flags=0), "predicate"), (dict(flags=4), "predicate"), (dict(box=None), "box"),
                     (dict(arch_color=None), "arch_color"), (dict(arch_born=None), "arch_born"), (dict(arch_tsdf=None), "archive"),
                     (dict(scratch=None), "scratch"), (dict(scratch=scratch.data_ptr() + 4), "scratch"), (dict(record=None), "record")):
        rc, msg = call(**kw)
        assert rc != 0 and said in msg, (kw, msg)
    assert lib.mipsf_sparse_release_scratch_words(0) == 0 and lib.mipsf_sparse_release_scratch_words(_lib.SPARSE_MAX_CAPACITY + 1) == 0
    torch.cuda.synchronize()
    assert _differs(vol, sp) == [] and _guards_hold(vol, guards) == [] and not rec.any()
    assert call()[0] == 0                                         # and the call these were made from goes through
    RL.release(sp, FAR, archive_capacity=4)
    assert _differs(vol, sp) == []
