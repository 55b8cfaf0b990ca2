"""GPU tests of the removal of fused views from the brick-sparse volume (mipsfusion_amd/sparse_tsdf.py history, deintegrate and
reintegrate, csrc/sparse_remove.hip) against the float64 restatement of tests/sparse_remove_cpu.py.  Both sides get the same fp32
words and evaluate the same float64 expressions in the same view order under the same history, so the words, the five counts,
`born` and `serial` are compared for EQUALITY; the restatement tests every voxel against every view, so equality also shows that the
brick culling takes a view out of every voxel it went into.  tests/test_sparse_remove_cpu.py holds the restatement to what is known
of it, and shows on the reversed box room that the equality here cannot hold without the history."""
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, sparse_tsdf

from . import sparse_cpu as S
from . import sparse_remove_cpu as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _make(c, dev, capacity, history=True, max_weight=math.inf):
    return sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], capacity, color=c["rgb"] is not None, max_weight=max_weight,
                                        device=dev, history=history)


def _fuse(c, dev, capacity, poses=None, **kw):
    vol = _make(c, dev, capacity)
    return vol, vol.integrate(c["depth"], c["poses"] if poses is None else poses, c["K"], c["rgb"], c["depth_max"], **kw)


def _counts(counts):
    return tuple(counts[k] for k in ("updates", "observed", "marked", "new", "dropped", "in_use"))


def _allocation(vol):
    return [t.clone() for t in (vol.table, vol.slot_brick, vol.count)]


def _allocation_differs(vol, sp):
    n = int(vol.count.item())
    out = []
    if n != len(sp["slot_brick"]):
        out.append(f"count {n} != {len(sp['slot_brick'])}")
    if vol.slot_brick[:n].cpu().tolist() != sp["slot_brick"]:
        out.append("slot order")
    if not np.array_equal(vol.table.cpu().numpy(), S.table_of(sp)):
        out.append("table")
    return out


def _history_differs(vol, sp):
    """born of the slots in use, born of the others (unset) and serial against the restatement's -> what differs"""
    n = len(sp["slot_brick"])
    born = vol.born.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    out = []
    if not np.array_equal(born[:n], SR.born_of_slots(sp)):
        out.append("born")
    if not (born[n:] == _lib.SPARSE_UNBORN).all():
        out.append("born beyond the count")
    if int(vol.serial.item()) != sp["serial"] or vol.views_fused != sp["serial"]:
        out.append(f"serial {int(vol.serial.item())}, mirror {vol.views_fused}, restatement {sp['serial']}")
    return out


def _state_differs(vol, sp):
    """the words of to_dense over the restatement's window -> differing words per array"""
    d = vol.to_dense(sp["lo"], sp["hi"])
    out = {"tsdf": int((_words(d.tsdf) != _words(sp["state"]["tsdf"])).sum()), "weight": int((_words(d.weight) != _words(sp["state"]["weight"])).sum())}
    if sp["state"]["color"] is not None:
        out["color"] = int((_words(d.color) != _words(sp["state"]["color"])).sum())
    return out


def _views(c, views, ids, poses=None):
    """the arguments of deintegrate for some views of a case"""
    return (c["depth"][views], (c["poses"] if poses is None else poses)[views], c["K"], ids[views], None if c["rgb"] is None else c["rgb"][views], c["depth_max"])


def _pool_is_zero(vol):
    return all(t is None or not _words(t).any() for t in (vol.tsdf, vol.weight, vol.color))


class _Launches:
    """counts the launches of the two routes a SparseTSDFVolume takes"""

    def __init__(self, monkeypatch):
        self.gone, self.fused = [], []
        real_gone, real_fused = sparse_tsdf.SparseTSDFVolume.deintegrate_enqueue, sparse_tsdf.SparseTSDFVolume.integrate_enqueue

        def gone(vol, depth, *a, **kw):
            self.gone.append(depth.shape[0])
            return real_gone(vol, depth, *a, **kw)

        def fused(vol, depth, *a, **kw):
            self.fused.append(depth.shape[0])
            return real_fused(vol, depth, *a, **kw)
        monkeypatch.setattr(sparse_tsdf.SparseTSDFVolume, "deintegrate_enqueue", gone)
        monkeypatch.setattr(sparse_tsdf.SparseTSDFVolume, "integrate_enqueue", fused)


# ------------------------------------------------------------------------------------------------------------- 1. words and counts
@pytest.mark.parametrize("name", SR.GPU_CASES)
def test_the_words_the_counts_and_the_history_equal_the_restatement(dev, name):
    """the case fused with history, the views at the even positions removed: the restatement's words, counts, born and serial; the
    rest too: every word of the pool is zero and nothing of the allocation moved"""
    c = SR.case(name)
    sp, half, want = c["fused"], c["half"], c["counts"]
    vol, counts = _fuse(c, dev, sp["capacity"])
    ids = vol.last_view_ids
    assert tuple(counts) == _counts(want) and counts.dropped == 0, name
    assert ids.dtype == np.int64 and np.array_equal(ids, want["ids"]) and vol.views_fused == len(c["depth"])
    assert _allocation_differs(vol, sp) == [] and _history_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values()), name
    held = _allocation(vol)
    got = vol.deintegrate(*_views(c, c["even"], ids))
    diff = _state_differs(vol, half)
    print(f"{name}: dims {c['dims']}, {len(c['even'])} of {len(c['depth'])} views removed from {counts.bricks_in_use} bricks, differing words {diff}, counts "
          f"{tuple(got)} (restatement {c['removed_even'][:5]}), pairs in bricks born after their view {c['removed_even'][5]}")
    assert isinstance(got, sparse_tsdf.SparseRemoveCounts) and tuple(got) == c["removed_even"][:5], name
    assert not any(diff.values()) and _history_differs(vol, half) == [], name
    rest = vol.deintegrate(*_views(c, c["odd"], ids))
    assert tuple(rest) == c["removed_odd"][:5] and rest.observed == 0 and rest.bricks_emptied == counts.bricks_in_use, name
    assert got.removed + rest.removed == counts.updates and got.emptied + rest.emptied == counts.observed and got.missing == rest.missing == 0
    assert _pool_is_zero(vol), name
    assert all(torch.equal(a, b) for a, b in zip(held, _allocation(vol))) and _history_differs(vol, sp) == [], name
    if name == SR.REVERSED:
        assert c["removed_even"][5] > 0
    if name == "many_views":                                      # 129 and 128 views a call above; all 257 in one cross the chunk boundary
        assert len(c["depth"]) == _lib.TSDF_VIEW_CHUNK + 1
        vol, counts = _fuse(c, dev, sp["capacity"])
        every = vol.deintegrate(*_views(c, slice(None), vol.last_view_ids))
        assert tuple(every) == (counts.updates, 0, counts.observed, 0, counts.bricks_in_use) and _pool_is_zero(vol)


# ------------------------------------------------------------------------------------------------------------- 2. cuts, culling
@pytest.mark.parametrize("name", [SR.REVERSED, "colour", "two_rooms/v0.20"])
def test_the_cut_into_calls_and_the_culling_do_not_reach_the_bytes(dev, name):
    c = SR.case(name)
    sp, half = c["fused"], c["half"]
    for per in (1, 7, None):
        vol, _ = _fuse(c, dev, sp["capacity"])
        got = vol.deintegrate(*_views(c, c["even"], vol.last_view_ids), views_per_call=per)
        assert not any(_state_differs(vol, half).values()) and tuple(got) == c["removed_even"][:5], per
        # the fusion cut the same way: other slot numbers, the same born for every brick, the same words and counts
        vol, _ = _fuse(c, dev, sp["capacity"], views_per_call=per)
        cut, _ = SR.fuse(name, views_per_call=per)
        assert _allocation_differs(vol, cut) == [] and _history_differs(vol, cut) == [] and np.array_equal(cut["born"], sp["born"]), per
        got = vol.deintegrate(*_views(c, c["even"], vol.last_view_ids), views_per_call=per)
        assert not any(_state_differs(vol, half).values()) and tuple(got) == c["removed_even"][:5], per
    vol, _ = _fuse(c, dev, sp["capacity"])                        # every brick takes every view of its history
    depth, poses, K, ids, rgb, depth_max = _views(c, c["even"], vol.last_view_ids)
    depth, poses = torch.from_numpy(depth).to(dev), poses.to(dev).contiguous()
    rgb = None if rgb is None else torch.from_numpy(rgb).to(dev)
    ids32 = torch.from_numpy(ids.astype(np.int32)).to(dev)
    rec = vol.deintegrate_enqueue(depth, poses, K, ids32, rgb, depth_max, flags=_lib.TSDF_NO_CULL)
    assert rec.dtype == torch.int64 and rec.is_cuda and tuple(rec.tolist()) == c["removed_even"][:5]
    assert not any(_state_differs(vol, half).values())
    none = vol.deintegrate_enqueue(depth[:0], poses[:0], K, ids32[:0], None if rgb is None else rgb[:0])        # n = 0: the two standing counts
    assert none.tolist() == [0, 0, 0, c["removed_even"][3], c["removed_even"][4]] and not any(_state_differs(vol, half).values())
    if hasattr(torch, "uint32"):                                  # the ids as unsigned words
        again = vol.deintegrate_enqueue(depth[:0], poses[:0], K, ids32[:0].view(torch.uint32), None if rgb is None else rgb[:0])
        assert again.tolist() == none.tolist()


# ------------------------------------------------------------------------------------------------------------- 3. opt-in
@pytest.mark.parametrize("name", [SR.REVERSED, "colour"])
def test_the_history_changes_nothing_of_the_volume(dev, name):
    c = SR.case(name)
    cap = c["fused"]["capacity"]
    plain, with_history = _make(c, dev, cap, history=False), _make(c, dev, cap)
    a = plain.integrate(c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], views_per_call=7)
    b = with_history.integrate(c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], views_per_call=7)
    assert a == b and plain.born is None and plain.serial is None and plain.views_fused == 0 and len(plain.last_view_ids) == 0
    for x, y in zip(_allocation(plain) + [plain._birth], _allocation(with_history) + [with_history._birth]):
        assert torch.equal(x, y)
    for x, y in ((plain.tsdf, with_history.tsdf), (plain.weight, with_history.weight), (plain.color, with_history.color)):
        assert x is None or np.array_equal(_words(x), _words(y))
    with_history.reset()
    assert with_history.views_fused == 0 and int(with_history.serial) == 0 and bool((with_history.born == -1).all()) and _pool_is_zero(with_history)


# ------------------------------------------------------------------------------------------------------------- 4. reintegrate
def test_reintegrate_equals_remove_then_fuse_of_the_restatement(dev, monkeypatch):
    d = SR.drifted()
    c, wrong, odd = d["case"], d["poses_drifted"], d["odd"]
    stale, corrected = d["stale"], d["corrected"]
    vol, _ = _fuse(c, dev, stale["capacity"], wrong)
    ids = vol.last_view_ids
    assert not any(_state_differs(vol, stale).values()) and _history_differs(vol, stale) == []
    launches = _Launches(monkeypatch)
    seen, idle = int((stale["state"]["weight"] > 0).sum()), SR.bricks_emptied(stale)
    # nothing moves: the same poses, or thresholds above the drift
    for old, new, kw in ((wrong, wrong, {}), (wrong, c["poses"], dict(min_translation=1.0, min_rotation=1.0))):
        got = vol.reintegrate(c["depth"], old, new, c["K"], ids, None, c["depth_max"], **kw)
        assert got.views_moved == 0 and np.array_equal(got.view_ids, ids)
        assert got.removed == sparse_tsdf.SparseRemoveCounts(0, 0, 0, seen, idle) and got.fused == sparse_tsdf.SparseTSDFCounts(0, seen, 0, 0, 0, len(stale["slot_brick"]))
        assert launches.gone == [] and launches.fused == [] and not any(_state_differs(vol, stale).values()) and _history_differs(vol, stale) == []
    got = vol.reintegrate(c["depth"], wrong, c["poses"], c["K"], ids, None, c["depth_max"])
    assert launches.gone == [len(odd)] and launches.fused == [len(odd)]                               # the moved views only, one launch each
    diff = _state_differs(vol, corrected)
    print(f"{SR.DRIFT}: {got.views_moved} views moved, removed {tuple(got.removed)} (restatement {d['removed'][:5]}), fused {tuple(got.fused)} "
          f"(restatement {_counts(d['fused'])}), differing words {diff}")
    assert isinstance(got, sparse_tsdf.SparseReintegrateCounts) and got.views_moved == len(odd)
    assert tuple(got.removed) == d["removed"][:5] and tuple(got.fused) == _counts(d["fused"])
    assert got.view_ids.dtype == np.int64 and np.array_equal(got.view_ids, d["ids"]) and np.array_equal(vol.last_view_ids, d["fused"]["ids"])
    assert not any(diff.values()) and _allocation_differs(vol, corrected) == [] and _history_differs(vol, corrected) == []
    assert len(corrected["slot_brick"]) >= len(stale["slot_brick"])
    # with the true poses for both arguments nothing is launched and the words are the ones from before
    launches.gone.clear(), launches.fused.clear()
    again = vol.reintegrate(c["depth"], c["poses"], c["poses"], c["K"], got.view_ids, None, c["depth_max"])
    assert again.views_moved == 0 and launches.gone == [] and launches.fused == [] and not any(_state_differs(vol, corrected).values())


# ------------------------------------------------------------------------------------------------------------- 5. graph replay
def test_one_frame_with_history_replays_from_a_graph(dev):
    """integrate_enqueue with history captured for one frame and replayed for frames 0 .. 4: the stamp reads and moves the serial
    on the device, so born, serial and the pool are those of five eager calls; the host's mirror saw one call (the capture) and
    sync_views() brings it up to the device's count"""
    c = SR.inputs(SR.REVERSED)
    frames = 5
    cap = SR.case(SR.REVERSED)["fused"]["capacity"]
    vol = _make(c, dev, cap)
    D, P = torch.from_numpy(c["depth"][:1]).to(dev), c["poses"][:1].to(dev).contiguous()
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        vol.integrate_enqueue(D, P, c["K"])                       # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    vol.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        rec, alloc = vol.integrate_enqueue(D, P, c["K"])
    assert vol.views_fused == 1
    for frame in range(frames):
        D.copy_(torch.from_numpy(c["depth"][frame:frame + 1]))
        P.copy_(c["poses"][frame:frame + 1])
        g.replay()
    torch.cuda.synchronize()
    eager = _make(c, dev, cap)
    eager.integrate(c["depth"][:frames], c["poses"][:frames], c["K"], views_per_call=1)
    assert eager.views_fused == frames and int(vol.serial) == frames and vol.views_fused == 1
    for x, y in zip(_allocation(vol) + [vol.born, vol.serial], _allocation(eager) + [eager.born, eager.serial]):
        assert torch.equal(x, y)
    assert np.array_equal(_words(vol.tsdf), _words(eager.tsdf)) and np.array_equal(_words(vol.weight), _words(eager.weight))
    assert vol.sync_views() == frames == vol.views_fused
    sp = SR.fresh(SR.REVERSED)
    SR.integrate(sp, c["depth"][:frames], c["poses"][:frames], c["K"], views_per_call=1)
    assert _allocation_differs(vol, sp) == [] and _history_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values())
    assert int(sp["born"].max()) > 0 and int(alloc[3]) == len(sp["slot_brick"])
    # and the replayed views leave under the ids the device gave them
    got = vol.deintegrate(c["depth"][:frames], c["poses"][:frames], c["K"], np.arange(frames))
    assert got.missing == 0 and got.observed == 0 and _pool_is_zero(vol)


# ------------------------------------------------------------------------------------------------------------- 6. a full pool
def test_a_full_pool_is_removed_from_like_any_other_and_nothing_beyond_it_is_written(dev):
    name = SR.REVERSED
    c = SR.case(name)
    need = c["counts"]["in_use"]
    cap = need // 2
    sp, want = SR.fuse(name, capacity=cap)
    vol = _make(c, dev, cap)
    # the pool and the per-slot arrays two slots longer, the two guard slots full of a sentinel
    fills = (("tsdf", 7.0), ("weight", 7.0), ("slot_brick", -77), ("_birth", -77), ("born", -77))
    guard = {}
    for key, fill in fills:
        old = getattr(vol, key)
        new = torch.full((cap + 2,) + tuple(old.shape[1:]), fill, dtype=old.dtype, device=dev)
        new[:cap] = old
        guard[key] = new
        setattr(vol, key, new[:cap])
    vol._bind()
    counts = vol.integrate(c["depth"], c["poses"], c["K"], None, c["depth_max"])
    ids = vol.last_view_ids
    print(f"capacity {cap} of {need}: counts {tuple(counts)} (restatement {_counts(want)})")
    assert tuple(counts) == _counts(want) and counts.dropped == need - cap and counts.bricks_in_use == cap
    assert _allocation_differs(vol, sp) == [] and _history_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values())
    held = _allocation(vol)
    want_even = SR.remove(sp, c["depth"][c["even"]], c["poses"][c["even"]], c["K"], want["ids"][c["even"]], None, c["depth_max"])
    got = vol.deintegrate(*_views(c, c["even"], ids))
    assert tuple(got) == want_even[:5] and not any(_state_differs(vol, sp).values())
    rest = vol.deintegrate(*_views(c, c["odd"], ids))
    assert rest.observed == 0 and rest.bricks_emptied == cap and got.removed + rest.removed == counts.updates and got.missing == rest.missing == 0
    assert _pool_is_zero(vol) and all(torch.equal(a, b) for a, b in zip(held, _allocation(vol)))
    assert int((vol.table >= 0).sum()) == cap                     # the dropped bricks stay unallocated
    for key, fill in fills:
        assert bool((guard[key][cap:] == fill).all()), key


# ------------------------------------------------------------------------------------------------------------- 7. inputs, refusals
def test_inputs_and_refusals(dev):
    name = "two_rooms/v0.20"
    c = SR.case(name)
    sp, half = c["fused"], c["half"]
    ev = c["even"]
    fx, fy, cx, cy = c["K"]
    Kmat = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    depth, poses, ids = c["depth"][ev], c["poses"][ev], c["counts"]["ids"][ev]
    for d, p, K, i in ((torch.from_numpy(depth).to(dev), poses.to(dev), torch.from_numpy(Kmat), torch.from_numpy(ids).to(dev)),
                       ([x for x in depth], [x for x in poses], Kmat, [int(x) for x in ids]),
                       (torch.from_numpy(depth).double(), poses.numpy(), c["K"], ids.astype(np.uint32))):
        vol, _ = _fuse(c, dev, sp["capacity"])
        assert tuple(vol.deintegrate(d, p, K, i)) == c["removed_even"][:5] and not any(_state_differs(vol, half).values())
    # removing twice: the second time the emptied voxels have nothing left, the others lose a view they held once only
    before = _allocation(vol)
    twice = vol.deintegrate(depth, poses, c["K"], ids)
    assert twice.missing > 0 and twice.removed + twice.missing == c["removed_even"][0] and all(torch.equal(a, b) for a, b in zip(before, _allocation(vol)))
    # ---- refusals, each naming its argument, with no word changed
    vol, _ = _fuse(c, dev, sp["capacity"])
    D, P, I = torch.from_numpy(depth).to(dev), poses.to(dev).contiguous(), torch.from_numpy(ids.astype(np.int32)).to(dev)
    plain = _make(c, dev, sp["capacity"], history=False)
    plain.integrate(c["depth"], c["poses"], c["K"])
    capped = _make(c, dev, sp["capacity"], max_weight=2.0)
    capped.integrate(c["depth"], c["poses"], c["K"])
    for bad, said in ((plain, "history"), (capped, "max_weight")):
        kept = bad.weight.clone()
        for call in (lambda: bad.deintegrate(depth, poses, c["K"], ids), lambda: bad.reintegrate(depth, poses, poses, c["K"], ids),
                     lambda: bad.deintegrate_enqueue(D, P, c["K"], I), lambda: bad.reintegrate_enqueue(D, P, P, c["K"], I)):
            with pytest.raises(ValueError, match=said):
                call()
        assert torch.equal(kept, bad.weight)
    with pytest.raises(ValueError, match="history"):
        plain.sync_views()
    kept = vol.weight.clone()
    with pytest.raises(ValueError, match="view_ids"):             # a wrong id count
        vol.deintegrate(depth, poses, c["K"], ids[:-1])
    with pytest.raises(ValueError, match="view_ids"):
        vol.reintegrate(c["depth"], c["poses"], c["poses"], c["K"], ids)
    with pytest.raises(ValueError, match="view_ids"):             # an id from the future
        vol.deintegrate(depth, poses, c["K"], ids + vol.views_fused)
    with pytest.raises(ValueError, match="view_ids"):
        vol.deintegrate_enqueue(D, P, c["K"], I[:-1])
    with pytest.raises(ValueError, match="view_ids"):
        vol.deintegrate_enqueue(D, P, c["K"], I.to(torch.int64))
    with pytest.raises(ValueError, match="rgb"):
        vol.deintegrate(depth, poses, c["K"], ids, rgb=np.zeros(depth.shape + (3,), np.float32))
    with pytest.raises(ValueError, match="rgb"):
        vol.reintegrate(depth, poses, poses, c["K"], ids, rgb=np.zeros(depth.shape + (3,), np.float32))
    with pytest.raises(ValueError, match="poses"):
        vol.deintegrate(depth, poses[:2], c["K"], ids)
    colour = SR.case("colour")
    with pytest.raises(ValueError, match="rgb"):
        _fuse(colour, dev, 64)[0].deintegrate(colour["depth"], colour["poses"], colour["K"], colour["counts"]["ids"])
    assert torch.equal(kept, vol.weight) and vol.views_fused == len(c["depth"])
