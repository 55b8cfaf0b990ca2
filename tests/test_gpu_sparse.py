"""GPU tests of the brick-sparse TSDF volume (mipsfusion_amd/sparse_tsdf.py, csrc/sparse.hip) against the float64 restatement of
tests/sparse_cpu.py.  Both sides get the same fp32 words and evaluate the same float64 expressions in the same order, so the table,
the slots, the births, the counts, the words of to_dense and of the ray cast and the mesh are compared for EQUALITY; the
registration is held to track_cpu.register run on the device's own ray cast, as in tests/test_gpu_track.py.
tests/test_sparse_cpu.py holds the restatement to the dense one."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, sparse_tsdf, tsdf

from . import raster_cpu as R
from . import sparse_cpu as S
from . import track_cpu as TC
from . import tsdf_cpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _make(c, dev, capacity=None):
    return sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], c["sp"]["capacity"] if capacity is None else capacity,
                                        color=c["rgb"] is not None, max_weight=c["max_weight"], device=dev)


def _fuse(c, dev, capacity=None, **kw):
    vol = _make(c, dev, capacity)
    return vol, vol.integrate(c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], **kw)


def _counts(counts):
    return tuple(counts[k] for k in ("updates", "observed", "marked", "new", "dropped", "in_use"))


def _allocation_differs(vol, sp):
    """the table, the count and the slots in use against the restatement's -> what differs"""
    n = int(vol.count.item())
    out = []
    if n != len(sp["slot_brick"]):
        out.append(f"count {n} != {len(sp['slot_brick'])}")
    if vol.slot_brick[:n].cpu().tolist() != sp["slot_brick"]:
        out.append("slot order")
    if not np.array_equal(vol.table.cpu().numpy(), S.table_of(sp)):
        out.append("table")
    return out


def _state_differs(vol, sp):
    """the words of to_dense over the restatement's window -> differing words per array"""
    d = vol.to_dense(sp["lo"], sp["hi"])
    out = {"tsdf": int((_words(d.tsdf) != _words(sp["state"]["tsdf"])).sum()), "weight": int((_words(d.weight) != _words(sp["state"]["weight"])).sum())}
    if sp["state"]["color"] is not None:
        out["color"] = int((_words(d.color) != _words(sp["state"]["color"])).sum())
    return out


def _views(c):
    """the poses a case is ray cast from, and the far plane: views 0, 7 and 13 of the box poses, the first two elsewhere; the
    virtual grid's rays end at 10 m (the restatement walks every ray sample by sample)"""
    n = len(c["poses"])
    picks = list(TC.BOX_VIEWS) if n >= 20 else [k for k in (0, 1) if k < n and np.isfinite(c["poses"][k].numpy()).all()]
    return c["poses"][picks], (10.0 if c["dims"] == S.VIRTUAL_DIMS else float("inf"))


# ------------------------------------------------------------------------------------------------------------- 1. the device = the restatement
@pytest.mark.parametrize("name", S.GPU_CASES)
def test_allocation_words_ray_cast_and_mesh_equal_the_restatement(dev, name):
    c = S.case(name)
    sp, want = c["sp"], c["counts"]
    vol, counts = _fuse(c, dev)
    assert isinstance(counts, sparse_tsdf.SparseTSDFCounts) and tuple(vol.tsdf.shape) == (sp["capacity"], 8, 8, 16) and vol.tsdf.device.type == "cuda"
    n = counts.bricks_in_use
    births = vol._birth[:n].cpu().tolist()
    diff = _state_differs(vol, sp)
    print(f"{name}: dims {c['dims']}, bricks {vol.bricks}, {len(c['poses'])} views, counts {tuple(counts)} (restatement {_counts(want)}), "
          f"born after view 0: {sum(b > 0 for b in births)}, differing words {diff}")
    assert tuple(counts) == _counts(want) and counts.dropped == 0, name
    assert _allocation_differs(vol, sp) == [], name
    assert births == [want["births"][b] for b in sp["slot_brick"]], name
    assert not any(diff.values()), name
    # words of slots beyond the count, and of a slot's voxels outside the grid, stay zero
    assert not vol.weight[n:].any() and not vol.tsdf[n:].any()
    # ---- the ray cast, with the shortcut for unallocated base bricks and without
    poses, far = _views(c)
    color = c["rgb"] is not None
    ref = S.raycast(sp, poses, c["K"], c["H"], c["W"], far=far, color=color)
    P = poses.to(dev).contiguous()
    for flags in (0, _lib.SPARSE_NO_SKIP):
        got = vol.raycast_enqueue(P, c["K"], c["H"], c["W"], far=far, color=color, flags=flags)
        bad = {"depth": int((_words(got.depth) != _words(ref["depth"])).sum()), "normals": int((_words(got.normals) != _words(ref["normals"])).sum())}
        if color:
            bad["color"] = int((_words(got.color) != _words(ref["color"])).sum())
        print(f"  ray cast flags {flags}: hits {int(got.hits[0])} (restatement {ref['hits']}) of {len(poses) * c['H'] * c['W']}, differing words {bad}")
        assert not any(bad.values()) and got.hits.tolist() == [ref["hits"], 0], (name, flags)
    # ---- the mesh of the window
    window = (sp["lo"], sp["hi"])
    m = vol.extract_mesh(window=window)
    if min(b - a for a, b in zip(*window)) < 2:
        assert len(m.faces) == 0
    else:
        want_v, want_f, index_v = S.extract_mesh(sp)
        assert np.array_equal(m.faces, want_f) and np.array_equal(m.vertices, want_v), name
        if color:
            st = S.window_state(sp)
            assert np.array_equal(_words(m.vertex_colors), _words(T.sample_color(index_v, st["weight"], st["color"])))
    if name == "box/40x56/v0.10/t4":
        assert len(m.faces) > 1000 and sum(b > 0 for b in births) == 106 and n == 129
    if name == "many_views":
        assert len(c["poses"]) == _lib.TSDF_VIEW_CHUNK + 1
    if name == "nan_pose":
        assert not np.isfinite(c["poses"][2].numpy()).any() and 2 not in births


def test_the_virtual_grid_is_refused_by_the_dense_volume_and_the_default_window_is_tight(dev):
    c = S.case(S.VIRTUAL)
    assert c["dims"][0] * c["dims"][1] * c["dims"][2] > _lib.TSDF_MAX_VOXELS
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], device=dev)
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.tsdf_mesh_from_frames(c["depth"], c["poses"], c["K"], c["voxel"], c["trunc"],
                                   bounds=np.stack([c["origin"], c["origin"] + c["voxel"] * (np.asarray(c["dims"]) - 1.5)], 1), device=dev)
    vol, counts = _fuse(c, dev)
    lo, hi = vol.tight_window()
    assert (lo, hi) == S.tight_window(c["sp"]) and all(a >= b for a, b in zip(lo, c["sp"]["lo"])) and all(a <= b for a, b in zip(hi, c["sp"]["hi"]))
    d = vol.to_dense()
    assert d.dims == tuple(b - a for a, b in zip(lo, hi)) and np.array_equal(d.origin, c["origin"] + c["voxel"] * np.asarray(lo, np.float64))
    want_v, want_f, _ = S.extract_mesh(c["sp"], lo, hi)
    m = vol.extract_mesh()
    assert np.array_equal(m.faces, want_f) and np.array_equal(m.vertices, want_v) and len(want_f) > 1000
    with pytest.raises(ValueError, match="window of 2048 x 2048 x 2048"):
        vol.extract_mesh(window=((0, 0, 0), c["dims"]))
    # the namesake of tsdf_mesh_from_frames over the same bounds gives the same mesh
    bounds = np.stack([c["origin"], c["origin"] + c["voxel"] * (np.asarray(c["dims"]) - 1.5)], 1)
    m2 = sparse_tsdf.sparse_tsdf_mesh_from_frames(c["depth"], c["poses"], c["K"], c["voxel"], 1024, c["trunc"], bounds=bounds, device=dev)
    assert np.array_equal(m2.faces, want_f) and np.array_equal(m2.vertices, want_v)
    with pytest.raises(RuntimeError, match="found no slot"):
        sparse_tsdf.sparse_tsdf_mesh_from_frames(c["depth"], c["poses"], c["K"], c["voxel"], 50, c["trunc"], bounds=bounds, device=dev)


# ------------------------------------------------------------------------------------------------------------- 2. overflow, cuts
def test_a_full_pool_drops_the_rest_and_writes_nothing_beyond_it(dev):
    name = "box/40x56/v0.10/t4"
    c = S.case(name)
    need = c["counts"]["in_use"]
    cap = need // 2
    sp, want = S.fuse(name, capacity=cap)
    vol = _make(c, dev, cap)
    # the pool and the per-slot arrays two slots longer, the two guard slots full of a sentinel
    guard = {}
    for key, fill in (("tsdf", 7.0), ("weight", 7.0), ("slot_brick", -77), ("_birth", -77)):
        old = getattr(vol, key)
        new = torch.full((cap + 2,) + tuple(old.shape[1:]), fill, dtype=old.dtype, device=dev)
        new[:cap] = old
        guard[key] = new
        setattr(vol, key, new[:cap])
    vol._bind()
    counts = vol.integrate(c["depth"], c["poses"], c["K"], None, c["depth_max"])
    print(f"capacity {cap} of {need}: counts {tuple(counts)} (restatement {_counts(want)})")
    assert tuple(counts) == _counts(want) and counts.dropped == need - cap and counts.bricks_in_use == cap
    assert _allocation_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values())
    for key, fill in (("tsdf", 7.0), ("weight", 7.0), ("slot_brick", -77), ("_birth", -77)):
        assert bool((guard[key][cap:] == fill).all()), key
    assert int((vol.table >= 0).sum()) == cap and int(vol.table.max()) == cap - 1
    # a second call over a full pool: the same drops again, nothing moves
    again = vol.integrate(c["depth"][:3], c["poses"][:3], c["K"])
    assert again.new == 0 and again.dropped > 0 and again.bricks_in_use == cap
    for key, fill in (("tsdf", 7.0), ("weight", 7.0), ("slot_brick", -77), ("_birth", -77)):
        assert bool((guard[key][cap:] == fill).all()), key


@pytest.mark.parametrize("name", ["box/40x56/v0.10/t4", "colour"])
def test_the_cut_into_calls_does_not_reach_the_words(dev, name):
    c = S.case(name)
    for per in (1, 3, None):
        vol, counts = _fuse(c, dev, views_per_call=per)
        assert not any(_state_differs(vol, c["sp"]).values()), per
        assert (counts.updates, counts.observed, counts.dropped, counts.bricks_in_use) == tuple(c["counts"][k] for k in ("updates", "observed", "dropped", "in_use"))
        if per == 1:                                             # the restatement cut the same way numbers the slots the same way
            sp, _ = S.fuse(name, views_per_call=1)
            assert _allocation_differs(vol, sp) == [] and sp["slot_brick"] != c["sp"]["slot_brick"]
    # culling off, and n = 0
    D, P = torch.from_numpy(c["depth"]).to(dev), c["poses"].to(dev).contiguous()
    C3 = None if c["rgb"] is None else torch.from_numpy(c["rgb"]).to(dev)
    vol.reset()
    assert int(vol.count) == 0 and not vol.weight.any() and int(vol.table.max()) == -1
    rec, alloc = vol.integrate_enqueue(D, P, c["K"], C3, c["depth_max"], flags=_lib.TSDF_NO_CULL)
    assert rec.tolist() == [c["counts"]["updates"], c["counts"]["observed"]] and alloc.tolist()[1:] == [c["counts"]["new"], 0, c["counts"]["in_use"]]
    assert not any(_state_differs(vol, c["sp"]).values()) and _allocation_differs(vol, c["sp"]) == []
    before = vol.tsdf.clone()
    rec, alloc = vol.integrate_enqueue(D[:0], P[:0], c["K"], None if C3 is None else C3[:0])
    assert rec.tolist() == [0, 0] and alloc.tolist() == [0, 0, 0, c["counts"]["in_use"]] and torch.equal(before, vol.tsdf)


# ------------------------------------------------------------------------------------------------------------- 3. tracking
@pytest.mark.parametrize("seed", [2, 4])
def test_track_equals_the_restatement_on_the_device_s_own_ray_cast(dev, seed):
    c = S.case("box/40x56/v0.10/t4")
    vol, _ = _fuse(c, dev)
    _, _, lo, hi = R.box_room()
    ref = c["poses"][7].numpy()
    truth = TC.perturbed(ref, 1.9, 5.8, seed)
    live = R.box_exit_depth(lo, hi, truth, c["K"], c["H"], c["W"]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)          # noqa: E731
    model = vol.raycast_enqueue(t(ref)[None], c["K"], c["H"], c["W"])
    result, pose, partner = vol.track_enqueue(t(live), c["K"], t(ref), t(ref), model, partner=True)
    want = TC.register(model.depth[0].cpu().numpy(), model.normals[0].cpu().numpy(), ref, live, ref, c["K"], max_dist=c["trunc"])
    r = result.cpu().numpy()
    Tg, amb = r[:16].reshape(4, 4), sum(want["ambiguous_per_eval"])
    print(f"seed {seed}: iterations {int(r[19])} {want['iterations']}, pairs {int(r[16])} {want['n']}, ambiguous {amb}, max |dT| {np.abs(Tg - want['transformation']).max():.3e}")
    assert amb == 0 and int(r[16]) == want["n"] and int(r[19]) == want["iterations"] and float(r[17]) == want["fitness"]
    assert np.array_equal(partner.cpu().numpy().reshape(-1), want["partner"])
    assert np.abs(Tg - want["transformation"]).max() < 1e-9 and abs(float(r[18]) - want["rmse"]) < 1e-12
    assert np.array_equal(pose.cpu().numpy(), Tg.astype(np.float32))
    # track(): the ray cast and the registration in one, and it has no arithmetic of its own: the dense volume of the same words
    # gives the same bytes
    got = vol.track(live, c["K"], ref)
    dense = vol.to_dense((0, 0, 0), c["dims"]).track(live, c["K"], ref)
    assert isinstance(got, tsdf.TrackResult) and torch.equal(got.transformation, dense.transformation) and got[2:] == dense[2:]
    assert np.array_equal(got.transformation.numpy(), Tg) and got.n_correspondences == want["n"]
    deg, m = TC.pose_error(got.transformation.numpy(), truth)
    assert m < 0.01 and deg < 0.3


def test_track_with_colour_is_the_dense_volume_s(dev):
    c = S.case("colour")
    vol, _ = _fuse(c, dev)
    dense = vol.to_dense((0, 0, 0), c["dims"])
    k = 1
    init = TC.perturbed(c["poses"][k].numpy(), 0.64, 2.3, 1)
    got = vol.track(c["depth"][k], c["K"], init, rgb=c["rgb"][k])
    want = dense.track(c["depth"][k], c["K"], init, rgb=c["rgb"][k])
    assert isinstance(got, tsdf.ColorTrackResult) and torch.equal(got.transformation, want.transformation) and got[2:] == want[2:]
    assert got.n_correspondences > 100 and got.n_color > 0
    with pytest.raises(ValueError, match="without colour"):
        _fuse(S.case("bad_pixels"), dev)[0].track(c["depth"][k], c["K"], init, rgb=c["rgb"][k])


def test_odometry_equals_the_restatement_fed_with_the_device_s_poses(dev):
    o = TC.odo_case()
    K, H, W = o["K"], o["H"], o["W"]
    poses, records, vol = sparse_tsdf.sparse_tsdf_odometry(torch.from_numpy(o["depth"]).to(dev), K, o["truth"][0], o["voxel"], o["bounds"], 256, o["trunc"])
    assert vol.dims == o["dims"] and np.array_equal(vol.origin, o["origin"]) and poses.dtype == torch.float32 and not poses.is_cuda
    poses = poses.numpy()
    assert np.array_equal(poses[0], o["truth"][0]) and not any(r["lost"] for r in records) and records[-1]["dropped"] == 0
    sp = S.new_volume(o["origin"], o["voxel"], o["dims"], o["trunc"], 256)
    S.integrate(sp, o["depth"][:1], poses[:1], K)
    for k in range(1, TC.ODO_FRAMES):
        m = S.raycast(sp, poses[k - 1:k], K, H, W)
        want = TC.register(m["depth"][0], m["normals"][0], poses[k - 1], o["depth"][k], poses[k - 1], K, max_dist=o["trunc"])
        got, amb = records[k], sum(want["ambiguous_per_eval"])
        Tg = got["transformation"].numpy()
        print(f"frame {k}: iterations {got['iterations']} {want['iterations']}, pairs {got['n_correspondences']} {want['n']}, ambiguous {amb}, "
              f"max |dT| {np.abs(Tg - want['transformation']).max():.3e}")
        assert abs(got["n_correspondences"] - want["n"]) <= amb
        if amb == 0:
            assert got["iterations"] == want["iterations"] and got["fitness"] == want["fitness"] and abs(got["inlier_rmse"] - want["rmse"]) < 1e-12
            assert np.abs(Tg - want["transformation"]).max() < 1e-9
        assert np.array_equal(poses[k], Tg.astype(np.float32))
        S.integrate(sp, o["depth"][k:k + 1], poses[k:k + 1], K)
    print(f"bricks in use {records[-1]['bricks_in_use']} of {np.prod(vol.bricks)}; decisions near a last bit {sp['ambiguous'].tolist()}")
    assert records[-1]["bricks_in_use"] == len(sp["slot_brick"]) and _allocation_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values())
    # a lost frame is fused at a NaN pose: it allocates and updates nothing
    depth = o["depth"].copy()
    depth[3] = 0.0
    poses2, records2, vol2 = sparse_tsdf.sparse_tsdf_odometry(depth[:5], K, o["truth"][0], o["voxel"], o["bounds"], 256, o["trunc"], min_correspondences=100, device=dev)
    assert [r["lost"] for r in records2] == [False, False, False, True, False] and np.array_equal(poses2[3].numpy(), poses2[2].numpy())
    sp2 = S.new_volume(o["origin"], o["voxel"], o["dims"], o["trunc"], 256)
    for k in (0, 1, 2, 4):
        S.integrate(sp2, depth[k:k + 1], poses2[k:k + 1].numpy(), K)
    assert _allocation_differs(vol2, sp2) == [] and not any(_state_differs(vol2, sp2).values())
    # every later frame lost, with depth that would allocate and update at the pose kept: the NaN pose keeps it out
    _, records3, vol3 = sparse_tsdf.sparse_tsdf_odometry(o["depth"][:3], K, o["truth"][0], o["voxel"], o["bounds"], 256, o["trunc"], min_correspondences=10 ** 6, device=dev)
    sp3 = S.new_volume(o["origin"], o["voxel"], o["dims"], o["trunc"], 256)
    S.integrate(sp3, o["depth"][:1], o["truth"][:1], K)
    assert [r["lost"] for r in records3] == [False, True, True] and _allocation_differs(vol3, sp3) == [] and not any(_state_differs(vol3, sp3).values())


# ------------------------------------------------------------------------------------------------------------- 4. reproducibility
def _snapshot(vol, cast):
    return [t.clone() for t in (vol.table, vol.slot_brick, vol.count, vol.tsdf, vol.weight, cast.depth, cast.normals, cast.hits)]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_every_output_repeats_bit_for_bit(dev):
    c = S.case("two_rooms/v0.20")
    P = c["poses"][:2].to(dev).contiguous()
    shots = []
    for _ in range(2):
        vol, counts = _fuse(c, dev)
        shots.append(_snapshot(vol, vol.raycast_enqueue(P, c["K"], c["H"], c["W"])) + [torch.tensor(tuple(counts)), vol.to_dense().tsdf])
    assert _same(*shots)
    vol.reset()                                                  # and the same object again after a reset
    vol.integrate(c["depth"], c["poses"], c["K"])
    assert _same(shots[0][:8], _snapshot(vol, vol.raycast_enqueue(P, c["K"], c["H"], c["W"])))


def test_one_frame_replays_from_a_graph_with_the_same_bytes(dev):
    c = S.case("box/40x56/v0.10/t4")
    vol = _make(c, dev)
    D, P = torch.from_numpy(c["depth"][:1]).to(dev), c["poses"][:1].to(dev).contiguous()

    def run():
        rec, alloc = vol.integrate_enqueue(D, P, c["K"])
        return rec, alloc, vol.raycast_enqueue(P, c["K"], c["H"], c["W"])

    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()                                                    # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        rec, alloc, cast = run()
    for frame in (7, 0):
        D.copy_(torch.from_numpy(c["depth"][frame:frame + 1]))
        P.copy_(c["poses"][frame:frame + 1])
        vol.reset()
        g.replay()
        torch.cuda.synchronize()
        replayed = _snapshot(vol, cast) + [rec.clone(), alloc.clone()]
        vol.reset()
        e_rec, e_alloc, e_cast = run()
        assert _same(replayed, _snapshot(vol, e_cast) + [e_rec, e_alloc]), frame
        assert int(alloc[3]) == int(vol.count) > 10 and int(cast.hits[0]) > 1000
    sp = S.new_volume(c["origin"], c["voxel"], c["dims"], c["trunc"], c["sp"]["capacity"])
    S.integrate(sp, c["depth"][:1], c["poses"][:1], c["K"])
    assert _allocation_differs(vol, sp) == [] and not any(_state_differs(vol, sp).values())
