"""GPU tests of the removal of fused views (mipsfusion_amd/tsdf.py deintegrate and reintegrate, csrc/tsdf_remove.hip) against the
float64 restatement of tests/tsdf_remove_cpu.py.  Both sides get the same fp32 words and evaluate the same float64 expressions in the
same view order, so tsdf, weight and colour words and the four counts are compared for EQUALITY; the restatement tests every voxel
against every view, so equality also shows that the brick culling takes a view out of every voxel it went into.
tests/test_tsdf_remove_cpu.py holds the restatement to the walls of the synthetic rooms."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, evaluate as ev, pose_graph, synth, tsdf

from . import tsdf_cpu as T
from . import tsdf_remove_cpu as RM

pytestmark = pytest.mark.gpu

CASES = ("box/33x47/v0.20/t3", "colour", "random_poses", "two_rooms/v0.20", "one_voxel", "1x5x70", "bad_pixels", "many_views", "outside")
ODD, EVEN = slice(1, None, 2), slice(0, None, 2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _fuse(c, dev, poses=None):
    vol = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], color=c["rgb"] is not None, device=dev)
    counts = vol.integrate(c["depth"], c["poses"] if poses is None else poses, c["K"], c["rgb"], c["depth_max"])
    return vol, counts


def _views(c, views, poses=None):
    """the arguments of deintegrate / integrate for some views of a case"""
    return (c["depth"][views], (c["poses"] if poses is None else poses)[views], c["K"], None if c["rgb"] is None else c["rgb"][views], c["depth_max"])


def _differing(vol, state):
    d = {"tsdf": int((_words(vol.tsdf) != _words(state["tsdf"])).sum()), "weight": int((_words(vol.weight) != _words(state["weight"])).sum())}
    if state["color"] is not None:
        d["color"] = int((_words(vol.color) != _words(state["color"])).sum())
    return d


def _snapshot(vol):
    return {"tsdf": vol.tsdf.cpu().numpy(), "weight": vol.weight.cpu().numpy(), "color": None if vol.color is None else vol.color.cpu().numpy()}


class _Launches:
    """counts the launches of the two kernels a TSDFVolume makes"""

    def __init__(self, monkeypatch):
        self.gone, self.fused = [], []
        real_gone, real_fused = tsdf.TSDFVolume.deintegrate_enqueue, tsdf.TSDFVolume.integrate_enqueue

        def gone(vol, depth, *a, **kw):
            self.gone.append(depth.shape[0])
            return real_gone(vol, depth, *a, **kw)

        def fused(vol, depth, *a, **kw):
            self.fused.append(depth.shape[0])
            return real_fused(vol, depth, *a, **kw)
        monkeypatch.setattr(tsdf.TSDFVolume, "deintegrate_enqueue", gone)
        monkeypatch.setattr(tsdf.TSDFVolume, "integrate_enqueue", fused)


# ------------------------------------------------------------------------------------------------------------- 1. the words
@pytest.mark.parametrize("name", CASES)
def test_the_volume_and_the_counts_equal_the_restatement(dev, name):
    """the case fused, its odd views removed: the restatement's words and counts; the even ones too: nothing is left"""
    c = T.case(name)
    want = RM.odd_removed(name)
    vol, fused = _fuse(c, dev)
    assert tuple(fused) == (c["updates"], c["observed"])
    counts = vol.deintegrate(*_views(c, ODD))
    diff = _differing(vol, want["state"])
    print(f"{name}: dims {c['dims']}, {len(c['poses'][ODD])} of {len(c['poses'])} views removed, differing words {diff}, counts {tuple(counts)} "
          f"(restatement {want['counts']})")
    assert isinstance(counts, tsdf.RemoveCounts) and tuple(counts) == want["counts"] and counts.missing == 0, name
    assert not any(diff.values()), name
    rest = vol.deintegrate(*_views(c, EVEN))
    assert rest.removed + counts.removed == c["updates"] and rest.emptied + counts.emptied == c["observed"] and (rest.missing, rest.observed) == (0, 0)
    for t in (vol.tsdf, vol.weight, vol.color):
        assert t is None or not _words(t).any()
    if name == "outside":
        assert tuple(counts) == (0, 0, 0, 0)
    if name == "many_views":                                      # 128 and 129 views a call above; all 257 in one cross the chunk boundary
        vol, _ = _fuse(c, dev)
        assert len(c["poses"]) == _lib.TSDF_VIEW_CHUNK + 1
        assert tuple(vol.deintegrate(*_views(c, slice(None)))) == (c["updates"], 0, c["observed"], 0) and not _words(vol.weight).any() and not _words(vol.tsdf).any()


# ------------------------------------------------------------------------------------------------------------- 2. calls, culling
@pytest.mark.parametrize("name", ["box/33x47/v0.20/t3", "two_rooms/v0.20", "colour"])
def test_the_cut_into_calls_and_the_culling_do_not_reach_the_bytes(dev, name):
    c = T.case(name)
    want = RM.odd_removed(name)
    for per in (1, 7, None):
        vol, _ = _fuse(c, dev)
        counts = vol.deintegrate(*_views(c, ODD), views_per_call=per)
        assert not any(_differing(vol, want["state"]).values()) and tuple(counts) == want["counts"], per
    vol, _ = _fuse(c, dev)                                        # every brick takes every view
    depth, poses, K, rgb, depth_max = _views(c, ODD)
    depth, poses = torch.from_numpy(depth).to(dev), poses.to(dev).contiguous()
    rgb = None if rgb is None else torch.from_numpy(rgb).to(dev)
    rec = vol.deintegrate_enqueue(depth, poses, K, rgb, depth_max, flags=_lib.TSDF_NO_CULL)
    assert rec.dtype == torch.int64 and rec.is_cuda and tuple(rec.tolist()) == want["counts"]
    assert not any(_differing(vol, want["state"]).values())
    none = vol.deintegrate_enqueue(depth[:0], poses[:0], K, None if rgb is None else rgb[:0])             # n = 0: a zero record, nothing else
    assert none.tolist() == [0, 0, 0, 0] and not any(_differing(vol, want["state"]).values())


# ------------------------------------------------------------------------------------------------------------- 3. reintegrate
@pytest.mark.parametrize("name", RM.DRIFTED_CASES)
def test_reintegrate_equals_remove_then_fuse_of_the_restatement(dev, name, monkeypatch):
    d = RM.drifted(name)
    c, wrong = d["case"], d["poses_drifted"]
    n_odd = len(c["poses"][ODD])
    vol, _ = _fuse(c, dev, wrong)
    assert not any(_differing(vol, d["stale"]).values())
    stale = _snapshot(vol)
    launches = _Launches(monkeypatch)
    # nothing moves: the same poses, or thresholds above the drift
    for old, new, kw in ((wrong, wrong, {}), (wrong, c["poses"], dict(min_translation=1.0, min_rotation=1.0))):
        got = vol.reintegrate(c["depth"], old, new, c["K"], c["rgb"], c["depth_max"], **kw)
        assert got == tsdf.ReintegrateCounts(0, tsdf.RemoveCounts(0, 0, 0, int((stale["weight"] > 0).sum())), tsdf.TSDFCounts(0, int((stale["weight"] > 0).sum())))
        assert launches.gone == [] and launches.fused == [] and not any(_differing(vol, stale).values())
    got = vol.reintegrate(c["depth"], wrong, c["poses"], c["K"], c["rgb"], c["depth_max"])
    assert launches.gone == [n_odd] and launches.fused == [n_odd]                                     # the moved views only, one launch each
    diff = _differing(vol, d["corrected"])
    print(f"{name}: {got.views_moved} views moved, {tuple(got.removed)} removed (restatement {d['removed']}), {tuple(got.fused)} fused "
          f"(restatement {d['fused']}), differing words {diff}")
    assert got.views_moved == n_odd and tuple(got.removed) == d["removed"] and tuple(got.fused) == d["fused"]
    assert not any(diff.values())
    fresh, _ = _fuse(c, dev)
    gap = float((vol.tsdf.double() - fresh.tsdf.double()).abs().max())
    gap_c = float((vol.color.double() - fresh.color.double()).abs().max()) if vol.color is not None else 0.0
    print(f"{name}: against a fresh fusion at the true poses: tsdf within {gap:.3g}, colour within {gap_c:.3g}")
    assert np.array_equal(_words(vol.weight), _words(fresh.weight)) and gap <= RM.TSDF_GATE and gap_c <= RM.COLOR_GATE
    # with the true poses for both arguments nothing is launched and the words are the ones from before
    before = _snapshot(vol)
    launches.gone.clear(), launches.fused.clear()
    again = vol.reintegrate(c["depth"], c["poses"], c["poses"], c["K"], c["rgb"], c["depth_max"])
    assert again.views_moved == 0 and launches.gone == [] and launches.fused == [] and not any(_differing(vol, before).values())


# ------------------------------------------------------------------------------------------------------------- 4. the route
def test_the_loop_closure_route_on_the_two_rooms(dev):
    """Two sub-maps, the second anchor drifted by RM.DRIFT_ANGLE rad and RM.DRIFT_SHIFT m (the drift the issue states; it did not
    have to be widened: tests/test_tsdf_remove_cpu.py measures the stale volume's accuracy at 0.078 m against 0.070 m on the
    restatement): fused at the drifted world poses, rebased to the true anchors, reintegrated.  The fresh fusion the result is
    held to is fused at the poses the volume then holds -- sub-map 0 where it was, sub-map 1 rebased -- which are the case's true
    poses up to the fp32 rounding of the rebase (asserted below 1e-6), not those poses word for word."""
    loop = RM.loop_closure()
    c, sub, wrong = loop["case"], loop["submap_of_pose"], loop["poses_drifted"]
    n_moved = int((sub == 1).sum())
    vol, _ = _fuse(c, dev, wrong)
    gt = synth.two_rooms_mesh()
    stale_mesh = vol.extract_mesh()
    stale = ev.reconstruction_metrics(stale_mesh, gt, n_samples=20000)
    poses_new = pose_graph.rebase(wrong, sub, loop["anchors_drifted"], loop["anchors_true"])
    got = vol.reintegrate(c["depth"], wrong, poses_new, c["K"], min_translation=RM.MOVED_TRANSLATION, min_rotation=RM.MOVED_ROTATION)
    assert got.views_moved == n_moved and got.removed.missing == 0 and got.removed.removed > 0 and got.fused.updates > 0
    held = wrong.clone()                                          # what the volume now holds: sub-map 0 where it was, sub-map 1 rebased
    held[sub == 1] = poses_new.to(torch.float32)[sub == 1]
    assert float((held - c["poses"]).abs().max()) < 1e-6
    fresh_vol, _ = _fuse(c, dev, held)
    assert np.array_equal(_words(vol.weight), _words(fresh_vol.weight)) and float((vol.tsdf.double() - fresh_vol.tsdf.double()).abs().max()) <= RM.TSDF_GATE
    mesh, fresh_mesh = vol.extract_mesh(), fresh_vol.extract_mesh()
    corrected, fresh = ev.reconstruction_metrics(mesh, gt, n_samples=20000), ev.reconstruction_metrics(fresh_mesh, gt, n_samples=20000)
    print(f"two rooms, {n_moved} of {len(sub)} views moved: accuracy stale {stale.accuracy:.4f} m ({len(stale_mesh.vertices)} vertices, {len(stale_mesh.faces)} "
          f"faces), corrected {corrected.accuracy:.4f} m ({len(mesh.vertices)}, {len(mesh.faces)}), fresh {fresh.accuracy:.4f} m ({len(fresh_mesh.vertices)}, "
          f"{len(fresh_mesh.faces)})")
    assert (len(mesh.vertices), len(mesh.faces)) == (len(fresh_mesh.vertices), len(fresh_mesh.faces))
    assert abs(corrected.accuracy - fresh.accuracy) <= 0.01 * fresh.accuracy
    assert stale.accuracy > max(corrected.accuracy, fresh.accuracy)


# ------------------------------------------------------------------------------------------------------------- 5. inputs
def test_inputs_and_missing_views(dev):
    c = T.case("box/33x47/v0.20/t3")
    want = RM.odd_removed("box/33x47/v0.20/t3")
    fx, fy, cx, cy = c["K"]
    Kmat = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    depth, poses = c["depth"][ODD], c["poses"][ODD]
    for d, p, K in ((torch.from_numpy(depth).to(dev), poses.to(dev), torch.from_numpy(Kmat)), ([x for x in depth], [x for x in poses], Kmat),
                    (torch.from_numpy(depth).double(), poses.numpy(), c["K"])):
        vol, _ = _fuse(c, dev)
        assert tuple(vol.deintegrate(d, p, K)) == want["counts"] and not any(_differing(vol, want["state"]).values())
    vol, _ = _fuse(c, dev)
    for d, p in zip(depth, poses):                                # a single image and pose at a time
        vol.deintegrate(d, p, c["K"])
    assert not any(_differing(vol, want["state"]).values())
    # a pose with a NaN removes nothing, as it fused nothing
    before = _snapshot(vol)
    lost = poses.clone()
    lost[:, 0, 3] = float("nan")
    assert tuple(vol.deintegrate(depth, lost, c["K"])) == (0, 0, 0, want["counts"][3]) and not any(_differing(vol, before).values())
    # a lost frame the optimisation found a pose for: nothing to remove at its NaN pose, fused for the first time at the new one
    n = len(c["poses"])
    was = c["poses"].clone()
    was[1] = float("nan")
    found, _ = _fuse(c, dev, was)
    got = found.reintegrate(c["depth"], was, c["poses"], c["K"], min_translation=1e-3, min_rotation=1e-3)
    assert got.views_moved == 1 and tuple(got.removed)[:3] == (0, 0, 0) and got.fused == (int(c["updated"][1].sum()), c["observed"])
    assert np.array_equal(_words(found.weight), _words(c["state"]["weight"])) and n > 2
    # a fresh volume has nothing to take: every hit is missing and no word changes
    empty = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], device=dev)
    assert tuple(empty.deintegrate(c["depth"], c["poses"], c["K"])) == (0, c["updates"], 0, 0) and not _words(empty.tsdf).any() and not _words(empty.weight).any()
    # removing twice: the second time the emptied voxels have nothing left, the others lose a view they never held twice
    twice = vol.deintegrate(depth, poses, c["K"])
    assert twice.missing > 0 and twice.removed + twice.missing == want["counts"][0]
    with pytest.raises(ValueError, match="color=True"):
        vol.deintegrate(depth, poses, c["K"], rgb=np.zeros(depth.shape + (3,), np.float32))
    with pytest.raises(ValueError, match="color=True"):
        vol.reintegrate(depth, poses, poses, c["K"], rgb=np.zeros(depth.shape + (3,), np.float32))
    with pytest.raises(ValueError, match="needs rgb"):
        tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], color=True, device=dev).deintegrate(depth, poses, c["K"])
    with pytest.raises(ValueError, match="poses"):
        vol.deintegrate(depth, poses[:3], c["K"])
    with pytest.raises(ValueError, match="poses"):
        vol.reintegrate(depth, poses, poses[:3], c["K"])
    capped = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], max_weight=2.0, device=dev)
    capped.integrate(c["depth"], c["poses"], c["K"])
    held = _snapshot(capped)
    for call in (lambda: capped.deintegrate(depth, poses, c["K"]), lambda: capped.reintegrate(depth, poses, poses, c["K"]),
                 lambda: capped.deintegrate_enqueue(torch.from_numpy(depth).to(dev), poses.to(dev), c["K"]),
                 lambda: capped.reintegrate_enqueue(torch.from_numpy(depth).to(dev), poses.to(dev), poses.to(dev), c["K"])):
        with pytest.raises(ValueError, match="max_weight"):
            call()
    assert not any(_differing(capped, held).values())
