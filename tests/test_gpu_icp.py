"""GPU tests of the switch-pose rectification (mipsfusion_amd/pose_corrector.py, csrc/icp.hip) against the float64 restatement
of tests/icp_cpu.py.  The device and the restatement get the same fp32 points and evaluate the same float64 expression, so
neighbour sets, pair sets and counts are compared for equality; tests/test_icp_cpu.py asserts, on the same cases, the caps that
argument needs."""
import random

import numpy as np
import pytest
import torch

from mipsfusion_amd import pose_corrector as pc, synth
from mipsfusion_amd.keyframe_rays import DeviceRayDB

from . import icp_cpu as R

pytestmark = pytest.mark.gpu

ICP_CASES = sorted(R.ROOM_CASES) + ["synth"]
# Angle between a device normal and numpy.linalg.eigh's of the same covariance, sign ignored, where (l1 - l0)/l2 >= 1e-3: the gate
# is 10 x the largest angle measured over the cases of the two normals tests, and never above 1e-5 rad (at which a 5 cm pair
# moves its residual by 5e-7 m).  MEASURED_MAX_ANGLE is filled in from a run on an MI355X.
MEASURED_MAX_ANGLE = 9.9e-15          # "first 3" of test_normals_special_cases; the 300 000-point room: 2.4e-15
NORMAL_ANGLE_GATE = 1e-5 if MEASURED_MAX_ANGLE is None else min(1e-5, 10 * MEASURED_MAX_ANGLE)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


_cache = {}


def _case(name):
    """-> (source fp32, target fp32, max_dist, restatement normals, neighbours, eigenvalues), computed once"""
    if name not in _cache:
        src, tgt, md = R.synth_case() if name == "synth" else R.room_case(name)
        _cache[name] = (src, tgt, md) + R.normals_cpu(tgt)
    return _cache[name]


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).reshape(-1, 3).to(dev).contiguous()


def _ulp_close(a, b, ulps):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


# ------------------------------------------------------------------------------------------------------------- 1. cloud
def test_cloud_keeps_rows_with_depth_in_order(dev):
    s = R.synth_scene()
    k, r = s["kf_rows"].shape[:2]
    rows = s["kf_rows"].reshape(-1, 7).contiguous()
    assert int((rows[:, 6] <= 0).sum()) > 0, "the case must hold pixels without depth"
    want, kept = R.cloud_cpu(rows, r, s["kf_poses"])
    got, m = pc.cloud_from_rays(rows.to(dev), r, s["kf_poses"].to(dev).contiguous())
    assert m == want.shape[0] and got.shape == (m, 3)
    assert _ulp_close(got.cpu().numpy(), want.numpy(), 2)
    # an owner per row, in an order of its own
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(rows.shape[0], generator=g)
    owner = (perm // r).to(torch.int32)
    want2, _ = R.cloud_cpu(rows[perm], owner, s["kf_poses"])
    got2, m2 = pc.cloud_from_rays(rows[perm].contiguous().to(dev), owner.to(dev), s["kf_poses"].to(dev).contiguous())
    assert m2 == want2.shape[0] and _ulp_close(got2.cpu().numpy(), want2.numpy(), 2)
    # nothing kept, and no rows at all
    dead = rows[:300].clone()
    dead[:, 6] = 0
    assert pc.cloud_from_rays(dead.to(dev), 300, s["kf_poses"][:1].to(dev).contiguous())[1] == 0
    assert pc.cloud_from_rays(rows[:0].to(dev), 1, s["kf_poses"][:1].to(dev).contiguous())[1] == 0
    for n in (1, 2, 1023, 1024, 1025):          # around the scan's tile
        w, _ = R.cloud_cpu(rows[:n], n, s["kf_poses"][:1])
        gg, mm = pc.cloud_from_rays(rows[:n].contiguous().to(dev), n, s["kf_poses"][:1].to(dev).contiguous())
        assert mm == w.shape[0] and _ulp_close(gg.cpu().numpy(), w.numpy(), 2)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 262145])
def test_cloud_compaction_equals_numpy_around_the_scan_tiles(dev, n):
    """flag, scan, emit with the device-wide scan of csrc/block_dev.h (uint32, exclusive): one tile of 1024 rows, either side of
    it, and just past 256 tiles, where a thread of the one-block top scan owns two tile sums.  About half the rows have no depth.
    Under the identity pose a kept row's point is fl(direction * depth), one fp32 rounding, so the cloud is compared with numpy's
    boolean compaction for equality."""
    g = np.random.default_rng(n)
    rows = np.zeros((n, 7), np.float32)
    rows[:, :3] = g.standard_normal((n, 3), dtype=np.float32)
    rows[:, 6] = np.where(g.random(n) < 0.5, g.uniform(0.5, 4.0, n), 0.0).astype(np.float32)
    keep = rows[:, 6] > 0
    assert 0.4 * n < keep.sum() < 0.6 * n
    want = (rows[:, :3] * rows[:, 6:7])[keep]
    got, m = pc.cloud_from_rays(torch.from_numpy(rows).to(dev), n, torch.eye(4).reshape(1, 4, 4).to(dev).contiguous())
    assert m == want.shape[0]
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------- 2. bin + nearest neighbour
def _check_nearest(dev, src, tgt, max_dist, max_cells=None):
    j, d2 = R.nearest_cpu(np.asarray(src, np.float64), tgt, max_dist)
    gj, gd2 = pc.nearest_neighbours(_t(src, dev), _t(tgt, dev), max_dist, max_cells=max_cells)
    gj, gd2 = gj.cpu().numpy().astype(np.int64), gd2.cpu().numpy()
    assert np.array_equal(gj, j), f"{np.count_nonzero(gj != j)} partners differ"
    assert np.array_equal(gd2, d2)
    return int((j >= 0).sum())


@pytest.mark.parametrize("name", ICP_CASES)
def test_nearest_neighbour_equals_the_restatement(dev, name):
    src, tgt, md = _case(name)[:3]
    n = _check_nearest(dev, src, tgt, md)
    print(name, "pairs", n, "of", len(src))
    if len(src) >= 1000:
        assert n > 0


def test_nearest_neighbour_special_cases(dev):
    src, tgt, md = _case("room_30k")[:3]
    # duplicates in the target: the lowest index wins
    dup = np.concatenate([tgt, tgt[:500]])
    assert _check_nearest(dev, tgt[:500], dup, md) == 500
    j, _ = pc.nearest_neighbours(_t(tgt[:500], dev), _t(dup, dev), md)
    assert torch.equal(j.cpu(), torch.arange(500, dtype=torch.int32))
    # source points outside the target's box, by less and by more than max_dist
    lo, hi = tgt.min(0), tgt.max(0)
    out = np.concatenate([tgt[:300], tgt[:300]]).copy()
    out[:300, 0] = lo[0] - np.float32(0.03)
    out[300:, 2] = hi[2] + np.float32(1.0)
    _check_nearest(dev, out, tgt, md)
    far = (src + np.float32(50.0)).astype(np.float32)
    assert _check_nearest(dev, far, tgt, md) == 0
    # an empty target
    assert _check_nearest(dev, src[:100], np.zeros((0, 3), np.float32), md) == 0
    # points on cell boundaries: a lattice of pitch = the cell edge from the box's corner, queries on and next to the planes
    edge = md * pc.EDGE_MARGIN
    ax = np.arange(12) * edge
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    g = np.random.default_rng(0)
    q = np.concatenate([lat, lat + g.normal(0, 1e-7, lat.shape).astype(np.float32), lat + np.float32(0.5 * edge)])
    assert _check_nearest(dev, q.astype(np.float32), lat, md) > 0
    # a cell cap small enough to force a larger edge
    for cap in (1, 64, 4096):
        assert _check_nearest(dev, src, tgt, md, max_cells=cap) == _check_nearest(dev, src, tgt, md)


# -------------------------------------------------------------------------------------------------------------- 3. normals
def _angles(a, b):
    c = np.cross(a, b)
    return np.arcsin(np.minimum(1.0, np.sqrt((c * c).sum(1))))


def _check_normals(dev, pts, label, max_cells=None, ref=None):
    want, nb, ev = ref if ref is not None else R.normals_cpu(pts)
    got, gnb = pc.normals_enqueue(_t(pts, dev), max_cells=max_cells, neighbours=True)
    got, gnb = got.cpu().numpy(), gnb.cpu().numpy().astype(np.int64)
    k = nb.shape[1]
    assert np.array_equal(gnb[:, :k], nb), f"{label}: {np.count_nonzero((gnb[:, :k] != nb).any(1))} neighbour lists differ"
    assert np.all(gnb[:, k:] == -1)
    assert np.all(np.isfinite(got)) and np.all(np.abs(np.linalg.norm(got, axis=1) - 1.0) < 1e-12)
    if len(pts) < 3:
        assert np.array_equal(got, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
        return 0.0
    gated = (ev[:, 1] - ev[:, 0]) >= 1e-3 * ev[:, 2]
    worst = float(_angles(got[gated], want[gated]).max()) if gated.any() else 0.0
    print(f"normals {label}: n {len(pts)} gated {int(gated.sum())} max angle {worst:.3e} rad")
    assert worst <= NORMAL_ANGLE_GATE, f"{label}: {worst:.3e} rad"
    return worst


@pytest.mark.parametrize("name", ["room_300k", "room_100k", "room_30k", "synth"])
def test_normals_equal_the_restatement(dev, name):
    _, tgt, _, n, nb, ev = _case(name)
    _check_normals(dev, tgt, name, ref=(n, nb, ev))


def test_normals_special_cases(dev):
    """Measured on an MI355X over this test and test_normals_equal_the_restatement: the largest angle to numpy's eigenvector is
    9.9e-15 rad (the first 3 points of the room; 2.4e-15 on the 300 000-point room, 0 on the lattice wall); gate = 10 x that."""
    # a noise-free fronto-parallel wall on a lattice: ranks 30 and 31 sit in shells of equal distance
    wall = R.wall_points()
    _check_normals(dev, wall, "wall")
    got = pc.estimate_normals(_t(wall, dev)).cpu().numpy()
    assert np.all(np.abs(np.abs(got[:, 2]) - 1.0) < 1e-12)
    tgt = _case("room_30k")[1]
    for n in (1, 2, 3, 29, 30, 31, 1000):
        _check_normals(dev, tgt[:n], f"first {n}")
    for cap in (1, 8, 512):                      # the edge grows; the result does not move
        _check_normals(dev, tgt[:5000], f"cap {cap}", max_cells=cap)
    same = np.tile(tgt[:1], (40, 1))             # coincident points: no direction
    got = pc.estimate_normals(_t(same, dev)).cpu().numpy()
    assert np.array_equal(got, np.tile([0.0, 0.0, 1.0], (40, 1)))
    assert pc.estimate_normals(_t(np.zeros((0, 3), np.float32), dev)).shape == (0, 3)


# ------------------------------------------------------------------------------------- 4. icp on the restatement's normals
@pytest.mark.parametrize("name", ICP_CASES)
def test_registration_equals_the_restatement(dev, name):
    src, tgt, md, normals = _case(name)[:4]
    want = R.icp_cpu(src, tgt, normals, md)
    s, t, nn = _t(src, dev), _t(tgt, dev), _t(normals, dev, torch.float64)
    first = pc.registration_icp(s, t, nn, md, max_iteration=0)
    j0, _ = R.nearest_cpu(np.asarray(src, np.float64), tgt, md)
    assert first.iterations == 0 and first.n_correspondences == int((j0 >= 0).sum())
    assert np.array_equal(first.correspondence_set.numpy(), np.stack([np.nonzero(j0 >= 0)[0], j0[j0 >= 0]], 1))
    assert torch.equal(first.transformation, torch.eye(4, dtype=torch.float64))
    got = pc.registration_icp(s, t, nn, md)
    amb = sum(want["ambiguous_per_eval"])
    print(name, "iterations", got.iterations, want["iterations"], "pairs", got.n_correspondences, want["n"], "ambiguous", amb,
          "max |dT| %.3e" % np.abs(got.transformation.numpy() - want["transformation"]).max())
    assert torch.isfinite(got.transformation).all()
    assert abs(got.n_correspondences - want["n"]) <= amb
    # the pair count of every evaluation: a loop cut off after k updates ends on evaluation k
    for k, (pairs, a) in enumerate(zip(want["pairs_per_eval"], np.cumsum(want["ambiguous_per_eval"]))):
        cut = pc.registration_icp(s, t, nn, md, max_iteration=k)
        assert cut.iterations == k and abs(cut.n_correspondences - pairs) <= a, (k, cut.n_correspondences, pairs)
    if amb == 0:
        assert got.n_correspondences == want["n"] and got.iterations == want["iterations"] and got.fitness == want["fitness"]
        assert abs(got.inlier_rmse - want["rmse"]) < 1e-12
        assert np.abs(got.transformation.numpy() - want["transformation"]).max() < 1e-9
        jw = want["partner"]
        assert np.array_equal(got.correspondence_set.numpy(), np.stack([np.nonzero(jw >= 0)[0], jw[jw >= 0]], 1))


def test_registration_without_pairs_is_the_identity(dev):
    src, tgt, md, normals = _case("room_1000")[:4]
    far = (src + np.float32(40.0)).astype(np.float32)
    got = pc.registration_icp(_t(far, dev), _t(tgt, dev), _t(normals, dev, torch.float64), md)
    assert got.n_correspondences == 0 and got.iterations == 1 and got.fitness == 0.0 and got.inlier_rmse == 0.0
    assert torch.equal(got.transformation, torch.eye(4, dtype=torch.float64)) and got.correspondence_set.shape == (0, 2)
    empty = pc.registration_icp(_t(src, dev), _t(np.zeros((0, 3), np.float32), dev),
                                torch.zeros(0, 3, dtype=torch.float64, device=dev), md)
    assert empty.n_correspondences == 0 and empty.iterations == 1 and torch.equal(empty.transformation, torch.eye(4, dtype=torch.float64))


# --------------------------------------------------------------------------------------------------- 5. reproducibility
def test_every_output_repeats_bit_for_bit(dev):
    s = R.synth_scene()
    r = s["kf_rows"].shape[1]
    rows, poses = s["kf_rows"].reshape(-1, 7).contiguous().to(dev), s["kf_poses"].to(dev).contiguous()
    a, b = pc.cloud_from_rays(rows, r, poses), pc.cloud_from_rays(rows, r, poses)
    assert a[1] == b[1] and torch.equal(a[0], b[0])
    src, tgt, md = _case("room_30k")[:3]
    sd, td = _t(src, dev), _t(tgt, dev)
    n1, k1 = pc.normals_enqueue(td, neighbours=True)
    n2, k2 = pc.normals_enqueue(td, neighbours=True)
    assert torch.equal(n1.view(torch.int64), n2.view(torch.int64)) and torch.equal(k1, k2)
    r1, p1 = pc.registration_enqueue(sd, td, n1, md)
    r2, p2 = pc.registration_enqueue(sd, td, n1, md)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)) and torch.equal(p1, p2)
    assert float(r1[19]) >= 2 and float(r1[16]) > 0


# ------------------------------------------------------------------------------------------ 6. switch_pose_rectifying
def _scene_on_device(dev):
    s = R.synth_scene()
    k, r = s["kf_rows"].shape[:2]
    db = DeviceRayDB(k + 2, r, dev)
    slots = [k + 1 - i for i in range(k)]          # not the identity: the slots are honoured
    for slot, rows in zip(slots, s["kf_rows"]):
        db.store(slot, rows.to(dev))
    return s, db, slots


def test_switch_pose_rectifying_equals_the_restatement(dev):
    s, db, slots = _scene_on_device(dev)
    cfg = s["cfg"]
    cfg["tracking"]["switch"] = {"lr_rot": 0.001, "lr_trans": 0.001, "map_num": 15}
    st = pc.switch_settings(cfg)
    assert st == {"align_threshold": 0.05, "including_last": 0, "min_correspondence": 2000, "min_trans_dist": 0.5}
    drifted, gt = s["frame_pose_drifted"], s["frame_pose_gt"]
    flag, n, pose = pc.switch_pose_rectifying(db, slots, s["kf_poses"], s["frame_rows"].to(dev), drifted, cfg)
    # the restatement on the device's own clouds, composed the same way
    r = s["kf_rows"].shape[1]
    tgt, _ = pc.cloud_from_rays(s["kf_rows"].reshape(-1, 7).contiguous().to(dev), r, s["kf_poses"].to(dev).contiguous())
    src, _ = pc.cloud_from_rays(s["frame_rows"].to(dev), s["frame_rows"].shape[0], drifted[None].to(dev).contiguous())
    wflag, wn, wpose, _ = R.rectify_cpu(tgt.cpu().numpy(), src.cpu().numpy(), drifted.numpy(), st)
    print("rectify: flag", flag, wflag, "n", n, wn, "max |dpose| %.3e" % np.abs(pose.numpy() - wpose).max())
    assert flag is True and wflag is True and n == wn
    assert pose.dtype == torch.float32 and np.abs(pose.numpy() - wpose).max() <= 2e-6
    err_in = float((drifted[:3, 3] - gt[:3, 3]).norm()), float((drifted[:3, :3] - gt[:3, :3]).norm())
    err_out = float((pose[:3, 3] - gt[:3, 3]).norm()), float((pose[:3, :3] - gt[:3, :3]).norm())
    print("rectify: translation error %.4f -> %.4f m, rotation error %.4f -> %.4f" % (err_in[0], err_out[0], err_in[1], err_out[1]))
    assert err_out[0] < err_in[0] and err_out[1] < err_in[1]
    # below min_correspondence: the input pose, flag False
    cfg["tracking"]["switch"]["min_correspondence"] = n + 1
    f2, n2, p2 = pc.switch_pose_rectifying(db, slots, s["kf_poses"], s["frame_rows"].to(dev), drifted, cfg)
    assert f2 is False and n2 == n and torch.equal(p2, drifted.float())
    # a translation beyond min_trans_dist: accepted, with the identity
    cfg["tracking"]["switch"].update(min_correspondence=2000, min_trans_dist=1e-6)
    f3, n3, p3 = pc.switch_pose_rectifying(db, slots, s["kf_poses"], s["frame_rows"].to(dev), drifted, cfg)
    assert f3 is True and n3 == n and torch.equal(p3, drifted.float())


# ---------------------------------------------------------------------------------------------------------------- 7. runner
def _small_two_room_cfg():
    """the trajectory configuration of tests/test_gpu_sequence.py (config_two_rooms on 160 x 120 images, the reference's cadence)"""
    cfg = synth.config_two_rooms()
    cfg["cam"].update(H=140, W=180, fx=80.0, fy=80.0, cx=89.5, cy=69.5, crop_edge=10)
    cfg["grid"]["hash_size"] = 16
    cfg["mapping"].update(sample=1200, pixels_cur=500, first_iters=300)
    cfg["tracking"].update(sample=600)
    cfg["tracking"]["RO"].update(particle_size=1024, n_rows=12, n_cols=16)
    cfg["tracking"]["RO"].update(initial_scaling_factor=0.02, rescaling_factor=0.5)
    return cfg


def _walk(dev, rectify):
    from mipsfusion_amd import sequence
    from mipsfusion_amd.graph import work_stream
    cfg = _small_two_room_cfg()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    gt, frames, schedule = synth.two_room_sequence(cfg, 300, kf_every=15)
    prev = torch.cuda.current_stream(dev)
    try:
        seq = sequence.GraphedSequence(cfg, dev, frames, kf_every=15, sampler="device", stream=work_stream(dev), schedule=schedule,
                                       deterministic=True, **({"rectify_switch": True} if rectify else {}))
        if rectify:
            # the reduced configuration stores seq.R rays per keyframe, not 30 000: the same share of them must pair
            cfg["tracking"]["switch"]["min_correspondence"] = int(round(2000 / 30000 * seq.R))
        res = seq.run(gt)
    finally:
        torch.cuda.set_stream(prev)
    return seq, res, sequence.summarise(res, gt, cfg, "graphs"), schedule


def test_two_room_walk_with_rectified_switch(dev):
    seq, res, out, schedule = _walk(dev, True)
    backs = [k for k, ev in sorted(schedule.items()) if ev[0] == "back"]
    print({k: out[k] for k in ("ate_rmse_m", "ate_max_m", "switch_frames")}, "rectified", res["rectified"],
          "min_correspondence", seq.cfg["tracking"]["switch"]["min_correspondence"])
    assert sorted(out["switch_frames"]) == sorted(schedule)
    assert len(res["rectified"]) == len(backs) == 1 and res["rectified"] == seq.rectified
    flag, n = res["rectified"][0]
    assert flag is True and n >= seq.cfg["tracking"]["switch"]["min_correspondence"]
    assert out["ate_rmse_m"] < 0.05 and out["ate_max_m"] < 0.30


def test_two_room_walk_without_the_flag_does_not_reach_the_rectification(dev):
    seq, res, out, schedule = _walk(dev, False)
    assert seq.rectify_switch is False and seq.rectified == [] and res["rectified"] == []
    assert sorted(out["switch_frames"]) == sorted(schedule)


# --------------------------------------------------------------------------------------------------------------- 8. capture
def test_registration_replays_from_a_graph_on_new_points(dev):
    src, tgt, md, normals = _case("room_1000")[:4]
    src2 = (src.astype(np.float64) @ R.offset_transform(0.7, 1.0, 11)[:3, :3].T).astype(np.float32)
    s, t, nn = _t(src, dev), _t(tgt, dev), _t(normals, dev, torch.float64)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        pc.registration_enqueue(s, t, nn, md)                      # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        res, partner = pc.registration_enqueue(s, t, nn, md)
    for points in (src2, src):
        s.copy_(_t(points, dev))
        g.replay()
        torch.cuda.synchronize()
        eager_res, eager_partner = pc.registration_enqueue(s, t, nn, md)
        assert torch.equal(res.view(torch.int64), eager_res.view(torch.int64)) and torch.equal(partner, eager_partner)
        assert float(res[19]) >= 2 and float(res[16]) > 0
