"""GPU tests of sub-map management (mipsfusion_amd/submap_manager.py, csrc/submap.hip, C ABI include/mipsf_submap.h) against the
numpy restatement tests/submap_cpu.py and the fixtures recorded from the reference's Manager (tests/golden/submap/*.npz).

The frame statistics are integer counts and float32 minima / maxima formed by the same float32 operations in the same order
(contraction off on both sides): the record is compared word for word, no tolerance.  One exception is stated where it is made:
without a valid pixel the surface box is (+inf, -inf), its centre inf - inf, and the expanded boxes are NaN on both sides -- a
NaN's sign and payload are the processor's, so two NaNs count as equal there."""
import ctypes as C

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, synth
from mipsfusion_amd import submap_manager as sm

from . import submap_cpu as sc
from . import submap_fixtures as sf

pytestmark = pytest.mark.gpu

NEAR, FAR, MIN_CR = 0.0, 5.0, (1.0, 0.5, 0.25)
SHAPES = {                                          # H, W, lattices A / B / C
    "20x28": (20, 28, (6, 8), (3, 4), (4, 6)),       # a lattice smaller than one wave
    "37x53": (37, 53, (10, 13), (5, 7), (6, 8)),     # 1 961 pixels, no multiple of 64
    "154x203": (154, 203, (150, 200), (15, 20), (24, 32)),   # the reference's lattices in the smallest image that holds them
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _pose(yaw=0.35, pitch=-0.08, t=(0.4, 0.0, 0.4)):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = synth.look_rotation(yaw, pitch).numpy()
    m[:3, 3] = t
    return m


def _frame_rows(H, W, pose, seed=3):
    f = synth.render_box_frame(sf.ROOM, torch.from_numpy(pose), H, W, 0.516 * W, 0.516 * W, (W - 1) / 2, (H - 1) / 2, shrink=0.0, seed=seed)
    return sf.rows_of(f).numpy()


def _boxes(kind, rows, pose, H, W, lats):
    """-> (boxes [n,6], max_len [n,3])"""
    s = sc.frame_stats(rows, pose, np.float32([[0, 0, 0, 1, 1, 1]]), np.float32([[9, 9, 9]]), H, W, *lats, NEAR, FAR, MIN_CR)
    surface = np.concatenate(s.surface) if s.n_valid else np.float32([0, 0, -1, 3, 2, 3])
    if kind == "one":
        return (surface * np.float32([1, 1, 1, 0.5, 1.2, 1.2]))[None], np.float32([[3.0, 9, 9]])
    rng = np.random.default_rng(7)
    boxes = np.concatenate([surface[:3] + rng.uniform(-1.5, 1.5, (64, 3)), rng.uniform(0.2, 4.5, (64, 3))], 1).astype(np.float32)
    boxes[0] = surface                               # the frame's own box: its extreme points lie ON the faces and are outside
    boxes[1] = np.float32([50, 50, 50, 1, 1, 1])     # holds nothing
    max_len = (boxes[:, 3:] * rng.uniform(0.8, 2.0, (64, 3))).astype(np.float32)
    return boxes, max_len


def _depths(kind, rows):
    rows = rows.copy()
    if kind == "zero":
        rows[:, 6] = 0.0
    elif kind == "beyond_far":
        rows[:, 6] = 100.0
    elif kind == "one_valid":
        keep = rows[len(rows) // 2 + 3, 6]
        rows[:, 6] = 0.0
        rows[len(rows) // 2 + 3, 6] = keep if keep > 0 else 2.0
    return rows


def _canonical(words, n):
    """NaNs of the float fields made one NaN (see the module's docstring)"""
    w = words.copy()
    fields = list(range(1, 7)) + [16 + 12 * i + j for i in range(n) for j in range(6)]
    f = w[fields].view(np.float32)
    w[fields] = np.where(np.isnan(f), np.uint32(0x7FC00000), w[fields])
    return w


def _gpu_words(dev, rows, pose, boxes, max_len, H, W, lats, out=None):
    t = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for v in (rows, pose, boxes, max_len)]
    out = sm.frame_stats_enqueue(*t, H, W, *lats, NEAR, FAR, MIN_CR, out=out)
    return out[0].cpu().numpy().view(np.uint32), out


@pytest.mark.parametrize("depths", ["frame", "zero", "beyond_far", "one_valid"])
@pytest.mark.parametrize("boxes", ["one", "sixty_four"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_stats_equal_the_restatement_word_for_word(dev, shape, boxes, depths):
    H, W, *lats = SHAPES[shape]
    pose = _pose()
    rows = _depths(depths, _frame_rows(H, W, pose))
    bx, mx = _boxes(boxes, rows, pose, H, W, lats)
    want = sc.frame_stats(rows, pose, bx, mx, H, W, *lats, NEAR, FAR, MIN_CR)
    got, _ = _gpu_words(dev, rows, pose, bx, mx, H, W, lats)
    n = len(bx)
    got, ref = got[:16 + 12 * n], sc.stats_to_words(want)
    if depths in ("zero", "beyond_far"):
        assert want.n_valid == 0 and got[0] == 0
        assert np.isposinf(got[1:4].view(np.float32)).all() and np.isneginf(got[4:7].view(np.float32)).all()
        got, ref = _canonical(got, n), _canonical(ref, n)
    else:
        assert want.n_valid == (1 if depths == "one_valid" else want.n_valid) and want.n_valid > 0
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"words {bad[:10].tolist()}: {got[bad[:10]].tolist()} != {ref[bad[:10]].tolist()}"
    if boxes == "sixty_four" and depths == "frame":
        assert want.a_clamped[1] == 0 and want.a_expanded[1] >= 0 and want.b_raw[1] == 0          # the box that holds nothing
        assert want.a_clamped.max() > 0 and len({sc.case_of(c, a) for c in want.cases for a in range(3)}) >= 4


# ------------------------------------------------------------------------------------------------------------- overlap
OH, OW, OLAT, KF_LAT = 96, 128, (24, 32), (12, 16)
OK_INTR, OCAM = (66.0, 66.0, 63.5, 47.5), (128.0, 96.0)


@pytest.fixture(scope="module")
def overlap_case():
    pose = _pose()
    rows = _frame_rows(OH, OW, pose)
    rng = np.random.default_rng(11)
    poses, table = [], []
    for j in range(24):
        p = _pose(0.35 + rng.uniform(-0.3, 0.3), -0.08 + rng.uniform(-0.1, 0.1), (0.4 + rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2),
                                                                                  0.4 + rng.uniform(-0.5, 0.5)))
        table.append(_frame_rows(OH, OW, p, seed=20 + j)[sc.lattice_pixels(OH, OW, *KF_LAT)])
        if j == 5:
            p = _pose(0.0, 0.0, (0.4, 0.0, -3.5))                # beyond the wall z = -3, looking away: every point is behind it
        poses.append(p)
    s = sc.frame_stats(rows, pose, np.float32([[0, 0, 0, 1, 1, 1]]), np.float32([[9, 9, 9]]), OH, OW, (8, 8), (4, 4), OLAT, NEAR, FAR, MIN_CR)
    c, l = s.surface                                             # the half of the surface box with the smaller x, a little wider elsewhere
    box = np.concatenate([c - np.float32([0.25, 0, 0]) * l, l * np.float32([0.5, 1.1, 1.1])])
    return pose, rows, np.stack(poses), np.stack(table), box


def _overlap_gpu(dev, case, related=None, top=None, out=None):
    pose, rows, poses, table, box = case
    kw = {}
    if related is not None:
        kw.update(table=torch.from_numpy(table).to(dev), related_slots=torch.tensor(related, dtype=torch.int32, device=dev),
                  related_poses=torch.from_numpy(poses[np.clip(related, 0, 23)]).to(dev))
    if top is not None:
        kw.update(top_poses=torch.from_numpy(poses[top]).to(dev))
    return sm.overlap_enqueue(torch.from_numpy(rows).to(dev), torch.from_numpy(pose).to(dev), OH, OW, OLAT, OK_INTR, OCAM, box, out=out, **kw)


@pytest.mark.parametrize("related", [[3], list(range(1, 24))], ids=["n1", "n23"])
def test_overlap_distances(dev, overlap_case, related):
    pose, rows, poses, table, box = overlap_case
    want = sc.overlap_distances(rows, pose, OH, OW, OLAT, table, related, poses[related])
    got = _overlap_gpu(dev, overlap_case, related=related)["dist"].cpu().numpy()
    assert np.isfinite(want).all() and (np.abs(got - want) <= 1e-6 * np.maximum(1.0, want)).all(), np.abs(got - want).max()


def test_overlap_slot_outside_the_table_is_nan(dev, overlap_case):
    got = _overlap_gpu(dev, overlap_case, related=[2, 24, -1])["dist"].cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2])


@pytest.mark.parametrize("top", [[7], list(range(10)), [5]], ids=["k1", "k10", "behind"])
def test_overlap_masks_equal_the_restatement(dev, overlap_case, top):
    pose, rows, poses, table, box = overlap_case
    want = sc.overlap_masks(rows, pose, OH, OW, OLAT, poses[top], box, *OK_INTR, *OCAM)
    got = {k: v.cpu().numpy() for k, v in _overlap_gpu(dev, overlap_case, top=top).items()}
    assert np.array_equal(got["top_kf_masks"].astype(bool), want["top_kf_masks"])
    assert np.array_equal(got["mask_final"].astype(bool), want["mask_final"])
    assert int(got["count"][0]) == want["count"]
    assert np.array_equal(got["target_d"].view(np.uint32), want["target_d"].view(np.uint32))
    assert np.array_equal(got["rays_d_cam"].view(np.uint32), want["rays_d_cam"].view(np.uint32))
    if top == [5]:
        assert want["count"] == 0 and not want["top_kf_masks"].any()
    else:
        assert 0 < want["count"] < OLAT[0] * OLAT[1]


# ------------------------------------------------------------------------------------------------------------- the manager
@pytest.mark.parametrize("path", sf.fixtures("branch"), ids=lambda p: p.rsplit("/", 1)[-1][:-4])
def test_manager_on_the_device_reproduces_branch_fixture(dev, path):
    fx = sf.load(path)
    m, d, stub = sf.run_branch(fx, "hip", dev)
    sf.check_branch(fx, m, d, stub)
    mc, dc, _ = sf.run_branch(fx, "cpu")
    assert np.array_equal(sc.stats_to_words(d.stats), sc.stats_to_words(dc.stats))
    for a, b in zip(m.dump_state().values(), mc.dump_state().values()):
        assert np.array_equal(a, b)
    if d.overlap is not None:
        for k in ("mask_final", "top_kf_masks", "kf_ids", "target_d", "rays_d_cam"):
            assert np.array_equal(d.overlap[k], dc.overlap[k]), k


@pytest.mark.parametrize("path", sf.fixtures("walk"), ids=lambda p: p.rsplit("/", 1)[-1][:-4])
def test_manager_on_the_device_reproduces_walk(dev, path):
    fx = sf.load(path)
    schedule, trace, m = sf.run_walk(fx, "hip", dev)
    sf.check_walk(fx, schedule, trace, m)
    _, trace_cpu, mc = sf.run_walk(fx, "cpu")
    for d, dc in zip(trace, trace_cpu):
        assert np.array_equal(sc.stats_to_words(d.stats), sc.stats_to_words(dc.stats)), d.keyframe
    assert np.array_equal(m.dump_state()["table"], mc.dump_state()["table"])


def test_default_rectification_runs_on_the_device(dev):
    """the branch that switches back, with the ICP of mipsfusion_amd.pose_corrector where the fixtures put a stub: it either
    accepts (then the pose stays within the ICP's own 0.2 m gate of where it started) or finds too few pairs and opens a sub-map"""
    fx = sf.load([p for p in sf.fixtures("branch") if p.endswith("branch_switch_to_prev.npz")][0])
    m = sm.SubmapManager(sf.config(fx["spec"]["cfg"]), sf.H, sf.W, sf.INTRINSICS, device=dev, max_keyframes=32)
    m.load_state(sf.state_of(fx))
    rows = sf.rows_of(sf.box_frame(fx["pose_world"], fx["spec"]["seed"], fx["spec"]["frame_id"])).to(dev)
    d = m.process_keyframe(rows, fx["pose_local"], fx["spec"]["frame_id"])
    assert (d.flag, d.label) in ((1, "switch to prev"), (3, "wait loop, new localMLP"))
    if d.flag == 1:
        assert d.rectified_pose.shape == (4, 4) and np.isfinite(d.rectified_pose).all()
        assert np.linalg.norm(d.rectified_pose[:3, 3] - fx["e_rectified"][:3, 3]) < 0.2 + 1e-4


# ------------------------------------------------------------------------------------------------------------- capture
def test_both_calls_capture_and_replay(dev, overlap_case):
    H, W, *lats = SHAPES["37x53"]
    pose = _pose()
    rows = _frame_rows(H, W, pose)
    bx, mx = _boxes("sixty_four", rows, pose, H, W, lats)
    direct, _ = _gpu_words(dev, rows, pose, bx, mx, H, W, lats)
    again, _ = _gpu_words(dev, rows, pose, bx, mx, H, W, lats)
    assert direct.tobytes() == again.tobytes()
    top, related = list(range(10)), list(range(1, 24))
    o_direct = {k: v.cpu().numpy() for k, v in _overlap_gpu(dev, overlap_case, related=related, top=top).items()}
    o_again = {k: v.cpu().numpy() for k, v in _overlap_gpu(dev, overlap_case, related=related, top=top).items()}
    assert all(o_direct[k].tobytes() == o_again[k].tobytes() for k in o_direct)

    t = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for v in (rows, pose, bx, mx)]
    o_pose, o_rows, o_poses, o_table, o_box = overlap_case
    ot = {"rows": torch.from_numpy(o_rows).to(dev), "pose": torch.from_numpy(o_pose).to(dev), "table": torch.from_numpy(o_table).to(dev),
          "slots": torch.tensor(related, dtype=torch.int32, device=dev), "rel": torch.from_numpy(o_poses[related]).to(dev),
          "top": torch.from_numpy(o_poses[top]).to(dev)}

    def both(out_s=None, out_o=None):
        out_s = sm.frame_stats_enqueue(*t, H, W, *lats, NEAR, FAR, MIN_CR, out=out_s)
        out_o = sm.overlap_enqueue(ot["rows"], ot["pose"], OH, OW, OLAT, OK_INTR, OCAM, o_box, table=ot["table"], related_slots=ot["slots"],
                                   related_poses=ot["rel"], top_poses=ot["top"], out=out_o)
        return out_s, out_o
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        out_s, out_o = both()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):          # one stream, one chain of launches: no parallel branches
        both(out_s, out_o)
    for _ in range(2):
        out_s[0].fill_(-1)
        for v in out_o.values():
            v.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert out_s[0].cpu().numpy().view(np.uint32).tobytes() == direct.tobytes()
        assert all(out_o[k].cpu().numpy().tobytes() == o_direct[k].tobytes() for k in o_direct)


# ------------------------------------------------------------------------------------------------------------- refusals
def _stats_args(dev, keep, **over):
    H, W = 20, 28
    keep += [torch.zeros(H * W, 7, device=dev), torch.eye(4, device=dev), torch.ones(70, 6, device=dev), torch.ones(70, 3, device=dev),
             torch.full((_lib.SUBMAP_RECORD_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
             torch.zeros(_lib.SUBMAP_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)]
    rows, pose, boxes, max_len, record, ws = keep[-6:]
    kw = dict(H=H, W=W, n_boxes=2, lat_a_h=6, lat_a_w=8, lat_b_h=3, lat_b_w=4, lat_c_h=4, lat_c_w=6, near=0.0, far=5.0,
              rows=rows.data_ptr(), pose=pose.data_ptr(), boxes=boxes.data_ptr(), max_len=max_len.data_ptr(), record=record.data_ptr(),
              workspace=ws.data_ptr())
    kw.update(over)
    return _lib.SubmapFrameStatsArgs.new(**kw), record


@pytest.mark.parametrize("over", [dict(lat_a_h=21), dict(lat_b_w=29), dict(lat_c_h=21), dict(n_boxes=0), dict(n_boxes=65), dict(rows=None),
                                  dict(pose=None), dict(boxes=None), dict(max_len=None), dict(record=None), dict(workspace=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_frame_stats_refusals(dev, over):
    keep = []
    a, record = _stats_args(dev, keep, **over)
    rc = _lib.lib().mipsf_submap_frame_stats(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and len(_lib.lib().mipsf_last_error()) > 10
    assert bool((record == 0x5A5A5A5A).all()), "a refused call wrote to its record"


def _overlap_args(dev, keep, **over):
    P = 24
    keep += [torch.zeros(20 * 28, 7, device=dev), torch.eye(4, device=dev), torch.zeros(4, 12, 7, device=dev),
             torch.zeros(3, dtype=torch.int32, device=dev), torch.eye(4, device=dev).repeat(12, 1, 1).contiguous(),
             torch.full((3,), 5.0, dtype=torch.float64, device=dev), torch.full((12, P), 9, dtype=torch.uint8, device=dev),
             torch.full((P,), 9, dtype=torch.uint8, device=dev), torch.full((1,), 9, dtype=torch.int32, device=dev),
             torch.full((P,), 9.0, device=dev), torch.full((P, 3), 9.0, device=dev)]
    rows, pose, table, slots, poses, dist, masks, final, count, td, rd = keep[-11:]
    kw = dict(H=20, W=28, lat_h=4, lat_w=6, n_related=3, k=2, n_slots=4, rows_per_slot=12, fx=14.0, fy=14.0, cx=13.5, cy=9.5, cam_W=28.0,
              cam_H=20.0, edge=2.0, rows=rows.data_ptr(), pose=pose.data_ptr(), table=table.data_ptr(), related_slots=slots.data_ptr(),
              related_poses=poses.data_ptr(), dist=dist.data_ptr(), top_poses=poses.data_ptr(), top_kf_masks=masks.data_ptr(),
              mask_final=final.data_ptr(), count=count.data_ptr(), target_d=td.data_ptr(), rays_d_cam=rd.data_ptr())
    kw.update(over)
    return _lib.SubmapOverlapArgs.new(**kw), (dist, masks, final, count, td, rd)


@pytest.mark.parametrize("over", [dict(lat_h=21), dict(lat_w=29), dict(k=11), dict(n_related=0, k=0), dict(rows=None), dict(pose=None),
                                  dict(table=None), dict(related_slots=None), dict(related_poses=None), dict(dist=None), dict(top_poses=None),
                                  dict(top_kf_masks=None), dict(mask_final=None), dict(count=None), dict(target_d=None),
                                  dict(rays_d_cam=None)], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_overlap_refusals(dev, over):
    keep = []
    a, outs = _overlap_args(dev, keep, **over)
    rc = _lib.lib().mipsf_submap_overlap(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and len(_lib.lib().mipsf_last_error()) > 10
    dist, masks, final, count, td, rd = outs
    assert bool((dist == 5.0).all()) and bool((masks == 9).all()) and bool((final == 9).all()) and int(count[0]) == 9
    assert bool((td == 9.0).all()) and bool((rd == 9.0).all()), "a refused call wrote to its outputs"


def test_python_layer_refuses_what_the_library_refuses(dev):
    with pytest.raises(ValueError, match="lattice A"):
        sm.SubmapManager(sf.config(), 100, 203, sf.INTRINSICS, device=dev, rectify=sf.StubRectify(True))
    rows = torch.zeros(20 * 28, 7, device=dev)
    with pytest.raises(RuntimeError, match="sub-maps"):
        sm.frame_stats_enqueue(rows, torch.eye(4, device=dev), torch.ones(65, 6, device=dev), torch.ones(65, 3, device=dev), 20, 28, (6, 8),
                               (3, 4), (4, 6), 0.0, 5.0, (1, 1, 1))
