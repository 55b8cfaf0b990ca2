"""CPU tests of sub-map management: the numpy restatement of the statistics kernels against the reference's own
Manager functions, the expand rule (one header for device and host) against ``localMLP_expand_rule``, and
``SubmapManager(backend="cpu")`` against the recorded fixtures tests/golden/submap/*.npz (tests/golden/make_submap_golden.py)."""
import types

import numpy as np
import pytest
import torch

from mipsfusion_amd.helper_functions import sampling_helper
from mipsfusion_amd.submap_manager import derive_schedule
from oracle import ref_import

from . import submap_cpu as sc
from . import submap_fixtures as sf

needs_reference = pytest.mark.skipif(not ref_import.available(), reason="the reference tree is not present")
BRANCHES, WALKS = sf.fixtures("branch"), sf.fixtures("walk")


def _name(path):
    return path.rsplit("/", 1)[-1][:-4]


def test_the_fixtures_are_there():
    labels = {sf.load(p)["spec"]["label"] for p in BRANCHES}
    assert labels == set(sf.LABELS)
    assert len(WALKS) == 2


# ------------------------------------------------------------------------------------------------------------- lattice
@pytest.mark.parametrize("H,W", [(5, 7), (20, 28), (37, 53), (154, 203)])
def test_lattice_is_sample_pixels_uniformly(H, W):
    for nh in sorted({1, 2, 3, H // 2, H - 1, H}):
        for nw in sorted({1, 2, 5, W // 3, W - 1, W}):
            if not (1 <= nh <= H and 1 <= nw <= W):
                continue
            r, c = sampling_helper.sample_pixels_uniformly(H, W, nh, nw)
            rr, cc = sc.lattice(H, W, nh, nw)
            assert np.array_equal(rr, r.numpy()) and np.array_equal(cc, c.numpy()), (nh, nw)
            assert rr.max() < H and cc.max() < W and rr.min() >= 0 and cc.min() >= 0
    with pytest.raises(ValueError):
        sc.lattice(H, W, H + 1, 1)


@needs_reference
def test_lattice_is_the_references():
    ref = ref_import.load().sampling_helper
    for H, W, nh, nw in [(154, 203, 150, 200), (154, 203, 15, 20), (154, 203, 24, 32), (20, 28, 20, 28), (37, 53, 10, 13)]:
        r, c = ref.sample_pixels_uniformly(H, W, nh, nw)
        rr, cc = sc.lattice(H, W, nh, nw)
        assert np.array_equal(rr, r.numpy()) and np.array_equal(cc, c.numpy())


# ------------------------------------------------------------------------------------------------------------- expand rule
def _random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    c, l = rng.uniform(-2, 2, (n, 3)), rng.uniform(0.5, 4, (n, 3))
    kc, kl = c + rng.uniform(-2, 2, (n, 3)), rng.uniform(0.3, 5, (n, 3))
    nested = rng.random(n) < 0.1                          # a tenth lie inside on all faces
    kc[nested], kl[nested] = c[nested] + 0.1 * l[nested] * rng.uniform(-1, 1, (int(nested.sum()), 3)), 0.5 * l[nested]
    mx = l * rng.uniform(0.8, 2.5, (n, 3))
    return [v.astype(np.float32) for v in (c, l, kc, kl, mx)]


@needs_reference
def test_expand_rule_is_the_references_bit_for_bit():
    ref_import.load()
    import Manager as upstream
    c, l, kc, kl, mx = _random_boxes(1000, 5)
    seen = np.zeros(6, np.int64)
    for i in range(1000):
        want_c, want_l = upstream.Manager.localMLP_expand_rule(None, *(torch.from_numpy(v[i]) for v in (c, l, kc, kl, mx)))
        got, cases = sc.expand_rule(np.concatenate([c[i], l[i]]), np.concatenate([kc[i], kl[i]]), mx[i])
        want = np.concatenate([want_c.numpy(), want_l.numpy()])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, got, want, [sc.case_of(cases, a) for a in range(3)])
        for a in range(3):
            seen[sc.case_of(cases, a)] += 1
    assert (seen > 0).all(), dict(zip(sc.CASE_NAMES, seen.tolist()))


def test_expand_rule_cases_by_hand():
    big = np.float32([10, 10, 10])
    box = np.float32([0, 0, 0, 2, 2, 2])
    out, cases = sc.expand_rule(box, np.float32([0, 0, 0, 1, 1, 1]), big)
    assert cases == 0 and np.array_equal(out, box)
    out, cases = sc.expand_rule(box, np.float32([1, 0, 0, 2, 1, 1]), np.float32([2.5, 10, 10]))       # reaches x = 2, may reach 1.5
    assert sc.case_of(cases, 0) == 3 and out[3] == 2.5 and out[0] == 0.25
    out, cases = sc.expand_rule(box, np.float32([-1, 0, 0, 2, 1, 1]), np.float32([2.5, 10, 10]))
    assert sc.case_of(cases, 0) == 4 and out[3] == 2.5 and out[0] == -0.25
    out, cases = sc.expand_rule(box, np.float32([0, 0, 0, 6, 1, 1]), np.float32([3, 10, 10]))         # 2 on either side, room for 1
    assert sc.case_of(cases, 0) == 5 and out[3] == 3 and out[0] == 0
    out, cases = sc.expand_rule(box, np.float32([0, 0, 0, 6, 1, 1]), np.float32([2, 10, 10]))
    assert sc.case_of(cases, 0) == 1 and out[3] == 2


# ------------------------------------------------------------------------------------------------------------- restatement
def _frame_and_state(path):
    fx = sf.load(path)
    frame = sf.box_frame(fx["pose_world"], fx["spec"]["seed"], fx["spec"]["frame_id"])
    return fx, frame, sf.config(fx["spec"]["cfg"])


@needs_reference
@pytest.mark.parametrize("path", BRANCHES, ids=_name)
def test_restatement_is_the_references_functions(path):
    """surface box, every containing ratio (clamped and expanded) and the lattice-B scores, bit for bit"""
    ref = ref_import.load()
    import Manager as upstream
    fx, frame, cfg = _frame_and_state(path)
    boxes, max_len, pose = fx["s_boxes"], fx["s_max_len"], fx["pose_world"]
    m = cfg["mapping"]
    s = sc.frame_stats(sf.rows_of(frame).numpy(), pose, boxes, max_len, sf.H, sf.W, (150, 200), (15, 20),
                       (m["overlapping"]["n_rays_h"], m["overlapping"]["n_rays_w"]), cfg["cam"]["near"], cfg["cam"]["far"], m["min_cr_localMLP_len"])
    tp, depth, dirs = torch.from_numpy(pose), frame["depth"], frame["direction"]
    c, l = ref.geometry_helper.get_frame_surface_bbox(tp, depth, dirs, cfg["cam"]["near"], cfg["cam"]["far"])
    assert np.array_equal(np.concatenate(s.surface).view(np.uint32), np.concatenate([c.numpy(), l.numpy()]).view(np.uint32))
    info = torch.cat([torch.ones(len(boxes), 1), torch.from_numpy(boxes)], 1)
    me = types.SimpleNamespace(dataset=types.SimpleNamespace(H=sf.H, W=sf.W), kfSet=types.SimpleNamespace(localMLP_info=info),
                               min_cr_localMLP_len=torch.tensor(m["min_cr_localMLP_len"]))
    with np.errstate(invalid="ignore"):
        for i in range(len(boxes)):
            want = upstream.Manager.compute_containing_ratio(me, depth, dirs, tp, i).numpy()
            assert np.float32(s.a_clamped[i]) / np.float32(s.a_valid) == want
            ec, el = upstream.Manager.localMLP_expand_rule(None, info[i, 1:4], info[i, 4:7], c, l, torch.from_numpy(max_len[i]))
            assert np.array_equal(s.expanded[i].view(np.uint32), torch.cat([ec, el]).numpy().view(np.uint32))
            want = upstream.Manager.compute_containing_ratio(me, depth, dirs, tp, i, localMLP_center=ec, localMLP_len=el).numpy()
            assert np.float32(s.a_expanded[i]) / np.float32(s.a_valid) == want
    # find_highest_containing_ratio's scores (it returns only the winner): its own steps, written out
    r, cc = ref.sampling_helper.sample_pixels_uniformly(sf.H, sf.W, 15, 20)
    d_w = torch.sum(dirs[r, cc][..., None, :] * tp[None, :3, :3], -1)
    pts = tp[:3, -1].repeat(300, 1) + d_w * depth[r, cc][:, None]
    lo, hi = info[:, 1:4] - 0.5 * info[:, 4:7], info[:, 1:4] + 0.5 * info[:, 4:7]
    score = torch.count_nonzero(ref.geometry_helper.pts_in_bbox(pts, lo, hi), dim=0)
    assert np.array_equal(s.b_raw, score.numpy())
    ids = torch.arange(len(boxes))
    assert int(upstream.Manager.find_highest_containing_ratio(me, depth, dirs, tp, ids)) == int(np.argsort(-s.b_raw, kind="stable")[0])


def test_record_words_round_trip():
    fx, frame, cfg = _frame_and_state(BRANCHES[0])
    m = cfg["mapping"]
    s = sc.frame_stats(sf.rows_of(frame).numpy(), fx["pose_world"], fx["s_boxes"], fx["s_max_len"], sf.H, sf.W, (150, 200), (15, 20), (24, 32),
                       cfg["cam"]["near"], cfg["cam"]["far"], m["min_cr_localMLP_len"])
    w = sc.stats_to_words(s)
    assert len(w) == 16 + 12 * len(fx["s_boxes"])
    assert np.array_equal(sc.stats_to_words(sc.stats_from_words(w)), w)


def test_tree_sum_is_a_sum():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 257, 768, 1000):
        v = rng.normal(size=(n, 3))
        assert np.allclose(sc.tree_sum(v), v.sum(0), rtol=1e-13, atol=1e-13)


def test_no_valid_pixel_is_refused():
    fx, frame, cfg = _frame_and_state(BRANCHES[0])
    m, _ = sf.manager_for(fx, "cpu")
    m.load_state(sf.state_of(fx))
    rows = sf.rows_of(frame).clone()
    rows[:, 6] = 100.0
    with pytest.raises(ValueError, match="no pixel"):
        m.process_keyframe(rows, fx["pose_local"], fx["spec"]["frame_id"])


def test_more_than_64_submaps_are_refused():
    fx, frame, cfg = _frame_and_state(BRANCHES[0])
    m, _ = sf.manager_for(fx, "cpu")
    m.load_state(sf.state_of(fx))
    while m.n_submaps < 64:
        m._new_submap(np.float32([0, 0, 0, 1, 1, 1]), 0)
    assert m.n_submaps == 64
    with pytest.raises(RuntimeError, match="at most 64"):
        m._new_submap(np.float32([0, 0, 0, 1, 1, 1]), 0)


# ------------------------------------------------------------------------------------------------------------- the manager
@pytest.mark.parametrize("path", BRANCHES, ids=_name)
def test_manager_reproduces_branch_fixture(path):
    fx = sf.load(path)
    m, d, stub = sf.run_branch(fx, "cpu")
    sf.check_branch(fx, m, d, stub)


@pytest.fixture(scope="module")
def walks():
    return {p: (sf.load(p),) + tuple(sf.run_walk(sf.load(p), "cpu")) for p in WALKS}


@pytest.mark.parametrize("path", WALKS, ids=_name)
def test_manager_reproduces_walk(path, walks):
    fx, schedule, trace, m = walks[path]
    sf.check_walk(fx, schedule, trace, m)


@pytest.mark.parametrize("path", WALKS, ids=_name)
def test_bindings_feed_the_pose_graph(path, walks):
    from mipsfusion_amd import pose_graph
    fx, schedule, trace, m = walks[path]
    pairs, participants = pose_graph.adjacent_pairs(m.bindings())
    assert {tuple(p) for p in pairs.tolist()} == m.adjacent
    assert set(schedule) == {d.keyframe * 15 for d in trace if d.flag != 2}
