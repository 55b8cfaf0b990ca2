"""GPU tests of the tracker's colour registration (mipsfusion_amd/tsdf.py: TSDFVolume.track(rgb=...), tsdf_odometry(color_weight=...);
csrc/track_color.hip) against the float64 restatement of tests/track_color_cpu.py.  The device and the restatement get the same
fp32 words and evaluate the same float64 expressions, so the geometric pair sets, the photometric row sets and the counts are
compared for EQUALITY; tests/test_track_color_cpu.py asserts, on the same cases, that no pixel lies within rounding of a decision."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, tsdf

from . import track_color_cpu as CC
from . import track_cpu as TC
from . import tsdf_cpu as T
from .test_track_color_cpu import CORNER_MARGIN, DEFAULT_WEIGHT, QUARTER, REGISTER_COLOR_REFUSALS, _ids, _register_color_block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _stub(dev, color=True):
    return tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (2, 2, 2), 0.4, color=color, device=dev)      # only its device is used: the model is given


def _kw(c, kw):
    out = dict(c["kw"], **kw)
    out.setdefault("color_weight", DEFAULT_WEIGHT)
    return out


def _register(dev, c, partner=True, **kw):
    model = tsdf.Raycast(_t(c["model_depth"], dev)[None], _t(c["model_normals"], dev)[None], _t(c["model_color"], dev)[None], None)
    return _stub(dev).track_enqueue(_t(c["live"], dev), c["K"], _t(c["pose_init"], dev), _t(c["pose_ref"], dev), model, c["max_dist"],
                                    depth_max=c["depth_max"], partner=partner, rgb=_t(c["live_color"], dev), **_kw(c, kw))


def _read(result):
    r = result.cpu().numpy()
    assert r.shape == (CC.RESULT_DOUBLES,)
    return {"transformation": r[:16].reshape(4, 4), "n": int(r[16]), "fitness": float(r[17]), "rmse": float(r[18]), "iterations": int(r[19]),
            "n_color": int(r[20]), "color_rmse": float(r[21])}


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(a), abs(b))


# ------------------------------------------------------------------------------------------------------------- 5. the restatement
@pytest.mark.parametrize("name", CC.CASES)
def test_colour_registration_equals_the_restatement(dev, name):
    c = CC.case(name)
    want, w0 = CC.want(name, **_kw(c, {})), CC.want(name, **_kw(c, {"max_iteration": 0}))
    result, pose, partner, rows = _register(dev, c, max_iteration=0)
    first = _read(result)
    assert first["iterations"] == 0 and first["n"] == w0["n"] and first["n_color"] == w0["n_color"]
    assert np.array_equal(partner.cpu().numpy().reshape(-1), w0["partner"]) and np.array_equal(rows.cpu().numpy().reshape(-1) != 0, w0["color_row"])
    assert _close(first["color_rmse"], w0["color_rmse"]) and np.array_equal(pose.cpu().numpy(), c["pose_init"])
    result, pose, partner, rows = _register(dev, c)
    got = _read(result)
    amb = sum(want["ambiguous_per_eval"])
    print(name, "iterations", got["iterations"], want["iterations"], "pairs", got["n"], want["n"], "rows", got["n_color"], want["n_color"], "ambiguous", amb,
          "max |dT| %.3e" % np.abs(got["transformation"] - want["transformation"]).max(), "rmse difference %.3e" % abs(got["rmse"] - want["rmse"]),
          "colour rmse difference %.3e" % abs(got["color_rmse"] - want["color_rmse"]))
    assert amb == 0 and np.isfinite(got["transformation"]).all()
    # both counts of every evaluation: a loop cut off after k updates ends on evaluation k
    for k, (pairs, nrows) in enumerate(zip(want["pairs_per_eval"], want["rows_per_eval"])):
        cut = _read(_register(dev, c, partner=False, max_iteration=k)[0])
        assert cut["iterations"] == k and cut["n"] == pairs and cut["n_color"] == nrows, (k, cut["n"], pairs, cut["n_color"], nrows)
    assert got["n"] == want["n"] and got["n_color"] == want["n_color"] and got["iterations"] == want["iterations"] and got["fitness"] == want["fitness"]
    assert _close(got["rmse"], want["rmse"]) and _close(got["color_rmse"], want["color_rmse"])
    assert np.abs(got["transformation"] - want["transformation"]).max() < 1e-9
    assert np.array_equal(partner.cpu().numpy().reshape(-1), want["partner"]) and np.array_equal(rows.cpu().numpy().reshape(-1) != 0, want["color_row"])
    assert np.array_equal(pose.cpu().numpy(), got["transformation"].astype(np.float32))
    if name in ("no_model", "image_1x1"):
        assert got["n_color"] == 0 and got["color_rmse"] == 0.0 and got["iterations"] == 1 and np.array_equal(pose.cpu().numpy(), c["pose_init"])


# ------------------------------------------------------------------------------------------------------------- 6. zero weight
@pytest.mark.parametrize("name", sorted(TC.REG_OFFSETS))
def test_zero_weight_gives_the_bytes_of_the_depth_only_kernel(dev, name):
    c = TC.reg_case(name)
    mc, lc = CC.reg_colors(name)
    args = (_t(c["live"], dev), c["K"], _t(c["pose_init"], dev), _t(c["pose_ref"], dev))
    plain = tsdf.Raycast(_t(c["model_depth"], dev)[None], _t(c["model_normals"], dev)[None], None, None)
    coloured = tsdf.Raycast(plain.depth, plain.normals, _t(mc, dev)[None], None)
    r0, p0, m0 = _stub(dev, False).track_enqueue(*args, plain, c["max_dist"], partner=True)
    r1, p1, m1, rows = _stub(dev).track_enqueue(*args, coloured, c["max_dist"], partner=True, rgb=_t(lc, dev), color_weight=0.0,
                                                relative_color_rmse=math.inf)
    assert r0.shape == (20,) and r1.shape == (22,) and float(r0[19]) >= 2 and float(r1[20]) > 0.9 * float(r1[16])
    assert torch.equal(r0.view(torch.int64), r1[:20].view(torch.int64)) and torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(m0, m1)


# ------------------------------------------------------------------------------------------------------------- 7. reproducibility
def test_every_output_repeats_bit_for_bit(dev):
    c = CC.case("two_walls")
    (r1, p1, m1, c1), (r2, p2, m2, c2) = _register(dev, c), _register(dev, c)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert torch.equal(m1, m2) and torch.equal(c1, c2)
    assert float(r1[19]) >= 2 and float(r1[16]) > 0 and float(r1[20]) > 0


def test_colour_registration_replays_from_a_graph_on_a_new_live_frame(dev):
    c = CC.case("corner")
    _, other_color = CC.reg_colors("0.64deg_2.3cm")
    other = TC.reg_case("0.64deg_2.3cm")["live"]                 # another frame against the same model
    vol = _stub(dev)
    model = tsdf.Raycast(_t(c["model_depth"], dev)[None], _t(c["model_normals"], dev)[None], _t(c["model_color"], dev)[None], None)
    live, rgb, init, ref = _t(c["live"], dev), _t(c["live_color"], dev), _t(c["pose_init"], dev), _t(c["pose_ref"], dev)
    run = lambda: vol.track_enqueue(live, c["K"], init, ref, model, c["max_dist"], partner=True, rgb=rgb, color_weight=DEFAULT_WEIGHT)      # noqa: E731
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()                                                    # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        res, pose, partner, rows = run()
    for depth, color in ((other, other_color), (c["live"], c["live_color"])):
        live.copy_(_t(depth, dev)), rgb.copy_(_t(color, dev))
        g.replay()
        torch.cuda.synchronize()
        eager_res, eager_pose, eager_partner, eager_rows = run()
        assert torch.equal(res.view(torch.int64), eager_res.view(torch.int64)) and torch.equal(partner, eager_partner) and torch.equal(rows, eager_rows)
        assert torch.equal(pose.view(torch.int32), eager_pose.view(torch.int32))
        assert float(res[19]) >= 2 and float(res[16]) > 0 and float(res[20]) > 0


# ------------------------------------------------------------------------------------------------------------- 8. the API
@pytest.fixture(scope="module")
def fused(dev):
    """the colour volume of the cases, fused on the device"""
    v = CC.color_volume()
    vol = tsdf.TSDFVolume(v["origin"], v["voxel"], v["dims"], v["trunc"], color=True, device=dev)
    vol.integrate(v["depth"], v["poses"], v["K"], rgb=v["rgb"])
    return vol


def test_track_with_rgb_holds_on_a_lone_wall(dev, fused):
    """The bound of tests/test_track_color_cpu.py on a volume the device fused itself.  Without rgb the same call does what it did
    before the colour term existed: on this frame depth alone runs off along the wall (93.5 cm in the restatement)."""
    assert tsdf.DEFAULT_COLOR_WEIGHT == DEFAULT_WEIGHT
    c = CC.case("one_wall")
    start = TC.pose_error(c["pose_init"], c["truth"])[1]
    got = fused.track(c["live"], c["K"], c["pose_init"], c["pose_ref"], rgb=c["live_color"])
    want = CC.want("one_wall", color_weight=DEFAULT_WEIGHT)
    end = TC.pose_error(got.transformation.numpy(), c["truth"])[1]
    print(f"one wall: start {100 * start:.2f} cm, with rgb {100 * end:.2f} cm (restatement {100 * TC.pose_error(want['transformation'], c['truth'])[1]:.2f} cm), "
          f"{got.n_color} rows of {got.n_correspondences} pairs, colour rmse {got.color_rmse:.5f}, {got.iterations} iterations")
    assert isinstance(got, tsdf.ColorTrackResult) and got.pose.dtype == torch.float32 and got.transformation.dtype == torch.float64
    assert end < QUARTER * start and got.n_color > 0.9 * got.n_correspondences and 0 < got.color_rmse < 0.02
    assert (got.n_correspondences, got.n_color, got.iterations) == (want["n"], want["n_color"], want["iterations"])
    assert np.abs(got.transformation.numpy() - want["transformation"]).max() < 1e-9
    alone = fused.track(c["live"], c["K"], c["pose_init"], c["pose_ref"])
    far = TC.pose_error(alone.transformation.numpy(), c["truth"])[1]
    print(f"one wall: without rgb {100 * far:.2f} cm, {alone.n_correspondences} pairs, {alone.iterations} iterations")
    assert isinstance(alone, tsdf.TrackResult) and not isinstance(alone, tsdf.ColorTrackResult) and far >= 0.9 * start


def test_track_without_rgb_returns_what_it_did(dev, fused):
    """a colour volume's tsdf and weight words are those of the volume without colour: TSDFVolume.track without rgb on it gives the
    words track_cpu.reg_want holds for the depth-only tracker"""
    r = TC.reg_case("1.9deg_5.8cm")
    got = fused.track(r["live"], r["K"], r["pose_init"], max_iteration=15)
    want = TC.reg_want("1.9deg_5.8cm", max_iteration=15)
    assert type(got) is tsdf.TrackResult and len(got) == 6
    assert got.n_correspondences == want["n"] and got.iterations == want["iterations"] and got.fitness == want["fitness"]
    assert np.abs(got.transformation.numpy() - want["transformation"]).max() < 1e-9 and abs(got.inlier_rmse - want["rmse"]) < 1e-12
    with_rgb = fused.track(r["live"], r["K"], r["pose_init"], max_iteration=15, rgb=CC.reg_colors("1.9deg_5.8cm")[1])
    m0, m1 = TC.pose_error(got.transformation.numpy(), r["truth"])[1], TC.pose_error(with_rgb.transformation.numpy(), r["truth"])[1]
    print(f"corner: depth alone {100 * m0:.2f} cm, with rgb {100 * m1:.2f} cm")
    assert m1 <= m0 + CORNER_MARGIN


# ------------------------------------------------------------------------------------------------------------- 9. odometry
def test_colour_odometry_along_a_wall(dev):
    from mipsfusion_amd.trajectory import trajectory_metrics
    o = CC.odo_case()
    K, H, W = o["K"], o["H"], o["W"]
    poses, records, vol = tsdf.tsdf_odometry(torch.from_numpy(o["depth"]).to(dev), K, o["truth"][0], o["voxel"], o["bounds"], o["trunc"],
                                             rgb=torch.from_numpy(o["rgb"]).to(dev), color_weight=DEFAULT_WEIGHT)
    assert vol.dims == o["dims"] and vol.color is not None and poses.dtype == torch.float32 and not poses.is_cuda
    poses = poses.numpy()
    assert np.array_equal(poses[0], o["truth"][0]) and not any(r["lost"] for r in records)
    # frame by frame: the restatement's registration from the device's own fp32 inputs of that frame.  Every registration here
    # starts ON the pose its model was cast from, so floor(u) of its first evaluation can sit within rounding of a pixel
    # (`ambiguous`); the device evaluates the same operations and is held to the restatement all the same
    ticks = T.make_ticks(o["origin"], o["voxel"], o["dims"])
    state = T.new_state(o["dims"], True)
    T.integrate(state, ticks, o["depth"][:1], poses[:1], K, o["trunc"], rgb=o["rgb"][:1])
    for k in range(1, CC.ODO_FRAMES):
        m = TC.raycast(state, o["origin"], o["voxel"], poses[k - 1:k], K, H, W, 0.5 * o["trunc"], color=True)
        want = CC.register_color(m["depth"][0], m["normals"][0], m["color"][0], poses[k - 1], o["depth"][k], o["rgb"][k], poses[k - 1], K, max_dist=o["trunc"],
                                 color_weight=DEFAULT_WEIGHT)
        got, amb = records[k], sum(want["ambiguous_per_eval"])
        Tg = got["transformation"].numpy()
        print(f"frame {k}: iterations {got['iterations']} {want['iterations']}, pairs {got['n_correspondences']} {want['n']}, rows {got['n_color']} {want['n_color']}, "
              f"ambiguous {amb}, max |dT| {np.abs(Tg - want['transformation']).max():.3e}")
        assert abs(got["n_correspondences"] - want["n"]) <= amb and abs(got["n_color"] - want["n_color"]) <= amb
        if amb == 0:
            assert got["iterations"] == want["iterations"] and got["fitness"] == want["fitness"] and abs(got["inlier_rmse"] - want["rmse"]) < 1e-12
            assert np.abs(Tg - want["transformation"]).max() < 1e-9
        assert np.abs(Tg - want["transformation"]).max() < 1e-6
        assert np.array_equal(poses[k], Tg.astype(np.float32))
        T.integrate(state, ticks, o["depth"][k:k + 1], poses[k:k + 1], K, o["trunc"], rgb=o["rgb"][k:k + 1])
    assert np.array_equal(_words(vol.tsdf), _words(state["tsdf"])) and np.array_equal(_words(vol.color), _words(state["color"]))
    ate = trajectory_metrics(poses, o["truth"]).rmse
    print(f"aligned ATE {1000 * ate:.3f} mm")
    assert ate <= 2 * 0.0022                                     # the gate of tests/test_track_color_cpu.py


def test_odometry_without_color_weight_tracks_by_depth_alone(dev):
    """rgb is fused, as before, and not registered against: on the arc along the wall the depth-only system is refused and every
    frame keeps the first pose (tests/test_track_color_cpu.py shows the restatement doing so); the records are the old ones"""
    o = CC.odo_case()
    poses, records, vol = tsdf.tsdf_odometry(o["depth"], o["K"], o["truth"][0], o["voxel"], o["bounds"], o["trunc"], rgb=o["rgb"], device=dev)
    plain, plain_records, _ = tsdf.tsdf_odometry(o["depth"], o["K"], o["truth"][0], o["voxel"], o["bounds"], o["trunc"], device=dev)
    assert torch.equal(poses.view(torch.int32), plain.view(torch.int32)) and all(np.array_equal(p, o["truth"][0]) for p in poses.numpy())
    assert vol.color is not None and float(vol.color.abs().sum()) > 0
    for a, b in zip(records, plain_records):
        assert set(a) == set(b) == {"transformation", "n_correspondences", "fitness", "inlier_rmse", "iterations", "lost"}
        assert torch.equal(a["transformation"], b["transformation"]) and a["n_correspondences"] == b["n_correspondences"] and a["iterations"] == b["iterations"]
    with pytest.raises(ValueError, match="needs rgb"):
        tsdf.tsdf_odometry(o["depth"], o["K"], o["truth"][0], o["voxel"], o["bounds"], o["trunc"], color_weight=1.0, device=dev)


# ------------------------------------------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("change,said", REGISTER_COLOR_REFUSALS, ids=_ids(REGISTER_COLOR_REFUSALS))
def test_the_colour_registration_refusals_name_their_argument(dev, change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_register_color(C.byref(_register_color_block(**change)), None) != 0
    assert b"mipsf_track_register_color" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_the_python_layer_refuses_too(dev):
    K, depth, rgb = (10.0, 10.0, 4.0, 4.0), np.ones((8, 9), np.float32), np.full((8, 9, 3), 0.5, np.float32)
    plain = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (4, 4, 4), 0.4, device=dev)
    with pytest.raises(ValueError, match="without colour"):
        plain.track(depth, K, torch.eye(4), rgb=rgb)
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (4, 4, 4), 0.4, color=True, device=dev)
    model = vol.raycast(torch.eye(4), K, 8, 9)
    assert model.color is None
    with pytest.raises(ValueError, match="color=True"):
        vol.track(depth, K, torch.eye(4), model=model, rgb=rgb)
    for bad in (np.ones((8, 9), np.float32), np.ones((8, 8, 3), np.float32), np.ones((2, 8, 9, 3), np.float32), np.ones((8, 9, 4), np.float32)):
        with pytest.raises(ValueError, match="rgb"):
            vol.track(depth, K, torch.eye(4), rgb=bad)
    with pytest.raises(RuntimeError, match="color_weight"):
        vol.track(depth, K, torch.eye(4), rgb=rgb, color_weight=-1.0)
    with pytest.raises(RuntimeError, match="max_color_diff"):
        vol.track(depth, K, torch.eye(4), rgb=rgb, max_color_diff=math.nan)
    got = vol.track(depth, K, torch.eye(4), rgb=rgb)                     # an empty volume: no model, no pair, no row
    assert isinstance(got, tsdf.ColorTrackResult) and got.n_correspondences == 0 and got.n_color == 0 and got.iterations == 1
