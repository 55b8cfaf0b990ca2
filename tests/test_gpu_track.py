"""GPU tests of the TSDF tracker's model side (mipsfusion_amd/tsdf.py: TSDFVolume.raycast, TSDFVolume.track, tsdf_odometry;
csrc/tsdf_track.hip) against the float64 restatement of tests/track_cpu.py.  The device and the restatement get the same fp32 words
and evaluate the same float64 expressions, so the ray cast's depth, normal and colour words and its hit count, and the
registration's pair sets and counts, are compared for EQUALITY; the restatement evaluates every sample of every ray, so equality
also shows that the brick skipping leaves out nothing that matters.  tests/test_track_cpu.py asserts, on the same cases, that no
pixel of a registration lies within rounding of a decision."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, tsdf

from . import raster_cpu as R
from . import track_cpu as TC
from . import tsdf_cpu as T
from .test_track_cpu import RAYCAST_REFUSALS, REGISTER_REFUSALS, _ids, _raycast_block, _register_block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _volume(dev, state, origin, voxel, trunc):
    vol = tsdf.TSDFVolume(origin, voxel, state["tsdf"].shape, trunc, color=state["color"] is not None, device=dev)
    vol.tsdf.copy_(torch.from_numpy(state["tsdf"]))
    vol.weight.copy_(torch.from_numpy(state["weight"]))
    if state["color"] is not None:
        vol.color.copy_(torch.from_numpy(state["color"]))
    return vol


def _cast(dev, c, flags=0):
    vol = _volume(dev, c["state"], c["origin"], c["voxel"], c["trunc"])
    poses = c["poses"].to(dev).to(torch.float32).contiguous()
    return vol.raycast_enqueue(poses, c["K"], c["H"], c["W"], c["near"], c["far"], c["step"], c["min_weight"], True, c["color"], flags)


def _differing(got, want):
    out = {"depth": int((_words(got.depth) != _words(want["depth"])).sum()), "normals": int((_words(got.normals) != _words(want["normals"])).sum())}
    if want["color"] is not None:
        out["color"] = int((_words(got.color) != _words(want["color"])).sum())
    return out


# ------------------------------------------------------------------------------------------------------------- 1, 2. ray cast
@pytest.mark.parametrize("name", TC.RAYCAST_CASES)
def test_the_ray_cast_words_equal_the_restatement(dev, name):
    c = TC.case(name)
    got = _cast(dev, c)
    diff = _differing(got, c["want"])
    hits, marked = (int(x) for x in got.hits.cpu())
    print(f"{name}: dims {c['dims']}, {len(c['poses'])} views of {c['H']} x {c['W']}, differing words {diff}, hits {hits} (restatement {c['want']['hits']}), "
          f"bricks marked {marked}")
    assert got.depth.shape == (len(c["poses"]), c["H"], c["W"]) and got.normals.shape == got.depth.shape + (3,)
    assert not any(diff.values()), name
    assert hits == c["want"]["hits"] and marked == (int(TC.brick_marks(c["state"], c["min_weight"]).sum()) if len(c["poses"]) else 0)


@pytest.mark.parametrize("name", TC.RAYCAST_CASES)
def test_without_the_skipping_the_bytes_are_the_same(dev, name):
    c = TC.case(name)
    skipped, plain = _cast(dev, c), _cast(dev, c, _lib.TRACK_NO_SKIP)
    assert not any(_differing(plain, c["want"]).values()), name
    assert torch.equal(skipped.depth.view(torch.int32), plain.depth.view(torch.int32)) and torch.equal(skipped.normals.view(torch.int32), plain.normals.view(torch.int32))
    if c["color"]:
        assert torch.equal(skipped.color.view(torch.int32), plain.color.view(torch.int32))
    assert plain.hits.tolist() == [c["want"]["hits"], 0]
    if name in ("plane", "unobserved"):                          # most bricks are free space here: the skipping is at work
        marks = TC.brick_marks(c["state"], c["min_weight"])
        assert marks.mean() <= 0.2 and c["want"]["samples"] > 1000, (name, marks.mean())


def test_the_ray_cast_of_the_fused_room_lies_on_the_closed_form(dev):
    """the gates of tests/test_track_cpu.py, on a volume the device fused itself"""
    c = T.case("box/40x56/v0.15/t4")
    vol = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], device=dev)
    vol.integrate(c["depth"], c["poses"], c["K"])
    poses = c["poses"][list(TC.BOX_VIEWS)]
    got = vol.raycast(poses, c["K"], c["H"], c["W"])
    assert isinstance(got, tsdf.Raycast) and got.depth.is_cuda and got.normals.is_cuda and got.color is None and got.hits.is_cuda
    _, _, lo, hi = R.box_room()
    for k, view in enumerate(TC.BOX_VIEWS):
        exact = R.box_exit_depth(lo, hi, poses[k].numpy(), c["K"], c["H"], c["W"])
        d = got.depth[k].cpu().numpy()
        err = np.abs(d[d != 0] - exact[d != 0]) / c["voxel"]
        print(f"view {view}: hit rate {(d != 0).mean():.3f}, mean {err.mean():.4f}, max {err.max():.4f} voxels")
        assert (d != 0).mean() >= 0.9 and err.mean() <= TC.DEPTH_MEAN_GATE and err.max() <= TC.DEPTH_MAX_GATE


# ------------------------------------------------------------------------------------------------------------- 4. registration
def _register(dev, c, partner=True, **kw):
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (2, 2, 2), 0.4, device=dev)              # only its device is used: the model is given
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)          # noqa: E731
    model = tsdf.Raycast(t(c["model_depth"])[None], t(c["model_normals"])[None], None, None)
    return vol.track_enqueue(t(c["live"]), c["K"], t(c["pose_init"]), t(c["pose_ref"]), model, c["max_dist"], depth_max=c["depth_max"], partner=partner, **kw)


def _read(result):
    r = result.cpu().numpy()
    return {"transformation": r[:16].reshape(4, 4), "n": int(r[16]), "fitness": float(r[17]), "rmse": float(r[18]), "iterations": int(r[19])}


@pytest.mark.parametrize("name", TC.REG_CASES)
def test_registration_equals_the_restatement(dev, name):
    c, want = TC.reg_case(name), TC.reg_want(name)
    H, W = c["H"], c["W"]
    result, pose, partner = _register(dev, c, max_iteration=0)
    first, w0 = _read(result), TC.reg_want(name, max_iteration=0)
    assert first["iterations"] == 0 and first["n"] == w0["n"] == want["pairs_per_eval"][0]
    assert np.array_equal(partner.cpu().numpy().reshape(-1), w0["partner"])
    assert np.array_equal(first["transformation"], np.asarray(c["pose_init"], np.float32).astype(np.float64)) and np.array_equal(pose.cpu().numpy(), c["pose_init"])
    result, pose, partner = _register(dev, c)
    got = _read(result)
    amb = sum(want["ambiguous_per_eval"])
    print(name, "iterations", got["iterations"], want["iterations"], "pairs", got["n"], want["n"], "ambiguous", amb,
          "max |dT| %.3e" % np.abs(got["transformation"] - want["transformation"]).max(), "rmse difference %.3e" % abs(got["rmse"] - want["rmse"]))
    assert amb == 0 and np.isfinite(got["transformation"]).all()
    # the pair count of every evaluation: a loop cut off after k updates ends on evaluation k
    for k, pairs in enumerate(want["pairs_per_eval"]):
        cut = _read(_register(dev, c, partner=False, max_iteration=k)[0])
        assert cut["iterations"] == k and cut["n"] == pairs, (k, cut["n"], pairs)
    assert got["n"] == want["n"] and got["iterations"] == want["iterations"] and got["fitness"] == want["fitness"]
    assert abs(got["rmse"] - want["rmse"]) < 1e-12
    assert np.abs(got["transformation"] - want["transformation"]).max() < 1e-9
    assert np.array_equal(partner.cpu().numpy().reshape(-1), want["partner"])
    assert np.array_equal(pose.cpu().numpy(), got["transformation"].astype(np.float32))
    if name == "no_model":
        assert got["n"] == 0 and got["fitness"] == 0.0 and got["iterations"] == 1 and np.array_equal(pose.cpu().numpy(), c["pose_init"])


def test_track_casts_its_own_model(dev):
    """TSDFVolume.track without a model: the ray cast from pose_ref and the registration, one read-back; the same as the two steps"""
    c = T.case(TC.REG_VOLUME)
    r = TC.reg_case("1.9deg_5.8cm")
    vol = _volume(dev, c["state"], c["origin"], c["voxel"], c["trunc"])
    got = vol.track(r["live"], r["K"], r["pose_init"], max_iteration=15)
    want = TC.reg_want("1.9deg_5.8cm", max_iteration=15)
    assert isinstance(got, tsdf.TrackResult) and got.pose.dtype == torch.float32 and got.transformation.dtype == torch.float64
    assert got.n_correspondences == want["n"] and got.iterations == want["iterations"] and got.fitness == want["fitness"]
    assert np.abs(got.transformation.numpy() - want["transformation"]).max() < 1e-9 and abs(got.inlier_rmse - want["rmse"]) < 1e-12
    deg, m = TC.pose_error(got.transformation.numpy(), r["truth"])
    assert m <= 2 * 0.0066 and deg <= 2 * 0.204


# ------------------------------------------------------------------------------------------------------------- 5. reproducibility
def test_every_output_repeats_bit_for_bit(dev):
    c = TC.case("colour")
    a, b = _cast(dev, c), _cast(dev, c)
    for x, y in ((a.depth, b.depth), (a.normals, b.normals), (a.color, b.color)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(a.hits, b.hits)
    r = TC.reg_case("3.8deg_11.7cm")
    (r1, p1, m1), (r2, p2, m2) = _register(dev, r), _register(dev, r)
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64)) and torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(m1, m2)
    assert float(r1[19]) >= 2 and float(r1[16]) > 0


def test_registration_replays_from_a_graph_on_a_new_live_frame(dev):
    c, other = TC.reg_case("0.64deg_2.3cm"), TC.reg_case("1.9deg_5.8cm")
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (2, 2, 2), 0.4, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)          # noqa: E731
    model = tsdf.Raycast(t(c["model_depth"])[None], t(c["model_normals"])[None], None, None)
    live, init, ref = t(c["live"]), t(c["pose_init"]), t(c["pose_ref"])
    run = lambda: vol.track_enqueue(live, c["K"], init, ref, model, c["max_dist"], partner=True)      # noqa: E731
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()                                                    # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        res, pose, partner = run()
    for frame in (other["live"], c["live"]):
        live.copy_(t(frame))
        g.replay()
        torch.cuda.synchronize()
        eager_res, eager_pose, eager_partner = run()
        assert torch.equal(res.view(torch.int64), eager_res.view(torch.int64)) and torch.equal(partner, eager_partner)
        assert torch.equal(pose.view(torch.int32), eager_pose.view(torch.int32))
        assert float(res[19]) >= 2 and float(res[16]) > 0


# ------------------------------------------------------------------------------------------------------------- 6. odometry
def test_odometry_over_an_arc(dev):
    from mipsfusion_amd.trajectory import trajectory_metrics
    o = TC.odo_case()
    K, H, W = o["K"], o["H"], o["W"]
    poses, records, vol = tsdf.tsdf_odometry(torch.from_numpy(o["depth"]).to(dev), K, o["truth"][0], o["voxel"], o["bounds"], o["trunc"])
    assert vol.dims == o["dims"] and np.array_equal(vol.origin, o["origin"]) and poses.dtype == torch.float32 and not poses.is_cuda
    poses = poses.numpy()
    assert np.array_equal(poses[0], o["truth"][0]) and not any(r["lost"] for r in records)
    # frame by frame: the restatement's registration from the device's own fp32 inputs of that frame
    ticks = T.make_ticks(o["origin"], o["voxel"], o["dims"])
    state = T.new_state(o["dims"])
    T.integrate(state, ticks, o["depth"][:1], poses[:1], K, o["trunc"])
    for k in range(1, TC.ODO_FRAMES):
        m = TC.raycast(state, o["origin"], o["voxel"], poses[k - 1:k], K, H, W, 0.5 * o["trunc"])
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
        T.integrate(state, ticks, o["depth"][k:k + 1], poses[k:k + 1], K, o["trunc"])
    assert np.array_equal(_words(vol.tsdf), _words(state["tsdf"])) and np.array_equal(_words(vol.weight), _words(state["weight"]))
    cpu_poses, _, _ = TC.odometry(o["depth"], K, o["truth"][0], o["origin"], o["voxel"], o["dims"], o["trunc"])
    ate, cpu_ate = trajectory_metrics(poses, o["truth"]).rmse, trajectory_metrics(cpu_poses, o["truth"]).rmse
    print(f"aligned ATE {1000 * ate:.3f} mm, the restatement's walk {1000 * cpu_ate:.3f} mm")
    assert ate <= 2 * cpu_ate


def test_odometry_flags_a_lost_frame_and_does_not_fuse_it(dev):
    o = TC.odo_case()
    K = o["K"]
    depth = o["depth"][:5].copy()
    depth[3] = 0
    poses, records, vol = tsdf.tsdf_odometry(depth, K, o["truth"][0], o["voxel"], o["bounds"], o["trunc"], min_correspondences=100, device=dev)
    poses = poses.numpy()
    assert [r["lost"] for r in records] == [False, False, False, True, False] and records[3]["n_correspondences"] == 0
    assert np.array_equal(poses[3], poses[2])
    ticks, state = T.make_ticks(o["origin"], o["voxel"], o["dims"]), T.new_state(o["dims"])
    keep = [0, 1, 2, 4]
    T.integrate(state, ticks, depth[keep], poses[keep], K, o["trunc"])
    assert np.array_equal(_words(vol.tsdf), _words(state["tsdf"])) and np.array_equal(_words(vol.weight), _words(state["weight"]))
    # every frame lost, with depth that would update the volume at the pose kept: the NaN pose keeps it out
    poses, records, vol = tsdf.tsdf_odometry(o["depth"][:3], K, o["truth"][0], o["voxel"], o["bounds"], o["trunc"], min_correspondences=10 ** 6, device=dev)
    assert [r["lost"] for r in records] == [False, True, True] and all(np.array_equal(p, o["truth"][0]) for p in poses.numpy())
    state = T.new_state(o["dims"])
    T.integrate(state, ticks, o["depth"][:1], o["truth"][:1], K, o["trunc"])
    assert np.array_equal(_words(vol.tsdf), _words(state["tsdf"])) and np.array_equal(_words(vol.weight), _words(state["weight"]))


def test_the_enqueue_forms_return_device_tensors(dev):
    """the walk of tsdf_odometry is made of these and reads back once, at its end"""
    c = T.case(TC.REG_VOLUME)
    r = TC.reg_case("0.64deg_2.3cm")
    vol = _volume(dev, c["state"], c["origin"], c["voxel"], c["trunc"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)          # noqa: E731
    cast = vol.raycast_enqueue(t(r["pose_ref"])[None], r["K"], r["H"], r["W"])
    assert all(x.is_cuda for x in (cast.depth, cast.normals, cast.hits))
    result, pose = vol.track_enqueue(t(r["live"]), r["K"], t(r["pose_init"]))
    assert result.is_cuda and result.dtype == torch.float64 and result.shape == (20,) and pose.is_cuda and pose.dtype == torch.float32
    assert vol.integrate_enqueue(t(r["live"])[None], pose[None], r["K"]).is_cuda
    assert torch.equal(cast.depth.view(torch.int32).cpu(), torch.from_numpy(TC.reg_model()[0])[None].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("change,said", RAYCAST_REFUSALS, ids=_ids(RAYCAST_REFUSALS))
def test_the_ray_cast_refusals_name_their_argument(dev, change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_raycast(C.byref(_raycast_block(**change)), None) != 0
    assert b"mipsf_track_raycast" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


@pytest.mark.parametrize("change,said", REGISTER_REFUSALS, ids=_ids(REGISTER_REFUSALS))
def test_the_registration_refusals_name_their_argument(dev, change, said):
    lib = _lib.lib()
    assert lib.mipsf_track_register(C.byref(_register_block(**change)), None) != 0
    assert b"mipsf_track_register" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_the_python_layer_refuses_too(dev):
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), 0.1, (4, 4, 4), 0.4, device=dev)
    with pytest.raises(ValueError, match="without colour"):
        vol.raycast(torch.eye(4), (10.0, 10.0, 4.0, 4.0), 8, 9, color=True)
    with pytest.raises(ValueError, match=r"\[n,4,4\]"):
        vol.raycast_enqueue(torch.eye(4, device=dev), (10.0, 10.0, 4.0, 4.0), 8, 9)
    with pytest.raises(RuntimeError, match="step"):
        vol.raycast(torch.eye(4), (10.0, 10.0, 4.0, 4.0), 8, 9, step=-1.0)
    with pytest.raises(RuntimeError, match="max_dist"):
        vol.track(np.ones((8, 9), np.float32), (10.0, 10.0, 4.0, 4.0), torch.eye(4), max_dist=math.inf)
    none = vol.raycast_enqueue(torch.zeros(0, 4, 4, device=dev), (10.0, 10.0, 4.0, 4.0), 8, 9)
    assert none.depth.shape == (0, 8, 9) and none.hits.tolist() == [0, 0]
