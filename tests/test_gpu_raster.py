"""GPU tests of the mesh renderer (mipsfusion_amd/mesh_render.py, csrc/raster.hip) against the float64 restatement of
tests/raster_cpu.py.  Both sides get the same fp32 words and evaluate the same float64 expressions, and a pixel's winner is an
integer minimum, so depth words, face indices and `seen` flags are compared for EQUALITY; only the L1 sums carry a tolerance, the
bound H*W * 2^-53 (relative) that holds for any order of adding H*W non-negative terms.  The restatement tests every pixel against
every face, so equality also shows that the device's screen boxes leave out no pixel.  tests/test_raster_cpu.py holds the
restatement to the closed-form depth of the synthetic rooms."""
import ctypes as C

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, evaluate as ev, mesh as mesh_mod, mesh_render as mr

from . import eval_cpu as E
from . import raster_cpu as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _render(c, **kw):
    return mr.render_mesh_depth((c["vertices"], c["faces"]), c["poses"], c["K"], c["H"], c["W"], c["near"], c["far"], **kw)


# ------------------------------------------------------------------------------------------------------------- 1. depth
@pytest.mark.parametrize("name", R.DEPTH_CASES)
def test_depth_and_faces_equal_the_restatement(dev, name):
    c = R.depth_case(name)
    depth, face = _render(c)
    n = len(c["poses"])
    assert depth.dtype == torch.float32 and face.dtype == torch.int32 and depth.device.type == "cuda"
    assert tuple(depth.shape) == (n, c["H"], c["W"]) == tuple(face.shape)
    got_d, got_f = depth.cpu().numpy(), face.cpu().numpy()
    print(f"{name}: pixels hit per view {[int((x >= 0).sum()) for x in got_f]}, differing depth words "
          f"{int((_words(got_d) != _words(c['depth'])).sum())}, differing faces {int((got_f != c['face']).sum())}")
    assert np.array_equal(got_f, c["face"]), name
    assert np.array_equal(_words(got_d), _words(c["depth"])), name
    if name.startswith("outside"):
        assert not got_d.any() and np.all(got_f == -1)


@pytest.mark.parametrize("name", ["two_rooms/33x47", "marched_24/33x47", "random_5000/33x47"])
def test_the_cut_into_launches_does_not_reach_the_bytes(dev, name):
    c = R.depth_case(name)
    one = _render(c)
    for other in (_render(c, views_per_launch=1), _render(c, views_per_launch=2), _render(c)):
        assert one[0].cpu().numpy().tobytes() == other[0].cpu().numpy().tobytes()
        assert one[1].cpu().numpy().tobytes() == other[1].cpu().numpy().tobytes()
    assert mr.views_per_launch_for(64, 12, 460, 620, cap=8 * (460 * 620 + 12) * 5 + 100) == 5


def test_renderer_accepts_a_mesh_tensors_and_a_matrix(dev):
    c = R.depth_case("box_room/33x47")
    v, f, _, _ = R.box_room()
    fx, fy, cx, cy = c["K"]
    Kmat = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    for mesh, poses in ((mesh_mod.Mesh(v, f, None), c["poses"]), ((torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)), c["poses"].to(dev)),
                        ((v, f), [p for p in c["poses"]])):
        depth, face = mr.render_mesh_depth(mesh, poses, Kmat, c["H"], c["W"])
        assert np.array_equal(_words(depth.cpu().numpy()), _words(c["depth"])) and np.array_equal(face.cpu().numpy(), c["face"])
    single = mr.render_mesh_depth((v, f), c["poses"][4], c["K"], c["H"], c["W"])[0]
    assert tuple(single.shape) == (1, c["H"], c["W"]) and np.array_equal(_words(single.cpu().numpy()[0]), _words(c["depth"][4]))


@pytest.mark.parametrize("size", sorted(R.SIZES))
def test_box_room_on_the_device_equals_the_analytic_depth(dev, size):
    """one fp32 rounding (2^-24) of a value both sides have to 1e-15: within 2^-23 relative, no pixel missed"""
    c = R.depth_case(f"box_room/{size}")
    _, _, lo, hi = R.box_room()
    depth = _render(c)[0].cpu().numpy().astype(np.float64)
    want = np.stack([R.box_exit_depth(lo, hi, p.numpy(), c["K"], c["H"], c["W"]) for p in c["poses"]])
    rel = np.abs(depth - want) / want
    print(f"box room {size}: largest relative difference to the analytic depth {rel.max():.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert np.all(depth > 0) and rel.max() <= 2.0 ** -23


def test_vertices_that_are_not_finite_and_bad_indices_are_inputs(dev):
    """NaN and infinite vertices: their faces hit nothing, every other pixel is as before (the three bad indices of mesh_random are
    in every random_5000 case already)"""
    c = dict(R.depth_case("random_5000/48x64"))
    hit_faces, pixels = np.unique(c["face"][c["face"] >= 0], return_counts=True)
    hit_faces = hit_faces[np.argsort(pixels, kind="stable")]                            # the smallest first: the giant face stays
    v = c["vertices"].copy()
    v[c["faces"][hit_faces[0]][1]] = np.nan
    v[c["faces"][hit_faces[1]][0], 2] = np.inf
    v[c["faces"][hit_faces[2]][2], 0] = -np.inf
    want_d, want_f = R.render_depth(v, c["faces"], c["poses"], c["K"], c["H"], c["W"])
    assert not np.isin(hit_faces[:3], want_f).any() and (want_f >= 0).sum() > 200
    depth, face = mr.render_mesh_depth((v, c["faces"]), c["poses"], c["K"], c["H"], c["W"])
    assert np.array_equal(face.cpu().numpy(), want_f) and np.array_equal(_words(depth.cpu().numpy()), _words(want_d))


# ------------------------------------------------------------------------------------------------------------- 2. depth L1
def _sums_close(got, want, n):
    return abs(got - want) <= n * 2.0 ** -53 * abs(want)


def _check_records(got, want, hw):
    for g, w in zip(got, want):
        assert (g.both, g.rec_only, g.gt_only, g.neither) == (w["both"], w["rec_only"], w["gt_only"], w["neither"])
        assert g.both + g.rec_only + g.gt_only + g.neither == hw
        print(f"l1 record: sum_all {g.sum_all!r} (fsum {w['sum_all']!r}), sum_both {g.sum_both!r} (fsum {w['sum_both']!r})")
        assert _sums_close(g.sum_all, w["sum_all"], hw) and _sums_close(g.sum_both, w["sum_both"], hw)


def test_l1_records_equal_the_restatement(dev):
    """the marched room against the 12 triangles, with holes punched into both stacks so that all four counts are exercised; a
    second pair of one pixel by one; a stack against itself"""
    a, b = R.depth_case("marched_24/33x47")["depth"].copy(), R.depth_case("box_room/33x47")["depth"][:3].copy()
    a[:, :4], b[:, 2:9, 5:20], b[1] = 0, 0, 0
    got = mr.read_l1_records(mr.l1_enqueue(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    want = R.l1_records(a, b)
    assert all(w["rec_only"] and w["gt_only"] or not w["both"] for w in want) and want[0]["neither"] and want[0]["both"]
    _check_records(got, want, a.shape[1] * a.shape[2])
    x, y = np.array([[[1.5]], [[0.0]]], np.float32), np.array([[[1.25]], [[2.0]]], np.float32)
    tiny = mr.read_l1_records(mr.l1_enqueue(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)))
    assert (tiny[0].sum_all, tiny[0].sum_both, tiny[0].both) == (0.25, 0.25, 1) and (tiny[1].sum_all, tiny[1].sum_both, tiny[1].gt_only) == (2.0, 0.0, 1)
    big = R.depth_case("box_room/40x56")["depth"]
    same = mr.read_l1_records(mr.l1_enqueue(torch.from_numpy(big).to(dev), torch.from_numpy(big).to(dev)))
    assert all(r.sum_all == 0.0 and r.sum_both == 0.0 and r.both == big.shape[1] * big.shape[2] for r in same)


def test_depth_l1_of_the_marched_room(dev):
    c = R.depth_case("marched_24/33x47")
    v, f, _, _ = R.box_room()
    want = R.depth_metrics(R.l1_records(c["depth"], R.depth_case("box_room/33x47")["depth"][:3]), c["H"], c["W"])
    got = mr.depth_l1(mesh_mod.Mesh(c["vertices"].astype(np.float64), c["faces"], None), (v, f), c["poses"], c["K"], c["H"], c["W"])
    print("device %s\nrestatement %s" % (got, want))
    hw = c["H"] * c["W"]
    for k in ("both", "rec_only", "gt_only", "neither", "n_views", "pixels"):
        assert getattr(got, k) == want[k], k
    assert _sums_close(got.l1, want["l1"], hw) and _sums_close(got.l1_both, want["l1_both"], hw)
    assert all(_sums_close(g, w, hw) for g, w in zip(got.l1_per_view, want["l1_per_view"]))
    assert all(_sums_close(g, w, hw) for g, w in zip(got.l1_both_per_view, want["l1_both_per_view"]))
    assert got.both == 1.0 and 0.001 < got.l1 < 0.02                      # the bevel of the marched corners, millimetres
    zero = mr.depth_l1((v, f), (v, f), c["poses"], c["K"], c["H"], c["W"])
    assert zero.l1 == 0.0 and zero.l1_both == 0.0 and zero.both == 1.0


# ------------------------------------------------------------------------------------------------------------- 3. occlusion
_ROOM_A = None


def _room_a_case():
    """the two-room mesh seen from one pose in room A through the door: (vertices fp32, faces, pose [1,4,4], depth, max_depth)"""
    global _ROOM_A
    if _ROOM_A is None:
        c = R.depth_case("two_rooms/40x56")
        _ROOM_A = (c["vertices"], c["faces"], c["poses"][:1], c["depth"][:1], np.array([20.0], np.float32), c["K"], c["H"], c["W"])
    return _ROOM_A


def test_seen_equals_the_restatement(dev):
    v, f, pose, depth, md, K, H, W = _room_a_case()
    g = np.random.default_rng(4)
    lo, hi = v.min(0), v.max(0)
    cloud = (lo - 0.3 + g.random((2000, 3)) * (hi - lo + 0.6)).astype(np.float32)
    all_poses, all_depth = R.depth_case("two_rooms/40x56")["poses"], R.depth_case("two_rooms/40x56")["depth"]
    all_md = np.array([20.0, 20.0, 3.0, 2.5, 20.0, 1.0], np.float32)
    for points, P, D, M, edge, eps in ((v, pose, depth, md, 0, 0.02), (cloud, pose, depth, md, 2, 0.02), (cloud, all_poses, all_depth, all_md, 1.5, 0.05),
                                      (cloud, all_poses, np.zeros_like(all_depth), all_md, 0.25, 0.0), (cloud, pose, depth, md, -3.0, 0.02)):
        want = R.visible(points, D, P, M, K, edge, eps)
        got = mr.visible_points(points, torch.from_numpy(np.ascontiguousarray(D)).to(dev), P, M, K, edge, eps)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
        assert points is v or 0 < want.sum() < len(want)
    # the far walls of room B are occluded except through the door: without the depth image every vertex in the frustum is seen
    in_b = cloud[:, 2] > 2.76
    with_depth, without = R.visible(cloud, depth, pose, md, K, 0, 0.02), R.visible(cloud, np.zeros_like(depth), pose, md, K, 0, 0.02)
    assert (without & in_b).sum() > (with_depth & in_b).sum()
    assert mr.visible_points(v[:0], torch.from_numpy(depth).to(dev), pose, md, K, 0, 0.02).shape == (0,)


def test_cull_with_occlusion_equals_the_restatement(dev):
    """a box of 432 faces that spans both rooms, seen from the two door views: culled against its own depth (occluder=None), and
    against the two-room mesh, whose shared wall hides the other room's part of the box except through the door"""
    c = R.depth_case("two_rooms/40x56")
    v, f = E.tessellated_box(c["vertices"].min(0).astype(np.float64) + 0.05, c["vertices"].max(0).astype(np.float64) - 0.05, m=6)
    occluder = (c["vertices"].astype(np.float64), c["faces"])
    poses, md = c["poses"][:2], torch.tensor([20.0, 20.0])
    want_self = R.cull_faces((v, f), None, poses, md.numpy(), c["K"], c["W"], c["H"], 2, 0.02)
    got_self = ev.cull_to_views(mesh_mod.Mesh(v, f, None), poses, md, c["K"], c["W"], c["H"], edge=2, occlusion=True, eps=0.02)
    assert isinstance(got_self, mesh_mod.Mesh) and np.array_equal(got_self.faces, want_self) and 0 < len(want_self) < len(f)
    want = R.cull_faces((v, f), occluder, poses, md.numpy(), c["K"], c["W"], c["H"], 2, 0.02)
    got = ev.cull_to_views((v, f), poses, md, c["K"], c["W"], c["H"], edge=2, occlusion=True, occluder=occluder, eps=0.02)
    assert np.array_equal(got.faces, want) and np.array_equal(got.vertices, v) and 0 < len(want) < len(f)
    assert not np.array_equal(want, want_self)
    with pytest.raises(ValueError, match="eps"):
        ev.cull_to_views((v, f), poses, md, c["K"], c["W"], c["H"], occlusion=True)


def test_cull_without_occlusion_is_what_it_was(dev):
    from . import scene_mesh_cpu as S
    c = E.cull_case()
    views = (c["kf_c2w"], c["kf_max_depth"], c["K"], c["W"], c["H"])
    keep = S.point_mask(c["vertices"].astype(np.float32), *views)[c["faces"]].all(1)
    mesh = mesh_mod.Mesh(c["vertices"], c["faces"], None)
    for got in (ev.cull_to_views(mesh, *views), ev.cull_to_views(mesh, *views, occlusion=False), ev.cull_to_views(mesh, *views, 20, False)):
        assert np.array_equal(got.faces, c["faces"][keep]) and np.array_equal(got.vertices, c["vertices"])


# ------------------------------------------------------------------------------------------------------------- 4. refusals
def test_what_is_out_of_range_is_refused_on_the_host(dev):
    """refused with a message before anything is launched: the outputs keep the value they were filled with"""
    c = R.depth_case("box_room/33x47")
    v = torch.from_numpy(c["vertices"]).to(dev)
    f = torch.from_numpy(c["faces"]).to(torch.int32).to(dev)
    poses = c["poses"][:2].to(dev).contiguous()
    K, H, W = c["K"], c["H"], c["W"]
    depth = torch.full((2, H, W), -7.0, device=dev)
    face = torch.full((2, H, W), -7, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="without faces"):
        mr.render_enqueue(v, f[:0], poses, K, H, W, depth=depth, face=face)
    with pytest.raises(RuntimeError, match="no views"):
        mr.render_enqueue(v, f, poses[:0], K, H, W)
    with pytest.raises(RuntimeError, match="no pixels"):
        mr.render_enqueue(v, f, poses, K, 0, W)
    with pytest.raises(RuntimeError, match="no pixels"):
        mr.render_enqueue(v, f, poses, K, H, 0)
    with pytest.raises(RuntimeError, match="at most 8192 a side"):
        mr.render_enqueue(v, f, poses[:1], K, _lib.RASTER_MAX_SIDE + 1, 1)
    big = _lib.RasterDepthArgs.new(V=8, F=12, n=17, H=8192, W=8192, fx=1.0, fy=1.0, vertices=v.data_ptr(), faces=f.data_ptr(),
                                   poses=poses.data_ptr(), depth=depth.data_ptr(), face=face.data_ptr(), workspace=depth.data_ptr())
    assert _lib.lib().mipsf_raster_depth(C.byref(big), _lib.stream_ptr()) != 0            # 17 * 2^26 pixels: refused before a pointer is used
    assert b"pixels a call" in _lib.lib().mipsf_last_error()
    with pytest.raises(RuntimeError, match="intrinsics"):
        mr.render_enqueue(v, f, poses, (0.0, 35.0, 1.0, 1.0), H, W, depth=depth, face=face)
    ws = torch.empty(int(_lib.lib().mipsf_raster_workspace_bytes(_lib.RASTER_WS_DEPTH, 2, 12, H, W)) + 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        mr.render_enqueue(v, f, poses, K, H, W, depth=depth, face=face, workspace=ws[8:])
    with pytest.raises(ValueError, match="at least one"):
        mr.render_mesh_depth((c["vertices"], c["faces"][:0]), c["poses"], K, H, W)
    with pytest.raises(RuntimeError, match="out of range"):
        mr.render_mesh_depth((c["vertices"], c["faces"]), c["poses"], K, _lib.RASTER_MAX_SIDE + 8, 8)
    with pytest.raises(RuntimeError, match="no views"):
        mr.l1_enqueue(depth[:0], depth[:0])
    torch.cuda.synchronize()
    assert bool((depth == -7.0).all()) and bool((face == -7).all())
    got = mr.render_enqueue(v, f, poses, K, H, W, depth=depth, face=face, workspace=ws[16:])      # and the same blocks then serve a good call
    assert np.array_equal(_words(got[0].cpu().numpy()), _words(c["depth"][:2]))
