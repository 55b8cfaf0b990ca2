"""GPU tests of the TSDF fusion (mipsfusion_amd/tsdf.py, csrc/tsdf.hip) against the float64 restatement of tests/tsdf_cpu.py.  Both
sides get the same fp32 words and evaluate the same float64 expressions in the same view order, so tsdf, weight and colour words
and the two counts are compared for EQUALITY.  The restatement tests every voxel against every view, so equality also shows that
the device's brick culling leaves out no pair.  tests/test_tsdf_cpu.py holds the restatement to the walls of the synthetic rooms."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, evaluate as ev, mesh as mesh_mod, mesh_render as mr, synth, tsdf

from . import raster_cpu as R
from . import tsdf_cpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _words(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def _fuse(c, dev, **kw):
    vol = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], color=c["rgb"] is not None, max_weight=c["max_weight"], device=dev)
    counts = vol.integrate(c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], **kw)
    return vol, counts


def _differing(vol, c):
    d = {"tsdf": int((_words(vol.tsdf) != _words(c["state"]["tsdf"])).sum()), "weight": int((_words(vol.weight) != _words(c["state"]["weight"])).sum())}
    if c["rgb"] is not None:
        d["color"] = int((_words(vol.color) != _words(c["state"]["color"])).sum())
    return d


# ------------------------------------------------------------------------------------------------------------- 1. the words
@pytest.mark.parametrize("name", T.EQUALITY_CASES)
def test_the_volume_and_the_counts_equal_the_restatement(dev, name):
    c = T.case(name)
    vol, counts = _fuse(c, dev)
    assert vol.tsdf.dtype == torch.float32 and vol.tsdf.device.type == "cuda" and tuple(vol.tsdf.shape) == c["dims"]
    diff = _differing(vol, c)
    print(f"{name}: dims {c['dims']}, {len(c['poses'])} views, differing words {diff}, counts {tuple(counts)} (restatement {(c['updates'], c['observed'])})")
    assert not any(diff.values()), name
    assert tuple(counts) == (c["updates"], c["observed"]), name
    if name == "outside":
        assert counts == (0, 0) and not vol.tsdf.any() and not vol.weight.any()
    if name == "many_views":
        assert len(c["poses"]) == _lib.TSDF_VIEW_CHUNK + 1


@pytest.mark.parametrize("name", ["box/33x47/v0.20/t3", "two_rooms/v0.20", "colour"])
def test_the_cut_into_calls_and_the_culling_do_not_reach_the_bytes(dev, name):
    c = T.case(name)
    for per in (1, 3, None):
        vol, counts = _fuse(c, dev, views_per_call=per)
        assert not any(_differing(vol, c).values()) and tuple(counts) == (c["updates"], c["observed"]), per
    # the same volume object, zeroed and fused again; and with every brick taking every view
    first = [t.clone() for t in (vol.tsdf, vol.weight)]
    vol.reset()
    assert not vol.weight.any()
    poses, depth = c["poses"].to(dev).contiguous(), torch.from_numpy(c["depth"]).to(dev)
    rgb = None if c["rgb"] is None else torch.from_numpy(c["rgb"]).to(dev)
    rec = vol.integrate_enqueue(depth, poses, c["K"], rgb, c["depth_max"], flags=_lib.TSDF_NO_CULL)
    assert rec.tolist() == [c["updates"], c["observed"]]
    assert vol.tsdf.cpu().numpy().tobytes() == first[0].cpu().numpy().tobytes() and vol.weight.cpu().numpy().tobytes() == first[1].cpu().numpy().tobytes()
    none = vol.integrate_enqueue(depth[:0], poses[:0], c["K"], None if rgb is None else rgb[:0])          # n = 0: a zero record, nothing else
    assert none.tolist() == [0, 0] and vol.tsdf.cpu().numpy().tobytes() == first[0].cpu().numpy().tobytes()


def test_hosts_tensors_matrices_and_lists_are_accepted(dev):
    c = T.case("box/33x47/v0.20/t3")
    fx, fy, cx, cy = c["K"]
    Kmat = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    for depth, poses, K in ((torch.from_numpy(c["depth"]).to(dev), c["poses"].to(dev), torch.from_numpy(Kmat)), ([d for d in c["depth"]], [p for p in c["poses"]], Kmat),
                            (torch.from_numpy(c["depth"]).double(), c["poses"].numpy(), c["K"])):
        vol = tsdf.TSDFVolume(list(c["origin"]), c["voxel"], list(c["dims"]), c["trunc"], device=dev)
        vol.integrate(depth, poses, K)
        assert not any(_differing(vol, c).values())
    vol = tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], device=dev)
    for d, p in zip(c["depth"], c["poses"]):                      # a single image and pose at a time
        vol.integrate(d, p, c["K"])
    assert not any(_differing(vol, c).values())
    with pytest.raises(ValueError, match="color=True"):
        vol.integrate(c["depth"], c["poses"], c["K"], rgb=np.zeros(c["depth"].shape + (3,), np.float32))
    with pytest.raises(ValueError, match="poses"):
        vol.integrate(c["depth"], c["poses"][:3], c["K"])
    with pytest.raises(RuntimeError, match="trunc"):
        tsdf.TSDFVolume(c["origin"], c["voxel"], c["dims"], 0.0, device=dev).integrate(c["depth"], c["poses"], c["K"])
    assert not any(_differing(vol, c).values())


# ------------------------------------------------------------------------------------------------------------- 2. the mesh
@pytest.mark.parametrize("name", sorted(T.BOX_CASES))
def test_extract_mesh_equals_the_restatement_and_lies_on_the_walls(dev, name):
    c = T.case(name)
    vol, _ = _fuse(c, dev)
    m = vol.extract_mesh()
    want_v, want_f, _ = T.extract_mesh(c["state"], c["origin"], c["voxel"])
    assert isinstance(m, mesh_mod.Mesh) and m.vertices.dtype == np.float64 and m.faces.dtype == np.int64 and m.vertex_colors is None
    assert np.array_equal(m.faces, want_f) and np.array_equal(m.vertices, want_v)
    assert np.array_equal(_words(vol.volume()), _words(T.marching_volume(c["state"])))
    _, _, lo, hi = R.box_room()
    d = T.wall_distance(m.vertices[np.unique(m.faces)], lo, hi) / c["voxel"]
    print(f"{name}: faces {len(m.faces)}, wall distance in voxels: mean {d.mean():.3f}, p95 {np.percentile(d, 95):.3f}, max {d.max():.3f}")
    assert d.mean() <= T.MEAN_GATE and d.max() <= T.MAX_GATE
    if name == "box/33x47/v0.20/t3":
        got = ev.reconstruction_metrics(m, R.box_room()[:2], n_samples=4096)
        print(f"{name}: reconstruction metrics against the 12 triangles (not gated; sampling-limited): {got}")


def test_vertex_colours_equal_the_restatement(dev):
    c = T.case("colour")
    vol, _ = _fuse(c, dev)
    m = vol.extract_mesh()
    want_v, want_f, index_v = T.extract_mesh(c["state"], c["origin"], c["voxel"])
    want_c = T.sample_color(index_v, c["state"]["weight"], c["state"]["color"])
    assert np.array_equal(m.faces, want_f) and np.array_equal(m.vertices, want_v)
    assert m.vertex_colors.dtype == np.float32 and m.vertex_colors.shape == (len(want_v), 3)
    print(f"colour: {len(want_v)} vertices, differing colour words {int((_words(m.vertex_colors) != _words(want_c)).sum())}")
    assert np.array_equal(_words(m.vertex_colors), _words(want_c))
    g = np.random.default_rng(5)                                  # points all over, outside the volume and not finite too
    pts = g.uniform(-2.0, max(c["dims"]) + 2.0, (500, 3))
    pts[:3] = [[np.nan, 1, 1], [np.inf, 2, 2], [3, -np.inf, 1]]
    got = vol.sample_enqueue(torch.from_numpy(pts).to(dev)).cpu().numpy()
    assert np.array_equal(_words(got), _words(T.sample_color(pts, c["state"]["weight"], c["state"]["color"])))


# ------------------------------------------------------------------------------------------------------------- 3. the loop
def test_mesh_to_depth_to_mesh(dev, monkeypatch):
    """marched room -> render_mesh_depth from the 20 views -> tsdf_mesh_from_frames -> depth_l1 against the marched room: the loop
    the fusion closes, on device tensors from end to end"""
    room = R.marched_room(24)
    H, W, K = R.SIZES["40x56"]
    poses = T.box_poses20().to(dev)
    depth, _ = mr.render_mesh_depth(room, poses, K, H, W)
    seen = []
    real = tsdf.TSDFVolume.integrate_enqueue

    def spy(self, d, p, *a, **kw):
        seen.append((d.is_cuda, d.data_ptr(), p.data_ptr()))
        return real(self, d, p, *a, **kw)
    monkeypatch.setattr(tsdf.TSDFVolume, "integrate_enqueue", spy)
    mesh, vol = tsdf.tsdf_mesh_from_frames(depth, poses, K, 0.1, return_volume=True)
    assert seen == [(True, depth.data_ptr(), poses.data_ptr())]                 # the rendered images themselves, no copy through the host
    assert vol.trunc == pytest.approx(0.4) and len(mesh.faces) > 1000
    got = mr.depth_l1(mesh, room, poses, K, H, W)
    print(f"loop: volume {vol.dims}, {len(mesh.faces)} faces, depth L1 against the marched room {got.l1 * 1e3:.2f} mm "
          f"(both {got.both:.4f}, l1_both {got.l1_both * 1e3:.2f} mm)")
    assert got.both > 0
    with pytest.raises(ValueError, match="voxel size 1e-05"):
        tsdf.tsdf_mesh_from_frames(depth, poses, K, 1e-5)


def test_mesh_from_rendered_depth_is_the_fusion_of_the_rendered_images(dev):
    from mipsfusion_amd import inference
    from mipsfusion_amd.model import JointEncoding
    cfg = synth.config_plumbing()
    bound = np.array(cfg["mapping"]["bound"])
    torch.manual_seed(0)
    model = JointEncoding(cfg, torch.from_numpy(bound), torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))).to(dev).eval()
    with torch.no_grad():
        model.embed_fn.params.copy_((torch.randn(model.embed_fn.params.shape) * 0.2).to(dev))
    H, W, K = 12, 16, (12.0, 12.0, 7.5, 5.5)
    rays = synth.camera_rays(H, W, *K)
    first = R.pose_of((0.1, -0.2, 0.05), 0.2, 0.1)
    local = torch.stack([R.pose_of((0.0, 0.0, 0.0), 0.0, 0.0), R.pose_of((0.2, 0.1, -0.1), -0.3, 0.05)])
    torch.manual_seed(7)
    mesh, vol = tsdf.mesh_from_rendered_depth(model, rays, local, first, H, W, K, 0.25, bounds=bound, return_volume=True)
    torch.manual_seed(7)
    images = [inference.render_full_img(model, rays, p.to(dev), None, H, W) for p in local]
    by_hand = tsdf.TSDFVolume(bound[:, 0], 0.25, vol.dims, 1.0, color=True, device=dev)
    by_hand.integrate(torch.stack([d for _, d in images]), first.to(dev) @ local.to(dev), K, rgb=torch.stack([c for c, _ in images]))
    for a, b in ((vol.tsdf, by_hand.tsdf), (vol.weight, by_hand.weight), (vol.color, by_hand.color)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    print(f"rendered depth: volume {vol.dims}, {int((vol.weight > 0).sum())} voxels observed, {len(mesh.faces)} faces")
    assert isinstance(mesh, mesh_mod.Mesh)
