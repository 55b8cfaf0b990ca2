"""GPU tests of the mesh shader (mipsfusion_amd/mesh_render.py, csrc/shade.hip) against the float64 restatement of
tests/shade_cpu.py.  Both sides get the same fp32 words and evaluate the same float64 expressions in the same order (the vertex
normals add their faces in ascending index on both sides), so colour, normal and shaded words, vertex-normal words and the record
are compared for EQUALITY of bit patterns.  tests/test_shade_cpu.py holds the restatement to what is known without a GPU, and
shows that no pixel of these cases has an ambiguous facing decision."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, image_metrics as im, mesh as mesh_mod, mesh_render as mr

from . import raster_cpu as R
from . import shade_cpu as S

pytestmark = pytest.mark.gpu

MODES = {"flat": S.FLAT, "smooth": S.SMOOTH}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _same(got: mr.MeshRender, want, what):
    for key in ("color", "normals", "shaded"):
        g, w = getattr(got, key), want[key]
        assert (g is None) == (w is None), (what, key)
        if g is not None:
            diff = int((_bits(g) != _bits(w)).sum())
            print(f"{what}: {key} words that differ {diff} of {w.size}")
            assert np.array_equal(_bits(g), _bits(w)), (what, key)


def _device_inputs(c, dev):
    return (_t(c["vertices"], dev), _t(c["faces"], dev, np.int32), c["poses"].to(dev).contiguous(), _t(c["face"], dev, np.int32), _t(c["colors"], dev),
            _t(c["vertex_normals"], dev))


# ------------------------------------------------------------------------------------------------------------- 1. the pixel pass
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", S.SHADE_CASES)
def test_colour_normals_and_shading_equal_the_restatement(dev, name, mode):
    c = S.case(name)
    args = (c["poses"], c["K"], c["H"], c["W"], c["near"], c["far"])
    plain = mr.render_mesh((c["vertices"], c["faces"]), *args, normals=mode)
    assert plain.color is None and plain.normals.dtype == torch.float32 and tuple(plain.shaded.shape) == tuple(c["face"].shape)
    _same(plain, S.want(name, MODES[mode], colored=False), f"{name} {mode} no colours")
    coloured = mr.render_mesh(mesh_mod.Mesh(c["vertices"].astype(np.float64), c["faces"], c["colors"]), *args, normals=mode, background=S.BACKGROUND)
    _same(coloured, S.want(name, MODES[mode], background=S.BACKGROUND), f"{name} {mode} coloured")
    d, f = mr.render_mesh_depth((c["vertices"], c["faces"]), *args)
    for r in (plain, coloured):
        assert torch.equal(r.face, f) and torch.equal(r.depth.view(torch.int32), d.view(torch.int32))
    assert np.array_equal(f.cpu().numpy(), c["face"])
    # the record, and colour alone (no normal is computed: the second count is 0)
    v, faces, poses, face, cols, vn = _device_inputs(c, dev)
    shaded = torch.empty(face.shape, device=dev)
    rec = mr.shade_enqueue(v, faces, poses, c["K"], face, cols, vn, MODES[mode], shaded=shaded)
    assert tuple(int(x) for x in rec.cpu()) == S.want(name, MODES[mode])["record"]
    color = torch.empty(tuple(face.shape) + (3,), device=dev)
    rec = mr.shade_enqueue(v, faces, poses, c["K"], face, cols, None, MODES[mode], color=color)
    assert tuple(int(x) for x in rec.cpu()) == (S.want(name, S.FLAT)["record"][0], 0)
    assert np.array_equal(_bits(color), _bits(S.want(name, S.FLAT)["color"])) and np.array_equal(_bits(shaded), _bits(S.want(name, MODES[mode])["shaded"]))


def test_render_mesh_skips_the_normals_on_request(dev):
    c = S.case("one_face/40x56")
    r = mr.render_mesh((c["vertices"], c["faces"], c["colors"]), c["poses"], c["K"], c["H"], c["W"], normals=None)
    assert r.normals is None and r.shaded is None
    assert np.array_equal(_bits(r.color), _bits(S.want("one_face/40x56", S.FLAT)["color"]))
    with pytest.raises(ValueError, match="smooth"):
        mr.render_mesh((c["vertices"], c["faces"]), c["poses"], c["K"], c["H"], c["W"], normals="phong")


def _enqueue_all(c, dev, face_image, mode=S.SMOOTH, background=S.BACKGROUND, poses=None):
    v, faces, p, _, cols, vn = _device_inputs(c, dev)
    p = p if poses is None else poses
    face = _t(face_image, dev, np.int32)
    shape = tuple(face.shape)
    color, normals, shaded = torch.full(shape + (3,), -7.0, device=dev), torch.full(shape + (3,), -7.0, device=dev), torch.full(shape, -7.0, device=dev)
    record = torch.full((2,), 77, dtype=torch.int64, device=dev)
    mr.shade_enqueue(v, faces, p, c["K"], face, cols, vn, mode, background, color, normals, shaded, record)
    return mr.MeshRender(None, face, color, normals, shaded), tuple(int(x) for x in record.cpu())


def test_a_face_image_of_misses_and_of_indices_past_the_end(dev):
    c = S.case("box_room/33x47")
    F = len(c["faces"])
    empty = np.full_like(c["face"], -1)
    got, rec = _enqueue_all(c, dev, empty)
    assert rec == (0, 0) and not got.normals.any() and not got.shaded.any()
    assert np.array_equal(_bits(got.color), _bits(np.broadcast_to(np.asarray(S.BACKGROUND, np.float32), got.color.shape)))
    odd = c["face"].copy()
    odd[:, ::3, ::5], odd[:, 1::3, ::5], odd[:, 2::3, 1::5], odd[:, ::4, 2::5] = F, F + 5, 2 ** 31 - 1, -7
    want = S.shade(c["vertices"], c["faces"], c["poses"], c["K"], odd, c["colors"], c["vertex_normals"], S.SMOOTH, S.BACKGROUND)
    got, rec = _enqueue_all(c, dev, odd)
    _same(got, want, "indices past the end")
    assert rec == want["record"] and 0 < rec[0] < S.want("box_room/33x47", S.SMOOTH)["record"][0]


@pytest.mark.parametrize("H,W,K", [(1, 1, (40.0, 40.0, 0.0, 0.0)), (17, 33, (20.0, 21.0, 16.3, 8.2))], ids=["1x1", "17x33"])
def test_images_that_are_no_multiple_of_the_tile(dev, H, W, K):
    c = S.case("marched_24/33x47")
    face = R.render_depth(c["vertices"], c["faces"], c["poses"], K, H, W)[1]
    assert (face >= 0).all()
    for mode in (S.FLAT, S.SMOOTH):
        want = S.shade(c["vertices"], c["faces"], c["poses"], K, face, c["colors"], c["vertex_normals"], mode, S.BACKGROUND)
        got = mr.render_mesh((c["vertices"], c["faces"], c["colors"]), c["poses"], K, H, W, normals="flat" if mode == S.FLAT else "smooth",
                             background=S.BACKGROUND)
        assert np.array_equal(got.face.cpu().numpy(), face)
        _same(got, want, f"{H}x{W} mode {mode}")


def test_no_views_is_a_zero_record(dev):
    c = S.case("one_face/40x56")
    got, rec = _enqueue_all(c, dev, c["face"][:0], poses=c["poses"][:0].to(dev).contiguous())
    assert rec == (0, 0) and got.color.shape[0] == 0


def test_the_cut_into_launches_and_a_second_call_do_not_reach_the_bytes(dev):
    c = S.case("marched_24/33x47")
    mesh = (c["vertices"], c["faces"], c["colors"])
    args = (c["poses"], c["K"], c["H"], c["W"])
    one = mr.render_mesh(mesh, *args, background=S.BACKGROUND)
    for other in (mr.render_mesh(mesh, *args, background=S.BACKGROUND, views_per_launch=1), mr.render_mesh(mesh, *args, background=S.BACKGROUND,
                                                                                                      views_per_launch=len(c["poses"])),
                  mr.render_mesh(mesh, *args, background=S.BACKGROUND)):
        for a, b in zip(one, other):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    v, f = _t(c["vertices"], dev), _t(c["faces"], dev, np.int32)
    assert mr.vertex_normals_enqueue(v, f).cpu().numpy().tobytes() == mr.vertex_normals_enqueue(v, f).cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------- 2. vertex normals
def _normal_meshes():
    yield "marched_24", S.case("marched_24/33x47")["vertices"], S.case("marched_24/33x47")["faces"]
    yield "random_5000", S.case("random_5000/33x47")["vertices"], S.case("random_5000/33x47")["faces"]
    v, f = S.sphere()
    yield "sphere", v.astype(np.float32), f
    yield "one_face", S.case("one_face/40x56")["vertices"], S.case("one_face/40x56")["faces"]
    yield "one_vertex_one_invalid_face", np.array([[0.5, 0.25, -1.0]], np.float32), np.array([[0, 0, 1]])
    yield "fan_2000", *S.fan(2000)
    v, f = S.fan(40)                      # a segment just past the one-lane limit, NaN and repeated vertices, a cancelling pair, an isolated vertex
    v = np.concatenate([v, [[np.nan, 0.0, 0.0], [3.0, 3.0, 3.0], [4.0, 3.0, 3.0], [3.0, 4.0, 3.0], [9.0, 9.0, 9.0]]]).astype(np.float32)
    f = np.concatenate([f[::-1], [[0, 1, 41], [0, 0, 0], [0, 5, 5], [42, 43, 44], [42, 44, 43], [0, 1, 99], [-1, 1, 2]]])
    yield "fan_40_with_odd_faces", v, f


@pytest.mark.parametrize("name,v,f", list(_normal_meshes()), ids=[m[0] for m in _normal_meshes()])
def test_vertex_normals_equal_the_restatement(dev, name, v, f):
    want = S.vertex_normals(v, f)
    got = mr.vertex_normals(mesh_mod.Mesh(v.astype(np.float64), f, None))
    assert got.dtype == np.float32 and got.shape == want.shape
    print(f"{name}: {len(v)} vertices, {len(f)} faces, words that differ {int((_bits(got) != _bits(want)).sum())}, vertices without a normal "
          f"{int((~want.any(1)).sum())}")
    assert np.array_equal(_bits(got), _bits(want))
    if name == "fan_40_with_odd_faces":
        assert want[0].any() and not want[41:].any()
    if name == "fan_2000":
        corners = np.bincount(f.reshape(-1), minlength=len(v))
        assert corners[0] == 2000 > _lib.SHADE_SHORT_SEGMENT and want[0].any()


def test_no_faces_and_no_vertices(dev):
    v = _t(np.ones((5, 3)), dev)
    none = torch.zeros(0, 3, dtype=torch.int32, device=dev)
    assert not mr.vertex_normals_enqueue(v, none).any()
    assert tuple(mr.vertex_normals_enqueue(v[:0], none).shape) == (0, 3)


# ------------------------------------------------------------------------------------------------------------- 3. graphs
def test_both_entry_points_replay_from_a_graph(dev):
    c, other = S.case("marched_24/33x47"), S.case("box_room/33x47")
    v, faces, poses, face, cols, vn = _device_inputs(c, dev)
    shape = tuple(face.shape)
    color, normals, shaded = torch.empty(shape + (3,), device=dev), torch.empty(shape + (3,), device=dev), torch.empty(shape, device=dev)
    record = torch.empty(2, dtype=torch.int64, device=dev)
    out = torch.empty_like(v)
    ws = torch.empty(int(_lib.lib().mipsf_shade_workspace_bytes(_lib.SHADE_WS_VERTEX_NORMALS, v.shape[0], faces.shape[0])), dtype=torch.uint8, device=dev)

    def run():
        mr.vertex_normals_enqueue(v, faces, out, ws)
        mr.shade_enqueue(v, faces, poses, c["K"], face, cols, out, S.SMOOTH, S.BACKGROUND, color, normals, shaded, record)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        run()                                                    # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):                     # one stream, one chain of launches: no parallel branches
        run()
    want = S.want("marched_24/33x47", S.SMOOTH, background=S.BACKGROUND)
    for k in range(2):
        for t in (color, normals, shaded, out):
            t.fill_(-3.0)
        record.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        _same(mr.MeshRender(None, face, color, normals, shaded), want, f"replay {k}")
        assert np.array_equal(_bits(out), _bits(c["vertex_normals"])) and tuple(int(x) for x in record.cpu()) == want["record"]
    # new poses in the same buffers: the replay follows them
    poses.copy_(other["poses"][3:3 + len(poses)].to(dev))
    face.copy_(mr.render_mesh_depth((v, faces), poses, c["K"], c["H"], c["W"])[1])
    g.replay()
    torch.cuda.synchronize()
    moved = S.shade(c["vertices"], c["faces"], poses.cpu(), c["K"], face.cpu().numpy(), c["colors"], c["vertex_normals"], S.SMOOTH, S.BACKGROUND)
    _same(mr.MeshRender(None, face, color, normals, shaded), moved, "replay on new poses")


# ------------------------------------------------------------------------------------------------------------- 4. the chain
def test_mesh_render_metrics_is_image_metrics_of_the_render(dev):
    ch = S.chain_case()
    mesh = mesh_mod.Mesh(ch["vertices"].astype(np.float64), ch["faces"], ch["colors"])
    got = mr.mesh_render_metrics(mesh, ch["poses"], ch["K"], ch["rgb"], ch["depth"], ms_ssim=False)
    r = mr.render_mesh(mesh, ch["poses"], ch["K"], ch["H"], ch["W"], normals=None)
    gt_d = _t(ch["depth"], dev)
    mask = (r.face >= 0) & (gt_d > 0)
    by_hand = im.image_metrics(r.color, _t(ch["rgb"], dev), 1.0, False, mask)
    same = lambda a, b: a._replace(ms_ssim=0.0, ms_ssim_per_view=()) == b._replace(ms_ssim=0.0, ms_ssim_per_view=())      # noqa: E731 (nan: not asked for)
    assert same(got.image, by_hand) and got.n_views == len(ch["poses"])
    l1 = [float((r.depth[k].double() - gt_d[k].double()).abs()[mask[k]].mean()) for k in range(got.n_views)]
    print(f"chain on the device: PSNR {got.image.psnr:.2f} dB, SSIM {got.image.ssim:.4f}, depth L1 {got.depth_l1 * 1e3:.2f} mm, coverage {got.coverage:.4f}")
    assert np.allclose(got.depth_l1_per_view, l1, rtol=1e-12, atol=0) and got.coverage == float(mask.sum()) / mask.numel()
    want = S.shade(ch["vertices"], ch["faces"], ch["poses"], ch["K"], r.face.cpu().numpy(), ch["colors"], None, S.FLAT, want_normals=False)
    assert np.array_equal(_bits(r.color), _bits(want["color"]))
    no_depth = mr.mesh_render_metrics(mesh, ch["poses"], ch["K"], ch["rgb"], ms_ssim=False)
    assert np.isnan(no_depth.depth_l1) and same(no_depth.image, im.image_metrics(r.color, _t(ch["rgb"], dev), 1.0, False, r.face >= 0))
    with pytest.raises(ValueError, match="no vertex colours"):
        mr.mesh_render_metrics((ch["vertices"], ch["faces"]), ch["poses"], ch["K"], ch["rgb"])


# ------------------------------------------------------------------------------------------------------------- 5. refusals
def test_what_is_refused_leaves_the_outputs_alone(dev):
    c = S.case("box_room/33x47")
    v, faces, poses, face, cols, vn = _device_inputs(c, dev)
    shape = tuple(face.shape)
    color, normals = torch.full(shape + (3,), -7.0, device=dev), torch.full(shape + (3,), -7.0, device=dev)
    with pytest.raises(RuntimeError, match="without vertex_normals"):
        mr.shade_enqueue(v, faces, poses, c["K"], face, cols, None, S.SMOOTH, normals=normals)
    with pytest.raises(RuntimeError, match="without vertex colours"):
        mr.shade_enqueue(v, faces, poses, c["K"], face, None, vn, S.FLAT, color=color)
    with pytest.raises(RuntimeError, match="flags"):
        mr.shade_enqueue(v, faces, poses, c["K"], face, cols, vn, 3, color=color)
    with pytest.raises(RuntimeError, match="intrinsics"):
        mr.shade_enqueue(v, faces, poses, (0.0, 35.0, 1.0, 1.0), face, cols, vn, S.FLAT, color=color)
    with pytest.raises(RuntimeError, match="without faces"):
        mr.shade_enqueue(v, faces[:0], poses, c["K"], face, cols, vn, S.FLAT, color=color)
    torch.cuda.synchronize()
    assert bool((color == -7.0).all()) and bool((normals == -7.0).all())
