"""GPU (-m gpu): the mesh extractor (csrc/mcubes.hip through mipsfusion_amd/mesh.py -> ctypes -> C ABI) against its numpy
restatement, exactly, against the meshes recorded from the upstream extractor, and end to end through extract_mesh2."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import inference, mesh, synth
from mipsfusion_amd.model import JointEncoding

from . import mcubes_cpu as mc
from .conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURES = ["sphere", "wavy", "noise", "plane_snap", "plane_snap2", "iso025", "trunc8"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def assert_identical(vol, iso, trunc, dev):
    """device == restatement: soup, cell ids, welded vertices (bit patterns) and faces"""
    t_dev, c_dev = mesh.triangle_soup(torch.from_numpy(vol).to(dev), iso, trunc)
    t_cpu, c_cpu = mc.soup(vol, iso, trunc)
    assert t_dev.shape == t_cpu.shape, (t_dev.shape, t_cpu.shape)
    assert np.array_equal(t_dev.cpu().numpy().view(np.int32), t_cpu.view(np.int32))
    assert np.array_equal(c_dev.cpu().numpy(), c_cpu)
    v, f, cells = mesh.marching_cubes(torch.from_numpy(vol).to(dev), iso, trunc, return_device=True, return_cells=True)
    rv, rf, rcells = mc.marching_cubes(vol, iso, trunc, return_cells=True)
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(v.astype(np.float32).view(np.int32), rv.astype(np.float32).view(np.int32))
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert np.array_equal(f, rf) and np.array_equal(cells.cpu().numpy(), rcells)
    return v, f


@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_restatement_and_matches_the_recorded_mesh(name, dev):
    g = load_golden("mcubes.npz")
    vol = g[name + "_vol"]
    iso, trunc = (float(t) for t in g[name + "_par"])
    v, f = assert_identical(vol, iso, trunc, dev)
    mc.compare_with_reference(name, v, f, g)
    mc.check_manifold(v, f, vol, iso, trunc)
    nv, nf = mesh.marching_cubes(vol, iso, trunc)                 # a numpy volume is uploaded; numpy comes back
    assert isinstance(nv, np.ndarray) and nv.dtype == np.float64 and nf.dtype == np.int64
    assert np.array_equal(nv, v) and np.array_equal(nf, f)


def random_volume(seed, shape):
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    v = np.zeros(shape)
    for _ in range(6):
        k = rng.uniform(0.15, 0.9, 3)
        v += rng.uniform(0.5, 1.5) * np.sin(k[0] * x + rng.uniform(0, 6)) * np.sin(k[1] * y + rng.uniform(0, 6)) * np.sin(k[2] * z + rng.uniform(0, 6))
    v += 0.05 * rng.standard_normal(shape)
    v = v.astype(np.float32)
    for _ in range(3):                      # invalid patches of the three kinds
        lo = [int(rng.integers(0, n)) for n in shape]
        sl = tuple(slice(l, l + int(rng.integers(1, 4))) for l in lo)
        v[sl] = rng.choice([-np.inf, np.inf, 9.0, -9.0, np.nan])
    return v


RAGGED = [(0, (2, 17, 19)), (1, (3, 33, 9)), (2, (129, 6, 7)), (3, (21, 3, 40)), (4, (17, 70, 2)), (5, (5, 5, 129)),
          (6, (33, 31, 35)), (7, (64, 9, 65)), (8, (12, 47, 31)), (9, (40, 41, 67))]


@pytest.mark.parametrize("seed,shape", RAGGED)
def test_device_equals_restatement_on_ragged_random_volumes(seed, shape, dev):
    rng = np.random.default_rng(100 + seed)
    iso = float(rng.choice([0.0, 0.25, -0.4]))
    trunc = float(rng.choice([3.0, 1.5, 8.0]))
    v, f = assert_identical(random_volume(seed, shape), iso, trunc, dev)
    if min(shape) < 3:
        assert len(v) == 0 and len(f) == 0          # no cell has all of its corners


def test_empty_results(dev):
    for vol in (np.full((9, 10, 11), -np.inf, np.float32), np.full((9, 10, 11), 5.0, np.float32),
                np.full((20, 20, 20), 1.0, np.float32), np.zeros((1, 1, 1), np.float32)):
        v, f = assert_identical(vol, 0.0, 3.0, dev)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_weld_takes_connected_components_of_a_chain(dev):
    """a - b - c with a, c not adjacent, the middle one last in the soup: two rounds do not settle it, the caller goes on"""
    soup = np.zeros((2, 3, 3), np.float32)
    soup[0, :, 0] = [1.00000, 1.000021, 1.000011]
    soup[1] = [[3.0, 1.0, 1.0], [3.0, 2.0, 1.0], [3.0, 1.0, 2.0]]
    assert mc.weld_cells(soup[0, :, 0]).tolist() == [100000, 100002, 100001]
    v, f = mesh.weld(torch.from_numpy(soup).to(dev))
    rv, rf = mc.weld(soup)
    assert len(rv) == 4 and rf.tolist() == [[0, 0, 0], [1, 2, 3]]
    assert np.array_equal(v.cpu().numpy().view(np.int32), rv.view(np.int32)) and np.array_equal(f.cpu().numpy(), rf)
    ff, = mesh.filter_faces(f)
    assert ff.cpu().tolist() == [[1, 2, 3]]


def test_two_runs_give_identical_bytes(dev):
    x, y, z = torch.meshgrid(*[torch.arange(128, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = (torch.sqrt((x - 63.2) ** 2 + (y - 64.9) ** 2 + (z - 61.7) ** 2) - 41.3
           + 2.0 * torch.sin(0.3 * x) * torch.sin(0.27 * y) * torch.sin(0.33 * z)).contiguous()
    a = mesh.marching_cubes(vol, 0.0, 3.0, return_device=True, return_cells=True)
    b = mesh.marching_cubes(vol, 0.0, 3.0, return_device=True, return_cells=True)
    assert a[1].shape[0] > 10000
    for s, t in zip(a, b):
        assert s.shape == t.shape and torch.equal(s.view(torch.int64) if s.dtype == torch.float64 else s,
                                                  t.view(torch.int64) if t.dtype == torch.float64 else t)


def test_extract_mesh2_end_to_end(dev, tmp_path, monkeypatch):
    cfg = synth.config_plumbing()
    cfg["data"]["translation"] = 0.25
    cfg["data"]["sc_factor"] = 2.0
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"])).to(dev)
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    torch.manual_seed(11)
    model = JointEncoding(cfg, bb.cpu(), nf).to(dev).eval()
    with torch.no_grad():
        model.embed_fn.params.copy_((torch.randn(model.embed_fn.params.shape) * 0.5).to(dev))
    c2w = synth.default_pose(cfg).to(dev, torch.float32)
    mcb = torch.tensor([[-0.8, 0.7], [-0.75, 0.8], [-0.6, 0.65]], dtype=torch.float64, device=dev)
    voxel_size = 0.05

    seen = []
    host_copies = []
    real_cpu = torch.Tensor.cpu

    def watched_cpu(self, *a, **k):
        if self.dim() >= 1 and seen and self.numel() >= seen[0].numel() and self.dtype == torch.float32 and self.dim() != 2:
            host_copies.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", watched_cpu)
    path = str(tmp_path / "out" / "mesh.ply")
    m = mesh.extract_mesh2(model.query_sdf, c2w, cfg, bb, marching_cube_bound=mcb, color_func=model.query_color,
                           voxel_size=voxel_size, mesh_savepath=path, on_volume=seen.append)
    monkeypatch.undo()
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].dtype == torch.float32
    assert not host_copies, f"the volume went to the host: {host_copies}"

    # the composition: own grid query -> host -> restatement -> the reference's numpy post-processing -> query_color
    tx, ty, tz = mesh.getVoxels(mcb[0, 1], mcb[0, 0], mcb[1, 1], mcb[1, 0], mcb[2, 1], mcb[2, 0], voxel_size, None)
    pts = torch.stack(torch.meshgrid(tx, ty, tz, indexing="ij"), -1).to(torch.float32)
    assert tuple(seen[0].shape) == tuple(pts.shape[:3])
    w2l = c2w.inverse()
    flat = mesh.transform_points(pts.reshape(-1, 3).to(bb[:, 0]).to(w2l), w2l)
    flat = (flat - bb[:, 0]) / (bb[:, 1] - bb[:, 0])
    raw = inference.query_in_batches(lambda p: model.query_sdf(p[:, None, :]), flat, 1024 * 64)
    vol = raw.cpu().numpy().astype(np.float32).reshape(pts.shape[:3])
    assert np.array_equal(vol, seen[0].cpu().numpy())
    v, f = mc.marching_cubes(vol, 0.0, 3.0)
    assert len(f) > 100, "the seeded model has no surface in the box: the test would show nothing"
    v[:, :3] /= np.array([[tx.shape[0] - 1, ty.shape[0] - 1, tz.shape[0] - 1]])
    txn, tyn, tzn = (t.numpy() for t in (tx, ty, tz))
    v = np.array([txn[-1] - txn[0], tyn[-1] - tyn[0], tzn[-1] - tzn[0]])[None] * v + np.array([txn[0], tyn[0], tzn[0]])
    v = v / cfg["data"]["sc_factor"] - cfg["data"]["translation"]
    assert m.faces.dtype == np.int64 and np.array_equal(m.faces, f)
    assert m.vertices.dtype == np.float64 and np.abs(m.vertices - v).max() <= 1e-12 * np.abs(v).max()
    vl = mesh.transform_points(torch.from_numpy(m.vertices).to(bb).to(w2l), w2l)
    col = inference.query_in_batches(lambda p: model.query_color(p[:, None, :]), vl, 1024 * 64).cpu().numpy().astype(np.float32)
    assert m.vertex_colors.shape == (len(v), 3) and np.array_equal(m.vertex_colors, col.reshape(len(v), -1))

    pv, pf, pc = mesh.load_ply(path)
    assert np.array_equal(pv, m.vertices) and np.array_equal(pf, m.faces) and np.array_equal(pc, mesh.colors_to_uint8(m.vertex_colors))

    # extract_mesh (no pose) and the normalised-colour switch run and agree on geometry where they must
    m1 = mesh.extract_mesh(model.query_sdf, cfg, bb, marching_cube_bound=mcb, color_func=model.query_color, resolution=24)
    assert m1.vertex_colors.shape == (len(m1.vertices), 3) and len(m1.faces) > 0
    m2 = mesh.extract_mesh2(model.query_sdf, c2w, cfg, bb, marching_cube_bound=mcb, color_func=model.query_color,
                            voxel_size=voxel_size, color_normalised=True)
    assert np.array_equal(m2.vertices, m.vertices) and np.array_equal(m2.faces, m.faces)
    assert not np.array_equal(m2.vertex_colors, m.vertex_colors)


@pytest.mark.slow
def test_256_cubed_volume_equals_the_restatement_in_slabs(dev):
    """F = 2V - 4 does NOT hold for a sphere under these semantics (measured: V 154093, F 308060): where a dual value is within
    1e-5 of the isovalue the vertices of a corner-cutting triangle snap together and the face is dropped while the welded
    vertex stays.  So the comparison is the stronger one: everything equal to the restatement run on the same data in slabs."""
    x, y, z = torch.meshgrid(*[torch.arange(256, device=dev, dtype=torch.float32)] * 3, indexing="ij")
    vol = (torch.sqrt((x - 127.3) ** 2 + (y - 128.6) ** 2 + (z - 126.1) ** 2) - 90.4).contiguous()
    v, f = mesh.marching_cubes(vol, 0.0, 3.0)
    rv, rf = mc.marching_cubes(vol.cpu().numpy(), 0.0, 3.0, slabs=True)
    print(f"256^3 sphere: V {len(v)}/{len(rv)} F {len(f)}/{len(rf)}")
    assert len(f) > 300000 and v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v, rv) and np.array_equal(f, rf)
    r = np.sqrt(((v - np.array([127.3, 128.6, 126.1])) ** 2).sum(1))
    assert np.abs(r - 90.4).max() < 0.05
