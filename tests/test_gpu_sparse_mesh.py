"""GPU tests of the sparse volume's mesh marched brick by brick (SparseTSDFVolume.extract_mesh_bricks, csrc/sparse_mesh.hip,
include/mipsf_sparse_mesh.h) against the restatement of tests/sparse_mesh_cpu.py fed the device's slot order.  Both sides evaluate
the same fp32 and float64 expressions in the same order on the same words, so the soup, tri_slot, the offsets, the vertices, the faces
and the colours are compared for EQUALITY.  tests/test_sparse_mesh_cpu.py holds the restatement to the dense one."""
import ctypes as C

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, mesh, sparse_tsdf

from . import sparse_cpu as S
from . import sparse_mesh_cpu as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def _bits(a, dtype=np.float32):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype)
    return a.view(np.uint32 if dtype == np.float32 else np.uint64)


def _fuse(c, dev, capacity=None, **kw):
    vol = sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], c["sp"]["capacity"] if capacity is None else capacity,
                                       color=c["rgb"] is not None, max_weight=c["max_weight"], device=dev)
    counts = vol.integrate(c["depth"], c["poses"], c["K"], c["rgb"], c["depth_max"], **kw)
    return vol, counts


def _order(vol):
    n = min(int(vol.count.item()), vol.capacity)
    return vol.slot_brick[:n].cpu().tolist()


def _equals_the_restatement(name, vol, sp, min_weight=1.0):
    """every output of the device against sparse_mesh_cpu.mesh fed the device's slot order; prints, then asserts -> (Mesh, restatement)"""
    order = _order(vol)
    assert sorted(order) == sorted(sp["slot_brick"]), name
    want = B.mesh(sp, min_weight, bricks=order)
    n, T = len(order), len(want["soup"])
    soup, tri_slot, offsets, cells = vol.brick_soup_enqueue(min_weight, return_cells=True)
    off = offsets.cpu().numpy().astype(np.int64)
    print(f"{name}: min_weight {min_weight:g}, {n} slots of {vol.capacity}, T {soup.shape[0]} (restatement {T}), V {len(want['index'])}, F {len(want['faces'])}")
    assert soup.shape[0] == T and off[-1] == T and np.array_equal(off[:n + 1], want["offsets"]) and (off[n:] == T).all(), name
    assert tuple(soup.shape) == (T, 3, 3) and soup.dtype == torch.float32 and tri_slot.dtype == torch.int32 and soup.is_cuda
    assert np.array_equal(_bits(soup), _bits(want["soup"])), name
    assert np.array_equal(tri_slot.cpu().numpy(), want["tri_slot"]) and np.array_equal(cells.cpu().numpy(), want["cells"]), name
    v, f = vol.weld_bricks(soup, tri_slot)
    assert v.dtype == torch.float64 and np.array_equal(_bits(v, np.float64), _bits(want["index"], np.float64)), name
    assert np.array_equal(f.cpu().numpy(), want["all_faces"]), name
    m = vol.extract_mesh_bricks(min_weight)
    assert isinstance(m, mesh.Mesh) and m.vertices.dtype == np.float64 and m.faces.dtype == np.int64
    assert np.array_equal(m.faces, want["faces"]) and np.array_equal(_bits(m.vertices, np.float64), _bits(want["vertices"], np.float64)), name
    if want["colors"] is None:
        assert m.vertex_colors is None
    else:
        assert m.vertex_colors.dtype == np.float32 and np.array_equal(_bits(m.vertex_colors), _bits(want["colors"])), name
    return m, want


# ------------------------------------------------------------------------------------------------------------- 1. the device = the restatement
@pytest.mark.parametrize("name", S.GPU_CASES)
def test_soup_weld_faces_and_colour_equal_the_restatement(dev, name):
    c = S.case(name)
    vol, counts = _fuse(c, dev)
    assert counts.dropped == 0
    m, want = _equals_the_restatement(name, vol, c["sp"])
    if name == "1x5x70":                                         # bricks in use, and nothing to march: the empty mesh
        assert counts.bricks_in_use > 0 and m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
        assert not vol.brick_soup_enqueue()[2].any()
    if name == "one_voxel":
        assert len(m.faces) == 0
    if name == S.VIRTUAL:                                        # the whole 2048^3 grid in one call; the windowed call refuses it
        assert vol.dims == S.VIRTUAL_DIMS and len(m.faces) == 17176 and len(m.vertices) == 8963
        with pytest.raises(ValueError, match="window of 2048 x 2048 x 2048"):
            vol.extract_mesh(window=((0, 0, 0), c["dims"]))
        lo = np.asarray(S.VIRTUAL_BRICK, np.float64) * B.BRICK
        assert (want["index"].min(0) > lo - 8).all() and (want["index"].max(0) < lo + 80).all()
    if name == "box/40x56/v0.10/t4":
        assert (len(want["soup"]), len(m.vertices), len(m.faces)) == (17194, 8963, 17176)


def test_min_weight_two(dev):
    c = S.case("box/40x56/v0.10/t4")
    vol, _ = _fuse(c, dev)
    m, _ = _equals_the_restatement("box/40x56/v0.10/t4", vol, c["sp"], 2.0)
    assert 1000 < len(m.faces) < 17176


@pytest.mark.parametrize("name", B.HAND_CASES)
def test_hand_made_states_on_3x3x2_bricks(dev, name):
    sp, beyond = B.hand_case(name)
    vol = B.to_device(sp, dev, beyond)
    for min_weight in (1.0, 2.0):
        m, want = _equals_the_restatement(name, vol, sp, min_weight)
        assert len(m.faces) > 100
    if name == "plane_snap":
        assert len(want["faces"]) < len(want["soup"])
    if name == "through_faces":
        assert m.vertices.min() >= 0.5 * sp["voxel"]


# ------------------------------------------------------------------------------------------------------------- 2. a full pool
def test_a_full_pool_meshes_what_got_slots_and_moves_no_guard_word(dev):
    name = "box/40x56/v0.10/t4"
    c = S.case(name)
    cap = c["counts"]["in_use"] // 2
    sp, _ = S.fuse(name, capacity=cap)
    vol = sparse_tsdf.SparseTSDFVolume(c["origin"], c["voxel"], c["dims"], c["trunc"], cap, device=dev)
    guard = {}
    for key, fill in (("tsdf", 0.0), ("weight", 7.0), ("slot_brick", 0), ("_birth", -77)):
        old = getattr(vol, key)
        new = torch.full((cap + 2,) + tuple(old.shape[1:]), fill, dtype=old.dtype, device=dev)      # the guards hold a surface: tsdf 0, weight 7
        new[:cap] = old
        guard[key] = new
        setattr(vol, key, new[:cap])
    vol._bind()
    counts = vol.integrate(c["depth"], c["poses"], c["K"], None, c["depth_max"])
    assert counts.dropped > 0 and counts.bricks_in_use == cap
    m, want = _equals_the_restatement(name + "/half", vol, sp)
    assert 1000 < len(m.faces) < 17176
    for key, fill in (("tsdf", 0.0), ("weight", 7.0), ("slot_brick", 0), ("_birth", -77)):
        assert bool((guard[key][cap:] == fill).all()), key


# ------------------------------------------------------------------------------------------------------------- 3. the dense kernels
def test_a_slot_s_soup_is_the_dense_marcher_s_on_its_padded_block(dev):
    c = S.case("colour")
    vol, _ = _fuse(c, dev)
    soup, tri_slot, offsets = vol.brick_soup_enqueue()
    off = offsets.cpu().tolist()
    dense = vol.to_dense((0, 0, 0), c["dims"]).volume(1.0)
    pad = [int(n * b) - d + 1 for n, b, d in zip(vol.bricks, B.BRICK, c["dims"])]
    padded = torch.nn.functional.pad(dense, (1, pad[2], 1, pad[1], 1, pad[0]), value=float("-inf"))
    coords = vol.allocated_bricks()
    busiest = np.argsort(np.diff(off[:len(coords) + 1]))[::-1][:3]
    for s in list(busiest) + [0]:
        lo = coords[s] * B.BRICK                                 # base + 1, and the padding shifted everything by 1
        block = padded[lo[0]:lo[0] + 10, lo[1]:lo[1] + 10, lo[2]:lo[2] + 18].contiguous()
        want, _ = mesh.triangle_soup(block, 0.0, 1.0)
        got = soup[off[s]:off[s + 1]]
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), s
        assert bool((tri_slot[off[s]:off[s + 1]] == int(s)).all())
    assert off[int(busiest[0]) + 1] - off[int(busiest[0])] > 50


# ------------------------------------------------------------------------------------------------------------- 4. repeatability
def _triangles(m):
    """the mesh as a sorted array of triangles, each its nine float64 words rotated to start at its smallest vertex"""
    t = m.vertices[m.faces]                                      # [F,3,3]
    key = np.ascontiguousarray(t).view(np.uint64).reshape(len(t), 3, 3)
    first = np.lexsort((key[..., 2], key[..., 1], key[..., 0]), axis=1)[:, 0]
    rot = np.stack([key[np.arange(len(t)), (first + s) % 3] for s in range(3)], 1).reshape(len(t), 9)
    return rot[np.lexsort(rot.T[::-1])]


def test_two_calls_give_the_same_bytes_and_another_cut_the_same_triangles(dev):
    c = S.case("two_rooms/v0.20")
    vol, _ = _fuse(c, dev)
    a, b = vol.brick_soup_enqueue(return_cells=True), vol.brick_soup_enqueue(return_cells=True)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    va, fa = vol.weld_bricks(a[0], a[1])
    vb, fb = vol.weld_bricks(b[0], b[1])
    assert torch.equal(va.view(torch.int64), vb.view(torch.int64)) and torch.equal(fa, fb)
    m = vol.extract_mesh_bricks()
    cut, _ = _fuse(c, dev, views_per_call=1)
    assert _order(cut) != _order(vol)                            # the slots are numbered differently, so the soup's order differs
    m2 = cut.extract_mesh_bricks()
    assert len(m2.faces) == len(m.faces) and len(m2.vertices) == len(m.vertices) and np.array_equal(_triangles(m), _triangles(m2))


def test_mesh_from_frames_with_bricks(dev):
    c = S.case(S.VIRTUAL)
    bounds = np.stack([c["origin"], c["origin"] + c["voxel"] * (np.asarray(c["dims"]) - 1.5)], 1)
    args = (c["depth"], c["poses"], c["K"], c["voxel"], 1024, c["trunc"])
    m, vol = sparse_tsdf.sparse_tsdf_mesh_from_frames(*args, bounds=bounds, device=dev, bricks=True, return_volume=True)
    own = vol.extract_mesh_bricks()
    assert vol.dims == S.VIRTUAL_DIMS and np.array_equal(m.faces, own.faces) and np.array_equal(_bits(m.vertices, np.float64), _bits(own.vertices, np.float64))
    assert len(m.faces) == 17176
    # the default is the windowed path
    d = sparse_tsdf.sparse_tsdf_mesh_from_frames(*args, bounds=bounds, device=dev)
    w = vol.extract_mesh()
    assert np.array_equal(d.faces, w.faces) and np.array_equal(_bits(d.vertices, np.float64), _bits(w.vertices, np.float64))
    assert len(d.faces) == len(m.faces) and len(d.vertices) == len(m.vertices)


# ------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_carry_their_messages(dev):
    sp, beyond = B.hand_case("sphere")
    vol = B.to_device(sp, dev, beyond)
    soup, tri_slot, _ = vol.brick_soup_enqueue()
    T = soup.shape[0]
    scratch = torch.empty(_lib.buffer_size(_lib.SIZE_MCUBES_WELD_WORDS, T) // 2 + 1, dtype=torch.int64, device=dev)
    vertices, faces, counts = torch.empty(3 * T, 3, dtype=torch.float64, device=dev), torch.empty(T, 3, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)

    def weld(**kw):
        a = _lib.SparseMeshWeldArgs.new(**dict(dict(T=T, capacity_tris=T, max_rounds=2, vol=vol._vol, soup=soup.data_ptr(), tri_slot=tri_slot.data_ptr(),
                                                    scratch=scratch.data_ptr(), vertices=vertices.data_ptr(), faces=faces.data_ptr(), counts=counts.data_ptr()), **kw))
        _lib.check(_lib.lib().mipsf_sparse_mesh_weld(C.byref(a), _lib.stream_ptr()), "sparse_mesh_weld")

    weld()
    with pytest.raises(RuntimeError, match=f"capacity_tris {T - 1} is below the {T} triangles"):
        weld(capacity_tris=T - 1)
    with pytest.raises(RuntimeError, match="are too many for the weld table"):
        weld(T=0x10000000, capacity_tris=0x10000000)
    with pytest.raises(RuntimeError, match="null pointer"):
        weld(tri_slot=None)
    with pytest.raises(RuntimeError, match="max_rounds 65"):
        weld(max_rounds=65)
    # a side above what 32-bit weld cells hold: the volume itself is accepted, fused into and counted; the weld names the side
    long = sparse_tsdf.SparseTSDFVolume((0.0, 0.0, 0.0), 0.05, (8, _lib.SPARSE_MESH_MAX_SIDE + 1, 16), 0.2, 4, device=dev)
    assert long.brick_soup_enqueue()[0].shape == (0, 3, 3)
    with pytest.raises(RuntimeError, match=f"a side of {_lib.SPARSE_MESH_MAX_SIDE + 1} voxels"):
        long.extract_mesh_bricks()
    ok = sparse_tsdf.SparseTSDFVolume((0.0, 0.0, 0.0), 0.05, (8, _lib.SPARSE_MESH_MAX_SIDE, 16), 0.2, 4, device=dev)
    assert len(ok.extract_mesh_bricks().faces) == 0
    # colour from a volume without colour
    with pytest.raises(ValueError, match="without colour"):
        vol.sample_enqueue(torch.zeros(1, 3, dtype=torch.float64, device=dev))
    a = _lib.SparseSampleArgs.new(m=1, vol=vol._vol, points=scratch.data_ptr(), out=vertices.data_ptr())
    with pytest.raises(RuntimeError, match="the volume has no colour"):
        _lib.check(_lib.lib().mipsf_sparse_sample(C.byref(a), _lib.stream_ptr()), "sparse_sample")
    # a struct of another size, and a null output of the count
    b = _lib.SparseMeshArgs.new(min_weight=1.0, vol=vol._vol)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(_lib.lib().mipsf_sparse_mesh_count(C.byref(b), _lib.stream_ptr()), "sparse_mesh_count")
    b.struct_size -= 8
    with pytest.raises(RuntimeError, match="struct_size"):
        _lib.check(_lib.lib().mipsf_sparse_mesh_count(C.byref(b), _lib.stream_ptr()), "sparse_mesh_count")
