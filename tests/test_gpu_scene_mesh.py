"""GPU (-m gpu): the scene mesher (csrc/fuse.hip through mipsfusion_amd/scene_mesh.py -> ctypes -> C ABI) against its numpy /
CPU-torch restatement (tests/scene_mesh_cpu.py) and against what the upstream's own code recorded (tests/golden/scene_mesh.npz).

Tolerances.  Visibility is a chain of fp32 comparisons: a point is *ambiguous* when a float64 evaluation puts a deciding u or v
within 1e-2 px of a threshold or z within 1e-5 m of one (fp32 evaluation of |u| <~ 1e3 px is good to about 1e-3 px; the margin is
ten times that); every other point must agree exactly, and ambiguous points may be at most 0.5 % of a case
(tests/test_scene_mesh_cpu.py asserts that share on the same inputs).  Blended SDF values are unit-scale quantities: 1e-5
absolute, the project's gate for them (DESIGN.md "Tolerances")."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import mesh, scene_mesh as sm, synth
from mipsfusion_amd.model import JointEncoding

from . import scene_mesh_cpu as sc
from .conftest import load_golden

pytestmark = pytest.mark.gpu

K, W, H = sc.CAMERA["K"], sc.CAMERA["W"], sc.CAMERA["H"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------- 1. visibility
def test_point_mask_equals_the_recorded_mask(dev):
    g = load_golden("scene_mesh.npz")
    Wg, Hg = (int(t) for t in g["vis_WH"])
    got = sm.point_mask(torch.from_numpy(g["vis_points"]).to(dev), g["vis_c2w"], g["vis_max_depth"], g["vis_K"], Wg, Hg)
    assert got.dtype == torch.bool and got.is_cuda
    amb = sc.ambiguous_points(g["vis_points"], g["vis_c2w"], g["vis_max_depth"], g["vis_K"], Wg, Hg)
    diff = got.cpu().numpy() != g["vis_mask"]
    print(f"golden: {int(diff.sum())} differences, {int(amb.sum())} ambiguous of {len(amb)}")
    assert amb.mean() <= sc.AMBIG_CAP and not (diff & ~amb).any()


@pytest.mark.parametrize("seed,n,k", sc.VIS_CASES)
def test_point_mask_equals_the_restatement(seed, n, k, dev):
    pts, c2w, md = sc.visibility_case(seed, n, k)
    got = sm.point_mask(torch.from_numpy(pts).to(dev), torch.from_numpy(c2w), torch.from_numpy(md).to(dev), K, W, H).cpu().numpy()
    want = sc.point_mask(pts, c2w, md, K, W, H)
    amb = sc.ambiguous_points(pts, c2w, md, K, W, H)
    diff = got != want
    print(f"n {n} k {k}: seen {int(want.sum())}, {int(diff.sum())} differences, {int(amb.sum())} ambiguous")
    assert amb.sum() <= sc.AMBIG_CAP * n and not (diff & ~amb).any()
    if n >= 1000:
        assert 0.02 < want.mean() < 0.98                       # the case tests something


@pytest.mark.parametrize("seed,dims", [(0, (33, 21, 70)), (1, (1, 65, 64)), (2, (130, 7, 129))])
def test_grid_description_gives_the_bytes_of_explicit_points(seed, dims, dev):
    rng = np.random.default_rng(50 + seed)
    ticks = [np.linspace(lo, lo + ext, n) for lo, ext, n in zip((-4.0, -3.0, 0.5), (8.0, 6.0, 9.0), dims)]
    _, c2w, md = sc.visibility_case(seed, 1, 9)
    for _ in range(3):
        lo = [int(rng.integers(0, n)) for n in dims]
        size = [int(rng.integers(1, n - l + 1)) for n, l in zip(dims, lo)]
        sub = [t[l:l + s] for t, l, s in zip(ticks, lo, size)]
        pts = sc.grid_points(sub).astype(np.float32)
        a = sm.grid_point_mask(ticks, c2w, md, K, W, H, lo=lo, size=size, device=dev)
        b = sm.point_mask(torch.from_numpy(pts).to(dev), c2w, md, K, W, H)
        assert tuple(a.shape) == tuple(size) and torch.equal(a.reshape(-1), b)
    whole = sm.grid_point_mask(ticks, c2w, md, K, W, H, device=dev)
    assert torch.equal(whole.reshape(-1), sm.point_mask(torch.from_numpy(sc.grid_points(ticks).astype(np.float32)).to(dev), c2w, md, K, W, H))
    assert whole.any() and not whole.all()


def test_max_depth_of_keyframes_from_the_ray_store(dev):
    from mipsfusion_amd.keyframe_rays import DeviceRayDB
    db = DeviceRayDB(6, 50, dev)
    rays = torch.rand((6, 50, 7), generator=torch.Generator().manual_seed(4))
    for j in range(6):
        db.rays[j].copy_(rays[j])
    got = sm.keyframe_max_depth(db.rays, [4, 0, 5])
    assert got.is_cuda and torch.equal(got.cpu(), rays[[4, 0, 5], :, 6].amax(1))


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="GPU only"):
        sm.point_mask(torch.zeros(4, 3), np.eye(4)[None], np.ones(1), K, W, H)


# ----------------------------------------------------------------------------------------------------------- 2. fusion
CFG = {"grid": {"tcnn_encoding": True, "use_bound_normalize": True}, "cam": {"W": W, "H": H},
       "mapping": {"bound": [[-3.0, 3.5], [-2.5, 2.5], [-4.0, 4.5]], "localMLP_max_len": [7.0, 7.0, 7.0]},
       "training": {"norm_factor": 1.0}, "mesh": {"voxel_final": 0.1}}


def analytic_submaps(entropies=None):
    """three sub-maps on a diagonal (the grid's off-diagonal corners lie in no box), overlapping pairwise, one oriented box"""
    centres = [(-1.2, -0.6, -1.5), (0.1, 0.0, 0.2), (1.3, 0.7, 2.0)]
    out = []
    for i, c in enumerate(centres):
        c = np.array(c)
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = sc.rot((0.3, 1.0, 0.2), 0.4 * i), c * 0.5
        c2w, md = sc.ring_of_keyframes(c, 7 + 3 * i, 70 + i)
        ent = sc.wavy_entropy(0.12, 0.1) if entropies is None else entropies[i]
        model = sc.Analytic(CFG, pose, sc.sphere((0.0, 0.1, 0.3), 1.9 + 0.02 * i), ent,
                         rgb=lambda w, i=i: torch.stack([torch.sin(2 * w[:, 0] + i), torch.cos(3 * w[:, 1]), 0.5 * w[:, 2] - i], -1))
        aabb = np.stack([c - (1.4, 1.2, 1.6), c + (1.4, 1.2, 1.6)], -1)
        obb = (c + 0.05, sc.rot((0.2, 0.1, 1.0), 0.5), np.array([2.5, 2.9, 2.7])) if i == 1 else None
        out.append(sm.SubMap(model, pose.astype(np.float32), c2w, md, aabb, obb, c.astype(np.float32) + 0.1, None))
    return out


def compare_volumes(fused, ref, label):
    vol, tsdf = fused.volume.cpu().numpy(), fused.tsdf.cpu().numpy()
    assert vol.shape == ref["volume"].shape and all(np.array_equal(a, b) for a, b in zip(fused.ticks, ref["ticks"]))
    amb = ref["ambiguous"]
    # a voxel is seen only inside a box, so the -inf pattern is the whole -inf / -1 pattern: -1 stands where -inf does
    # (a blended value may itself be -1, so the values of tsdf cannot be asked where the voxel is unseen)
    pattern = np.isneginf(vol) != np.isneginf(ref["volume"])
    assert np.array_equal(tsdf, np.where(np.isneginf(vol), np.float32(-1), vol))
    assert np.array_equal(ref["tsdf"], np.where(np.isneginf(ref["volume"]), np.float32(-1), ref["volume"]))
    both = np.isfinite(vol) & np.isfinite(ref["volume"])
    err = np.abs(vol[both] - ref["volume"][both]).max() if both.any() else 0.0
    print(f"{label}: {vol.shape}, finite {int(both.sum())}, -inf {int(np.isneginf(vol).sum())}, max |diff| {err:.3e}, "
          f"pattern differences {int(pattern.sum())}, ambiguous {int(amb.sum())}")
    assert not np.isnan(vol).any() and not np.isnan(tsdf).any()
    assert amb.mean() <= sc.AMBIG_CAP and not (pattern & ~amb).any()
    assert both.sum() > 1000 and err <= 1e-5
    assert np.abs(tsdf[both] - ref["tsdf"][both]).max() <= 1e-5
    return vol, tsdf


def test_fused_volume_of_analytic_submaps_equals_the_restatement(dev):
    subs = analytic_submaps()
    fused = sm.fuse_volume(subs, CFG, K, device=dev, chunk=50000)          # several chunks per sub-box
    ref = sc.fuse_volume(subs, CFG, K, device=dev)
    vol, _ = compare_volumes(fused, ref, "analytic")
    pts = sc.grid_points(fused.ticks)
    uncovered = ~np.any([sc.in_aabb(pts, s.aabb) for s in subs], 0).reshape(vol.shape)
    assert uncovered.sum() > 1000 and np.isneginf(vol[uncovered]).all()   # a voxel no sub-map covers is -inf
    one_chunk = sm.fuse_volume(subs, CFG, K, device=dev)
    assert torch.equal(one_chunk.volume, fused.volume)                     # chunking changes nothing


def test_zero_weights_give_zero_and_a_single_submap_gives_its_own_sdf(dev):
    heavy = analytic_submaps([lambda w: torch.full_like(w[:, 0], 1e4)] * 3)[1:2]
    fused = sm.fuse_volume(heavy, CFG, K, device=dev)
    ref = sc.fuse_volume(heavy, CFG, K, device=dev)
    vol, tsdf = compare_volumes(fused, ref, "entropy 1e4")
    seen = np.isfinite(vol)
    assert seen.sum() > 1000 and (vol[seen] == 0).all() and not np.isnan(tsdf).any()

    single = analytic_submaps()[1:2]
    fused = sm.fuse_volume(single, CFG, K, device=dev)
    vol, _ = compare_volumes(fused, sc.fuse_volume(single, CFG, K, device=dev), "m = 1")
    pts = torch.from_numpy(sc.grid_points(fused.ticks).astype(np.float32).astype(np.float64)).to(dev)
    own = single[0].model.sdf(pts).to(torch.float32).cpu().numpy().reshape(vol.shape)
    seen = np.isfinite(vol)
    assert seen.sum() > 1000 and np.abs(vol[seen] - own[seen]).max() <= 1e-5


def test_fused_volume_of_two_networks_equals_the_restatement(dev):
    cfg = synth.config_plumbing()
    cfg["mesh"] = {"voxel_final": 0.02}
    cfg["cam"].update(W=W, H=H)                          # the 32 x 32 frame of that configuration has no pixel 20 from its edges
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    lo, hi = np.array(cfg["mapping"]["bound"]).T
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    subs = []
    for i in range(2):
        torch.manual_seed(10 + i)
        model = JointEncoding(cfg, bb, nf).to(dev).eval()
        with torch.no_grad():
            model.embed_fn.params.copy_((torch.randn(model.embed_fn.params.shape) * 0.05).to(dev))
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = sc.rot((0.1, 1.0, 0.0), 0.2 * i), (0.1 * i, 0.0, 0.15 * i)
        centre = mid + (0.2 * i - 0.1) * half
        c2w, md = sc.ring_of_keyframes(centre, 9, 90 + i, radius=0.2)
        aabb = np.stack([centre - 0.45 * half, centre + 0.45 * half], -1)
        subs.append(sm.SubMap(model, pose.astype(np.float32), c2w, md * 2, aabb, None, centre.astype(np.float32), None))
    fused = sm.fuse_volume(subs, cfg, K, device=dev, chunk=1 << 16)
    ref = sc.fuse_volume(subs, cfg, K, device=dev)
    vol, _ = compare_volumes(fused, ref, "two networks")
    assert np.ptp(vol[np.isfinite(vol)]) > 1e-3                # the networks' output, not a constant


# ----------------------------------------------------------------------------------------------------------- 3. memory
MEM_CHUNK = 1 << 17                                     # points per chunk in the memory test
MEM_CHUNK_BYTES = MEM_CHUNK * 3 * 8                     # its coordinate buffer: float64 [chunk,3] = 3 MiB


def memory_submaps(m, k_total):
    """m sub-maps whose boxes tile the same 4 m cube along x (so the grid is the same for every m), k_total keyframes in all"""
    out = []
    edges = np.linspace(-2.0, 2.0, m + 1)
    for i in range(m):
        aabb = np.array([[edges[i] - (0.2 if i else 0.0), edges[i + 1] + (0.2 if i < m - 1 else 0.0)], [-2.0, 2.0], [-2.0, 2.0]])
        c = aabb.mean(1)
        c2w, md = sc.ring_of_keyframes(c, k_total // m, 30 + i)
        out.append(sm.SubMap(sc.Analytic(CFG, np.eye(4), sc.sphere((0.0, 0.0, 0.0), 1.5), sc.wavy_entropy(0.1, 0.05)), np.eye(4, dtype=np.float32),
                             c2w, md, aabb, None, c.astype(np.float32), None))
    return out


def test_memory_does_not_grow_with_submaps_or_keyframes(dev):
    peaks = {}
    for m, k in ((2, 10), (8, 200), (2, 10)):
        subs = memory_submaps(m, k)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fused = sm.fuse_volume(subs, CFG, K, voxel_size=0.025, device=dev, chunk=MEM_CHUNK)
        torch.cuda.synchronize()
        peaks[(m, k)] = torch.cuda.max_memory_allocated(dev) - base
        n = fused.volume.numel()
        assert all(np.prod(sm._Grid(fused.ticks, dev).index_box(s.aabb)[1]) > MEM_CHUNK for s in subs)
        del fused
    print(f"grid of {n} voxels: peak {peaks[(2, 10)]} B with 2 sub-maps / 10 keyframes, {peaks[(8, 200)]} B with 8 / 200; "
          f"one chunk buffer = {MEM_CHUNK_BYTES} B; an [n,8] fp32 matrix would be {n * 8 * 4} B")
    assert n > 3_000_000
    assert peaks[(8, 200)] - peaks[(2, 10)] < MEM_CHUNK_BYTES


# ------------------------------------------------------------------------------------------------------- 4. components
def patch(nx, ny, step, origin, v0):
    """a flat patch of nx x ny quads -> vertices, faces (2 nx ny triangles of area step^2 / 2)"""
    ix, iy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    verts = np.stack([ix.ravel() * step, iy.ravel() * step, np.zeros(ix.size)], -1) + origin
    q = (ix[:-1, :-1] * (ny + 1) + iy[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([q, q + ny + 1, q + 1], -1), np.stack([q + 1, q + ny + 1, q + ny + 2], -1)])
    return verts, faces + v0


def soup_of_blobs(seed, min_area):
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    v0 = 0
    for b in range(int(rng.integers(5, 12))):
        big = b % 2 == 0
        nx, ny = int(rng.integers(2, 30)), int(rng.integers(2, 30))
        area = min_area * (rng.uniform(2.0, 6.0) if big else rng.uniform(0.05, 0.5))      # a factor 2 away from the threshold
        v, f = patch(nx, ny, np.sqrt(area / (nx * ny)), np.array([0.0, 0.0, 10.0 * b]), v0)
        verts.append(v), faces.append(f)
        v0 += len(v)
    verts, faces = np.concatenate(verts), np.concatenate(faces)
    relabel = rng.permutation(len(verts))
    out_v = np.zeros_like(verts)
    out_v[relabel] = verts
    return out_v, relabel[faces][rng.permutation(len(faces))]


@pytest.mark.parametrize("seed", range(5))
def test_components_of_random_soups_equal_the_restatement(seed, dev):
    verts, faces = soup_of_blobs(seed, 0.5)
    keep, labels = sm.keep_large_components(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), 0.5)
    want_keep, want_labels = sc.keep_large_components(verts, faces, 0.5)
    assert np.array_equal(labels.cpu().numpy(), want_labels)               # both label by the smallest face: the same partition
    assert np.array_equal(keep.cpu().numpy(), want_keep) and 0 < want_keep.sum() < len(faces)
    assert np.array_equal(sm.face_pairs(torch.from_numpy(faces).to(dev)).cpu().numpy(), sc.face_pairs(faces))


def clean_up_case(kind, occupancy):
    """blobs 3 m apart along z in front of three cameras (one without depth); two sub-maps that leave a strip in x uncovered"""
    verts, faces = soup_of_blobs(7, 0.5)
    verts = verts * [1.0, 1.0, 0.3]
    c2w = np.stack([sc.look_at(e, t) for e, t in (((1.4, 1.3, -3.0), (1.4, 1.3, 10.0)), ((0.5, 1.0, -2.0), (2.0, 1.5, 10.0)),
                                                  ((1.4, 1.3, -3.0), (1.4, 1.3, 10.0)))]).astype(np.float32)
    md = np.array([9.0, 7.5, 0.0], np.float32)
    subs = []
    for x0, x1 in ((-0.2, 1.0), (1.8, 3.2)):
        aabb = np.array([[x0, x1], [-0.5, 3.5], [-1.0, 40.0]])
        obb = (aabb.mean(1), sc.rot((0.0, 0.0, 1.0), 0.1), aabb[:, 1] - aabb[:, 0]) if kind == "obb" else None
        cloud = verts[(verts[:, 0] >= x0) & (verts[:, 0] <= x1)]
        bounds = occupancy(cloud) if kind == "occupancy" else None
        subs.append(sm.SubMap(None, np.eye(4, dtype=np.float32), c2w, md, aabb, obb, aabb.mean(1).astype(np.float32), bounds))
    return verts, faces, subs, {"cam": {"W": W, "H": H}}


@pytest.mark.parametrize("kind", ["occupancy", "obb", "aabb"])
def test_clean_up_equals_the_restatement_for_every_bounding_geometry(kind, dev):
    verts, faces, subs, cfg = clean_up_case(kind, lambda cloud: sm.voxel_occupancy(torch.from_numpy(cloud).to(dev), 0.4))
    if kind == "occupancy":
        _, _, ref_subs, _ = clean_up_case(kind, lambda cloud: sc.voxel_occupancy(cloud, 0.4))
        for a, b in zip(subs, ref_subs):
            assert np.array_equal(a.bounds[0], b.bounds[0]) and np.array_equal(a.bounds[2].cpu().numpy(), b.bounds[2])
    v, f = sm.clean_up(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), subs, cfg, K, 0.5)
    rv, rf = sc.clean_up(verts, faces, subs, cfg, K, 0.5)
    print(f"{kind}: {len(faces)} faces in, {len(rf)} kept, {len(rv)} of {len(verts)} vertices")
    assert 0 < len(rf) < len(faces)
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf)


def test_a_long_chain_needs_and_gets_more_rounds(dev):
    rng = np.random.default_rng(3)
    verts, faces = patch(1, 30000, 0.01, np.zeros(3), 0)
    faces = faces[rng.permutation(len(faces))]
    stats = {}
    labels = sm.label_components(torch.from_numpy(faces).to(dev), max_rounds=1, stats=stats)
    print("chain of", len(faces), "faces:", stats)
    assert stats["calls"] >= 2 and stats["rounds"] > 1                     # the first call's single round was not enough
    assert (labels == 0).all() and np.array_equal(sc.component_labels(faces), np.zeros(len(faces), np.int64))


# ------------------------------------------------------------------------------------------------------- 5. end to end
WALL = 0.2                                              # the wall between the rooms, cut out of both
VOXEL = 0.06


def free_space():
    a, b, door = (np.array(synth.TWO_ROOMS[k], np.float64) for k in ("room_a", "room_b", "door"))
    a[2, 1] -= WALL / 2
    b[2, 0] += WALL / 2
    return [a, b, np.array([door[0], door[1], [a[2, 1] - 0.05, b[2, 0] + 0.05]])]


def scene_sdf(w):
    """positive in free space (the two rooms and the door between them), max-norm distance to its boundary, in metres"""
    d = None
    for box in free_space():
        bx = torch.tensor(box, dtype=w.dtype, device=w.device)
        inside = torch.minimum(w - bx[:, 0], bx[:, 1] - w).min(-1)[0]
        d = inside if d is None else torch.maximum(d, inside)
    return d


def two_room_submaps():
    cfg = synth.config_two_rooms()
    Hc, Wc, fx, fy, cx, cy = synth.intrinsics_after_crop(cfg)
    poses, frames, _ = synth.two_room_sequence(cfg)
    z_wall = synth.TWO_ROOMS["room_a"][2][1]
    kf = list(range(0, len(poses), 15))
    boxes = [np.array(synth.TWO_ROOMS["room_a"], np.float64), np.array(synth.TWO_ROOMS["room_b"], np.float64)]
    for box in boxes:                                    # the walls lie inside the boxes, not on their faces
        box[:, 0] -= 0.3
        box[:, 1] += 0.3
    boxes[0][2, 1] += 0.2                                # one sub-map per room, overlapping at the door
    boxes[1][2, 0] -= 0.2
    subs = []
    for room in range(2):
        ids = [k for k in kf if (float(poses[k][2, 3]) < z_wall) == (room == 0)]
        c2w = torch.stack([poses[k] for k in ids])
        md = torch.stack([frames[k]["depth"].max() for k in ids])
        bias = 0.01 * (1 - 2 * room)                     # the sub-maps disagree by a sixth of a voxel: the blend matters
        model = sc.Analytic(cfg, poses[ids[0]].numpy(), lambda w, bias=bias: torch.clamp((scene_sdf(w) + bias) / 0.3, -1, 1),
                         sc.wavy_entropy(0.1 + 0.05 * room, 0.05),
                         rgb=lambda w, room=room: 2.0 * torch.sin(4.0 * w + room))
        subs.append(sm.SubMap(model, poses[ids[0]], c2w, md, boxes[room], None, boxes[room].mean(1).astype(np.float32), None))
    return cfg, (fx, fy, cx, cy), subs


@pytest.fixture(scope="module")
def two_rooms():
    return two_room_submaps()


def test_two_room_scene_end_to_end(two_rooms, dev, tmp_path):
    cfg, Kc, subs = two_rooms
    seen_volume = []
    path = str(tmp_path / "scene.ply")
    got = sm.extract_scene_mesh(subs, cfg, Kc, voxel_size=VOXEL, device=dev, mesh_savepath=path, on_volume=seen_volume.append)
    fused = seen_volume[0]
    assert isinstance(got, mesh.Mesh) and got.vertices.dtype == np.float64 and got.faces.dtype == np.int64
    # face for face: the restated marching cubes on the DEVICE's volume, then the restated clean-up and colours
    v, f, c = sc.scene_mesh_from_volume(fused.volume.cpu().numpy(), fused.ticks, subs, cfg, Kc, device=dev)
    print(f"two rooms: grid {tuple(fused.volume.shape)}, {len(got.vertices)} vertices, {len(got.faces)} faces")
    assert len(f) > 5000 and got.faces.shape == f.shape and np.array_equal(got.faces, f)
    assert np.array_equal(got.vertices, v)
    assert np.abs(got.vertex_colors - c).max() <= 1 / 255 and got.vertex_colors.min() >= 0 and got.vertex_colors.max() <= 1
    assert np.ptp(got.vertex_colors) > 0.5

    # one surface within a voxel of the true one, in the overlap too
    d = scene_sdf(torch.from_numpy(got.vertices)).abs().numpy()
    z = got.vertices[:, 2]
    overlap = (z > subs[1].aabb[2, 0]) & (z < subs[0].aabb[2, 1])
    print(f"distance to the true surface: max {d.max():.4f} m ({d.max() / VOXEL:.2f} voxels), in the overlap {d[overlap].max():.4f} m "
          f"over {int(overlap.sum())} vertices")
    assert overlap.sum() > 200 and d.max() <= VOXEL
    # both sides of the wall between the rooms are there, and nothing inside it
    assert (np.abs(z - (2.75 - WALL / 2)) < VOXEL).sum() > 100 and (np.abs(z - (2.75 + WALL / 2)) < VOXEL).sum() > 100

    # no face where no keyframe looks
    c2w = torch.cat([s.kf_c2w for s in subs])
    md = torch.cat([s.kf_max_depth for s in subs])
    seen = sc.point_mask(got.vertices, c2w, md, Kc, cfg["cam"]["W"], cfg["cam"]["H"])
    assert seen[got.faces].any(-1).all()
    raw_v, raw_f = mesh.marching_cubes(fused.volume, 0.0, 3.0)
    raw_seen = sc.point_mask(sc.world_vertices(raw_v, fused.ticks), c2w, md, Kc, cfg["cam"]["W"], cfg["cam"]["H"])
    print(f"marched {len(raw_f)} faces, {int((~raw_seen[raw_f].any(-1)).sum())} of them with no seen vertex; kept {len(got.faces)}")

    lv, lf, lc = mesh.load_ply(path)
    assert np.array_equal(lv, got.vertices) and np.array_equal(lf, got.faces)
    assert np.array_equal(lc, mesh.colors_to_uint8(got.vertex_colors))


def test_what_no_keyframe_sees_is_not_meshed(two_rooms, dev):
    cfg, Kc, subs = two_rooms
    full = sm.extract_scene_mesh(subs, cfg, Kc, voxel_size=VOXEL, device=dev, render_color=False)
    blind_b = [subs[0], subs[1]._replace(kf_max_depth=torch.zeros_like(subs[1].kf_max_depth))]
    got = sm.extract_scene_mesh(blind_b, cfg, Kc, voxel_size=VOXEL, device=dev, render_color=False)
    assert got.vertex_colors is None and 1000 < len(got.faces) < len(full.faces)
    seen = sc.point_mask(got.vertices, subs[0].kf_c2w, subs[0].kf_max_depth, Kc, cfg["cam"]["W"], cfg["cam"]["H"])
    assert seen[got.faces].any(-1).all()                      # room A's keyframes are the only ones left
    blind = [s._replace(kf_max_depth=torch.zeros_like(s.kf_max_depth)) for s in subs]
    none = sm.extract_scene_mesh(blind, cfg, Kc, voxel_size=VOXEL, device=dev)
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.vertex_colors.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_calls_are_bit_identical(two_rooms, dev):
    cfg, Kc, subs = two_rooms
    a = sm.fuse_volume(subs, cfg, Kc, voxel_size=VOXEL, device=dev)
    b = sm.fuse_volume(subs, cfg, Kc, voxel_size=VOXEL, device=dev)
    assert torch.equal(a.volume.view(torch.int32), b.volume.view(torch.int32)) and torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32))
    m1 = sm.extract_scene_mesh(subs, cfg, Kc, voxel_size=VOXEL, device=dev)
    m2 = sm.extract_scene_mesh(subs, cfg, Kc, voxel_size=VOXEL, device=dev)
    assert np.array_equal(m1.vertices, m2.vertices) and np.array_equal(m1.faces, m2.faces)
    assert np.array_equal(m1.vertex_colors.view(np.int32), m2.vertex_colors.view(np.int32))
