"""The float64 restatement of the mesh renderer (tests/raster_cpu.py) against what is known without it: the ground-truth meshes of
mipsfusion_amd/synth.py are the exact surfaces of its two analytic renderers, so their rendered depth has a closed-form answer.
tests/test_gpu_raster.py then holds the device to the restatement, word for word."""
import math
import os

import numpy as np
import pytest

from mipsfusion_amd import _lib, synth

from . import eval_cpu as E
from . import raster_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size", sorted(R.SIZES))
def test_box_room_equals_the_analytic_depth(size):
    """Both sides compute the exit depth of the box to about 1e-15; the bound 2^-23 allows one fp32 rounding of it (2^-24) twice
    over.  tt itself is held to 1e-14 relative.  The fp32 words are NOT held to the analytic value rounded to fp32: the view that
    faces a wall head-on has a constant depth that lies, in float64, half way between two fp32 values, and the last float64 bit
    decides which one it becomes (179 pixels of that view at 33x47; every other pixel of the ten views has the same word)."""
    H, W, K = R.SIZES[size]
    v, f, lo, hi = R.box_room()
    poses = R.box_poses()
    depth, face, tt = R.render_depth(v.astype(np.float32), f, poses, K, H, W, return_tt=True)
    assert depth.dtype == np.float32 and face.dtype == np.int32 and depth.shape == (len(R.BOX_VIEWS), H, W)
    assert np.all(face >= 0) and np.all(depth > 0)                                       # no pixel misses
    want = np.stack([R.box_exit_depth(lo, hi, p.numpy(), K, H, W) for p in poses])
    rel_tt = np.abs(tt - want) / want
    rel = np.abs(depth.astype(np.float64) - want) / want
    print(f"{size}: tt rel max {rel_tt.max():.3e}; fp32 depth rel max {rel.max():.3e} (2^-24 = {2.0 ** -24:.3e}); "
          f"words equal to fp32(analytic): {np.mean(depth == want.astype(np.float32)):.6f}")
    assert rel_tt.max() <= 1e-14
    assert rel.max() <= 2.0 ** -23


def test_two_rooms_equal_the_fp32_renderer():
    """render_rooms_frame computes in fp32 (a handful of fp32 roundings: 1e-5 relative is a generous bound for them); its door
    test and the mesh's door are the same rectangle, so views through the door from both rooms and onto the coincident copies of
    the shared wall agree pixel by pixel."""
    H, W, K = R.SIZES["40x56"]
    v, f = synth.two_rooms_mesh()
    poses = R.rooms_poses()
    depth, face = R.render_depth(v.astype(np.float32), f, poses, K, H, W)
    assert np.all(face >= 0)
    T = synth.TWO_ROOMS
    worst = 0.0
    through = 0
    for k, pose in enumerate(poses):
        want = synth.render_rooms_frame(T["room_a"], T["room_b"], T["door"], pose, H, W, *K, drop=0.0)["depth"].numpy().astype(np.float64)
        rel = np.abs(depth[k].astype(np.float64) - want) / want
        worst = max(worst, float(rel.max()))
        z = pose[2, 3].item()
        zw = pose[:3, 3].numpy().astype(np.float64)[2] + depth[k].astype(np.float64) * np.stack(R.pixel_rays(pose.numpy().astype(np.float64), K, H, W), -1)[:, 2].reshape(H, W)
        through += int(np.count_nonzero((zw > 2.76) if z < 2.75 else (zw < 2.74)))
        assert rel.max() <= 1e-5, (k, float(rel.max()))
    print(f"two rooms: largest relative difference {worst:.3e}; {through} pixels end in the other room")
    assert through > 500                                                                  # the door views do look through the door


def test_marched_room_has_no_cracks():
    """4 936 welded faces; a pixel on an edge two faces share is hit by both (the edge rule is inclusive and the edge values negate
    exactly), so no ray escapes between them.  The L1 against the analytic depth is the bevel of the marched corners: printed, not
    gated."""
    H, W, K = R.SIZES["33x47"]
    v, f = R.marched_room()
    assert len(f) > 4000
    _, _, lo, hi = R.box_room()
    poses = R.box_poses(R.BOX_VIEWS[:3])
    depth, face = R.render_depth(v.astype(np.float32), f, poses, K, H, W)
    assert np.all(face >= 0) and np.all(depth > 0)
    for k, p in enumerate(poses):
        want = R.box_exit_depth(lo, hi, p.numpy(), K, H, W)
        print(f"marched view {k}: all-pixel L1 against the analytic depth {np.abs(depth[k] - want).mean() * 1e3:.2f} mm")


def test_split_square_ties_go_to_the_lower_face():
    v, f, poses, K, H, W = R.split_square()
    depth, face, tt = R.render_depth(v.astype(np.float32), f, poses, K, H, W, return_tt=True)
    assert np.all(depth == np.float32(1.0)) and np.all(tt == 1.0)                         # border pixels lie on the border and are hit
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    diagonal = i + j == 16
    assert diagonal.sum() == 17 and np.all(face[0][diagonal] == 0)
    assert np.array_equal(face[0], np.where(i + j >= 16, 0, 1))                           # x >= y is face 0, the edge included


def test_random_mesh_counts():
    """5 000 small faces (50 degenerate, 3 with bad indices, one giant) from 4 m away: the numbers found when the rule was fixed"""
    v, f = E.mesh_random()
    poses, K, H, W = R.random_view()
    depth, face = R.render_depth(v, f, poses, K, H, W)
    hit = face[0] >= 0
    assert np.array_equal(hit, depth[0] > 0)
    assert int(hit.sum()) == 328 and len(np.unique(face[0][hit])) == 23
    bad = np.any((f < 0) | (f >= len(v)), axis=1)
    assert not bad[face[0][hit]].any()
    nan_v = v.copy()
    nan_v[f[face[0][hit][0]][1]] = np.nan                                                  # a vertex that is not finite: that face hits nothing
    _, face2 = R.render_depth(nan_v, f, poses, K, H, W)
    assert not np.any(face2 == face[0][hit][0]) and np.any(face2 >= 0)


def test_near_and_far_cut_the_room():
    H, W, K = R.SIZES["33x47"]
    v, f, _, _ = R.box_room()
    poses = R.box_poses(R.BOX_VIEWS[:1])
    full = R.render_depth(v.astype(np.float32), f, poses, K, H, W)[0]
    near, far = float(np.quantile(full, 0.3)), float(np.quantile(full, 0.7))
    cut = R.render_depth(v.astype(np.float32), f, poses, K, H, W, near=near, far=far)[0]
    keep = (full > near) & (full < far)
    assert 0 < keep.sum() < keep.size
    assert np.array_equal(cut, np.where(keep, full, np.float32(0)))                       # the room is convex: one face per ray


def test_l1_of_a_mesh_against_itself():
    H, W, K = R.SIZES["33x47"]
    v, f, _, _ = R.box_room()
    poses = R.box_poses(R.BOX_VIEWS[:2])
    m = R.depth_l1((v, f), (v, f), poses, K, H, W)
    assert m["l1"] == 0.0 and m["l1_both"] == 0.0 and m["both"] == 1.0 and m["neither"] == 0.0 and m["pixels"] == H * W
    depth = R.render_depth(v.astype(np.float32), f, poses, K, H, W)[0]
    holes = depth.copy()
    holes[:, :5] = 0
    rec = R.l1_records(holes, depth)[0]
    assert (rec["both"], rec["rec_only"], rec["gt_only"], rec["neither"]) == (H * W - 5 * W, 0, 5 * W, 0)
    assert rec["sum_both"] == 0.0 and abs(rec["sum_all"] - math.fsum(depth[0, :5].astype(np.float64).ravel())) <= 1e-12


def test_visibility_in_front_of_and_behind_a_wall():
    """a point 1 cm in front of the wall the camera faces is seen; 2 eps behind the wall it is not; with no depth (D = 0) it is
    again, as it is when the view's max_depth alone decides"""
    H, W, K = R.SIZES["40x56"]
    v, f, lo, hi = R.box_room()
    poses = R.box_poses(((0.0, 0.0),))                                                    # looks along -z at the wall z = lo[2]
    t = poses[0][:3, 3].numpy().astype(np.float64)
    depth = R.render_depth(v.astype(np.float32), f, poses, K, H, W)[0]
    eps = 0.02
    front = np.array([[t[0] + 0.1, t[1] - 0.2, lo[2] + 0.01]], np.float32)
    behind = front - np.array([[0.0, 0.0, 0.01 + 2 * eps]], np.float32)
    md = np.array([100.0], np.float32)
    assert R.visible(front, depth, poses, md, K, 0, eps).all()
    assert not R.visible(behind, depth, poses, md, K, 0, eps).any()
    assert R.visible(behind, np.zeros_like(depth), poses, md, K, 0, eps).all()
    assert not R.visible(front, depth, poses, np.array([1.0], np.float32), K, 0, eps).any()      # farther than max_depth
    assert not R.visible(front, depth, poses, md, K, 30, eps).any()                              # an edge that leaves no image
    back = np.array([[t[0], t[1], t[2] + 1.0]], np.float32)                                     # behind the camera
    assert not R.visible(back, depth, poses, md, K, 0, eps).any()


def test_the_library_exports_the_renderer():
    lib = _lib.lib()
    for name in _lib.RASTER_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.mipsf_raster_workspace_bytes(_lib.RASTER_WS_DEPTH, 1, 12, 40, 56) >= 8 * (40 * 56 + 12)
    for bad in ((0, 12, 40, 56), (1, 0, 40, 56), (1, 12, 0, 56), (1, 12, 40, _lib.RASTER_MAX_SIDE + 1), (1, _lib.RASTER_MAX_FACES + 1, 8, 8),
                (2, 1 << 30, 8, 8), (17, 12, 8192, 8192)):
        assert lib.mipsf_raster_workspace_bytes(_lib.RASTER_WS_DEPTH, *bad) == 0, bad
    import mipsfusion_amd
    assert callable(mipsfusion_amd.render_mesh_depth) and callable(mipsfusion_amd.depth_l1)


@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    """tools/raster_host.hip: raster.hip's screen box and pixel test compiled for the host, driven by the kernels' loops"""
    import shutil
    import subprocess
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("raster_host")
    exe = str(d / "raster_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "raster_host.hip"), "-o", exe], check=True)

    def run(v32, faces, poses, K, H, W, near, far):
        import struct
        import subprocess
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 4, 4)
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("5I", len(v32), len(faces), len(p), H, W) + struct.pack("6d", *K, near, far))
            f.write(np.ascontiguousarray(v32, np.float32).tobytes() + np.ascontiguousarray(faces).astype(np.int32).tobytes() + p.tobytes())
        out = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], check=True, capture_output=True, text=True).stdout
        keys = np.fromfile(d / "out.bin", np.uint64).reshape(len(p), H, W)
        hit = keys != R.KEY_EMPTY
        depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
        return depth, np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32), out.strip()
    return run


@pytest.mark.parametrize("name", R.DEPTH_CASES)
def test_the_screen_boxes_leave_out_no_pixel(host_build, name):
    """The device tests only the pixels of each face's screen box; the restatement tests all.  The function that finds the box and
    the one that tests a pixel compile for the host too, so that what the box leaves out shows here, without a GPU: the images
    must be EQUAL on every case the GPU test renders."""
    c = R.depth_case(name)
    depth, face, said = host_build(c["vertices"], c["faces"], c["poses"].numpy(), c["K"], c["H"], c["W"], c["near"], c["far"])
    print(name, said)
    assert np.array_equal(face, c["face"]) and np.array_equal(depth.view(np.uint32), c["depth"].view(np.uint32))


def test_the_screen_boxes_of_triangles_around_the_camera(host_build):
    """1 500 random triangles of four sizes around four random poses each: most cross the camera plane or lie behind it"""
    g = np.random.default_rng(7)
    H, W, K = R.SIZES["33x47"]
    for size, spread in ((1.0, 2.0), (0.2, 1.0), (3.0, 1.0), (0.05, 0.3)):
        v = (g.uniform(-spread, spread, (1500, 1, 3)) + g.uniform(-size, size, (1500, 3, 3))).reshape(-1, 3).astype(np.float32)
        f = np.arange(4500).reshape(-1, 3)
        poses = np.stack([R.pose_of(tuple(g.uniform(-0.3, 0.3, 3)), float(g.uniform(0, 6.28)), float(g.uniform(-1.5, 1.5))).numpy() for _ in range(4)])
        want_d, want_f = R.render_depth(v, f, poses, K, H, W)
        depth, face, said = host_build(v, f, poses, K, H, W, 0.0, math.inf)
        print(size, spread, said, [int((x >= 0).sum()) for x in want_f])
        assert np.array_equal(face, want_f) and np.array_equal(depth.view(np.uint32), want_d.view(np.uint32))
