"""CPU: the restatement of the scene mesher (tests/scene_mesh_cpu.py) against what the upstream's own code gave
(tests/golden/scene_mesh.npz, recorded by tests/golden/make_scene_mesh_golden.py), and the ambiguity cap of the GPU test on the
reference's own result."""
import types

import numpy as np
import pytest

from . import scene_mesh_cpu as sc
from .conftest import load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("scene_mesh.npz")


def test_point_mask_equals_the_recorded_mask(g):
    W, H = (int(t) for t in g["vis_WH"])
    mask = sc.point_mask(g["vis_points"], g["vis_c2w"], g["vis_max_depth"], g["vis_K"], W, H)
    assert mask.dtype == bool and np.array_equal(mask, g["vis_mask"])
    assert 0.1 < mask.mean() < 0.9
    zero = int(np.where(g["vis_max_depth"] == 0)[0][0])
    alone = sc.point_mask(g["vis_points"], g["vis_c2w"][zero:zero + 1], g["vis_max_depth"][zero:zero + 1], g["vis_K"], W, H)
    assert not alone.any()                                     # a keyframe without depth sees nothing


def test_weights_and_blended_sdf_match_the_recorded_ones(g):
    n, m = g["w_box"].shape
    dw = np.zeros((n, m), np.float32)
    for i in range(m):
        idx = np.where(g["w_box"][:, i])[0]
        dw[idx, i] = sc.dist_weight(g["w_pts"][idx], g["w_centroids"][i])[0]
    assert np.abs(dw - g["w_dist_weight"]).max() <= 1e-6
    weighted, w = sc.blend(g["w_sdf"], g["w_entropy"], dw, g["w_mask"])
    assert np.abs(w - g["w_weights"]).max() <= 1e-6
    blended = np.where(g["w_mask"].any(-1), weighted, np.float32(-1))
    assert np.isfinite(blended).all() and np.abs(blended - g["w_blended"]).max() <= 1e-6
    dead = g["w_mask"].any(-1) & (g["w_weights"].sum(-1) == 0)
    assert dead.sum() >= 20 and (blended[dead] == 0).all()    # seen, every weight underflowed: 0, not NaN


def test_grid_ticks_equal_the_recorded_ones(g):
    for i in range(3):
        ticks = sc.get_grid_uniform(g["grid_min"][i], g["grid_max"][i], voxel_size=g["grid_vs"][i])
        for t, name in zip(ticks, "xyz"):
            assert np.array_equal(t, g[f"grid{i}_{name}"])


def test_face_mask_and_local_points_equal_the_recorded_ones(g):
    assert np.array_equal(sc.face_mask(g["face_vert_mask"], g["face_faces"]), g["face_seen"])
    cfg = {"grid": {"tcnn_encoding": False}}
    local = sc.local_normalised(g["local_pts"], g["local_pose"], cfg).numpy()
    assert np.array_equal(local.astype(np.float32), g["local_out"]) and local.dtype == np.float64


@pytest.mark.parametrize("seed,n,k", sc.VIS_CASES)
def test_ambiguous_share_of_the_gpu_cases_stays_under_the_cap(seed, n, k):
    """the GPU test excuses ambiguous points; on its own inputs they are few, so the cap cannot hide a failure"""
    pts, c2w, md = sc.visibility_case(seed, n, k)
    amb = sc.ambiguous_points(pts, c2w, md, sc.CAMERA["K"], sc.CAMERA["W"], sc.CAMERA["H"])
    assert amb.sum() <= sc.AMBIG_CAP * n, (int(amb.sum()), n)


def test_ambiguity_is_where_the_reference_could_flip(g):
    """outside the ambiguous set the recorded mask is what a float64 evaluation gives"""
    W, H = (int(t) for t in g["vis_WH"])
    amb = sc.ambiguous_points(g["vis_points"], g["vis_c2w"], g["vis_max_depth"], g["vis_K"], W, H)
    assert amb.mean() <= sc.AMBIG_CAP
    pts = g["vis_points"].astype(np.float64)
    fx, fy, cx, cy = g["vis_K"]
    w2c = sc.w2c_of(g["vis_c2w"]).numpy().astype(np.float64)
    seen = np.zeros(len(pts), bool)
    for j in range(len(w2c)):
        c = pts @ w2c[j, :3, :3].T + w2c[j, :3, 3]
        u, v = (fx * -c[:, 0] + cx * c[:, 2]) / (c[:, 2] + 1e-5), (fy * c[:, 1] + cy * c[:, 2]) / (c[:, 2] + 1e-5)
        seen |= (u < W - 20) & (u > 20) & (v < H - 20) & (v > 20) & (c[:, 2] < 0) & (np.abs(c[:, 2]) < g["vis_max_depth"][j])
    assert np.array_equal(seen[~amb], g["vis_mask"][~amb])


def test_components_and_clean_up_pieces():
    # two strips that share only a vertex are two components; a strip is one
    faces = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 5, 6], [5, 6, 7]])
    assert sc.component_labels(faces).tolist() == [0, 0, 0, 3, 3]
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0], [0.2, 2, 0], [0, 2.2, 0], [0.2, 2.2, 0]], np.float64)
    keep, _ = sc.keep_large_components(verts, faces, 1.2)
    assert keep.tolist() == [True, True, True, False, False]
    origin, vox, occ = sc.voxel_occupancy(np.array([[0.0, 0, 0], [1.0, 1, 1]]), 0.5, None, None)
    assert np.allclose(origin, -0.25) and occ.shape == (3, 3, 3) and occ.sum() == 2
    inside = sc.in_occupancy(np.array([[0.2, 0.2, 0.2], [0.6, 0.6, 0.6], [1.2, 1.0, 0.9], [-3.0, 0, 0]]), (origin, vox, occ))
    assert inside.tolist() == [True, False, True, False]
    sm = types.SimpleNamespace(bounds=None, obb=(np.zeros(3), np.eye(3), np.array([2.0, 2, 2])), aabb=None)
    assert sc.in_bounding_geometry(np.array([[0.9, -0.9, 0], [1.1, 0, 0]]), sm).tolist() == [True, False]


def test_submap_from_mesh_fills_centroid_and_box():
    from mipsfusion_amd import scene_mesh as sm
    v = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 4, 0], [0.0, 0, 6]])
    s = sm.submap_from_mesh("model", types.SimpleNamespace(vertices=v), np.eye(4), np.eye(4)[None], np.ones(1))
    assert s.model == "model" and s.obb is None and s.bounds is None
    assert s.centroid.dtype == np.float32 and np.allclose(s.centroid, [0.5, 1.0, 1.5])
    assert np.allclose(s.aabb, np.stack([v.mean(0) + 1.1 * (v.min(0) - v.mean(0)), v.mean(0) + 1.1 * (v.max(0) - v.mean(0))], -1))
    ticks = sm.get_grid_uniform(s.aabb[:, 0], s.aabb[:, 1], 0.05, 0.1)
    assert all(np.array_equal(a, b) for a, b in zip(ticks, sc.get_grid_uniform(s.aabb[:, 0], s.aabb[:, 1], 0.05, 0.1)))
