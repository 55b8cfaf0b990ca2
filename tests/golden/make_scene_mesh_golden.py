#!/usr/bin/env python3
"""Records the scene-mesher fixture scene_mesh.npz from the upstream's own code.

usage: make_scene_mesh_golden.py /path/to/upstream/MIPSFusion

``vis/math_helper.py`` is imported as it is (it uses ``np.bool``, aliased in this process).  ``point_mask``,
``get_grid_uniform`` and ``get_face_mask`` are taken out of ``model/Mesher.py`` by name, ``project_to_pixel`` and
``convert_to_local_pts2`` out of ``helper_functions/geometry_helper.py`` (both modules import libraries that are not
installed), and called with a small stand-in for ``self``.  Only inputs and recorded results are written.

vis_*      points fp32 [n,3], c2w fp32 [k,4,4], max_depth fp32 [k] (one keyframe has depth 0), K (fx fy cx cy), WH -> vis_mask
w_*        pts fp32 [n,3], centroids fp32 [m,3], box / mask bool [n,m], entropy / sdf fp32 [n,m] -> w_dist_weight [n,m]
           (convert_dist_to_weight over the points of each box), w_weights [n,m] (compute_weights on the clipped entropy),
           w_blended [n] (Mesher.py:518-527: the weighted sum where some sub-map holds, -1 elsewhere)
grid_*     three boxes: grid_min / grid_max [3,3], grid_vs [3] -> grid<i>_x / _y / _z tick arrays
face_*     vert_mask bool [V], faces int64 [F,3] -> face_seen bool [F]
local_*    pts fp32 [n,3], pose fp32 [4,4] -> local_out fp32 [n,3] (convert_to_local_pts2)
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1000 * 1000


def functions_of(path, names, ns):
    """the named functions / methods of a module whose imports cannot be satisfied"""
    tree = ast.parse(open(path).read())
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
    for fn in found:
        fn.decorator_list = []
    exec(compile(ast.Module(body=found, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def look_at(eye, target):
    """camera-to-world with the camera looking along its -z axis (points in front have z < 0 in the camera frame)"""
    back = (eye - target) / np.linalg.norm(eye - target)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, eye
    return m


def main():
    upstream = sys.argv[1]
    if not hasattr(np, "bool"):
        np.bool = bool
    sys.path.insert(0, upstream)
    from vis import math_helper as mh
    ns = {"torch": torch, "np": np}
    project_to_pixel, convert_to_local_pts2 = functions_of(os.path.join(upstream, "helper_functions", "geometry_helper.py"),
                                                           ["project_to_pixel", "convert_to_local_pts2"], ns)
    ns["reduce_and"], ns["reduce_or"] = mh.reduce_and, mh.reduce_or
    point_mask, get_grid_uniform, get_face_mask = functions_of(os.path.join(upstream, "model", "Mesher.py"),
                                                               ["point_mask", "get_grid_uniform", "get_face_mask"], ns)
    rng = np.random.default_rng(20)
    out = {}

    # ---- visibility
    k, n, W, H = 12, 3000, 640, 480
    fx, fy, cx, cy = 320.0, 320.0, 319.5, 239.5
    c2w = np.stack([look_at(rng.uniform(-1, 1, 3) + [0, 0, 4.0 * (j % 3)], rng.uniform(-3, 3, 3) + [0, 0, 4.0 * (j % 3) + 3]) for j in range(k)])
    pts = np.concatenate([rng.uniform(-6, 6, (n - 600, 3)) + [0, 0, 5], rng.uniform(-60, 60, (600, 3))]).astype(np.float32)
    max_depth = rng.uniform(2.0, 7.0, k).astype(np.float32)
    max_depth[5] = 0.0
    rays = torch.zeros((k, 16, 7))
    rays[:, :, 6] = torch.from_numpy(max_depth)[:, None] * torch.linspace(0, 1, 16)[None]
    me = types.SimpleNamespace(device="cpu", config={"cam": {"W": W, "H": H}}, kfSet=types.SimpleNamespace(rays=rays),
                               K=torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]]))
    mask = point_mask(me, torch.from_numpy(pts), torch.arange(k), torch.from_numpy(c2w.astype(np.float32)))
    out.update(vis_points=pts, vis_c2w=c2w.astype(np.float32), vis_max_depth=max_depth, vis_K=np.array([fx, fy, cx, cy]),
               vis_WH=np.array([W, H]), vis_mask=mask.numpy())
    print("visibility:", int(mask.sum()), "of", n, "seen")

    # ---- weights and the blended SDF (Mesher.py:456-527 with the recorded matrices in place of the queries)
    n, m = 4000, 3
    pts = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    centroids = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    box = rng.random((n, m)) < 0.7
    box[:50] = False
    maskm = box & (rng.random((n, m)) < 0.8)
    entropy = np.zeros((n, m), np.float32)
    sdf = np.full((n, m), -1, np.float32)
    dist_weight = np.zeros((n, m), np.float32)
    for i in range(m):
        idx = np.where(box[:, i])[0]
        e = rng.uniform(-0.05, 0.6, len(idx))
        e[rng.random(len(idx)) < 0.02] = 20000.0
        e[rng.random(len(idx)) < 0.02] = 0.0
        np.put(entropy[:, i], idx, e.astype(np.float32))
        np.put(sdf[:, i], idx, rng.uniform(-1, 1, len(idx)).astype(np.float32))
        dist = mh.compute_dist_to_center(pts[box[:, i]], centroids[i])
        np.put(dist_weight[:, i], idx, mh.convert_dist_to_weight(dist))
    maskm[50:80] &= False                                      # rows in a box that nothing sees
    heavy = np.where(maskm.sum(-1) == 1)[0][:40]
    entropy[heavy] = 10000.0                                   # rows whose weights all underflow to 0
    final = mh.reduce_or(maskm)
    clipped = np.clip(entropy, 0, 10000.)
    weights = mh.compute_weights(clipped, dist_weight, maskm)
    weighted = np.sum(sdf * weights, axis=-1)
    blended = np.full((n,), -1, np.float32)
    np.put(blended, np.where(final)[0], weighted[np.where(final)[0]])
    out.update(w_pts=pts, w_centroids=centroids, w_box=box, w_mask=maskm, w_entropy=entropy, w_sdf=sdf, w_dist_weight=dist_weight,
               w_weights=weights, w_blended=blended)
    print("weights: dtype", weights.dtype, "rows without a weight", int((weights.sum(-1) == 0).sum()))

    # ---- grids of three ragged extents
    gmin = np.array([[-0.31, 0.8, -0.85], [0.013, -2.2, 1.07], [-5.0, -0.4, -0.33]])
    gmax = np.array([[2.65, 6.75, 6.75], [1.9, 0.71, 1.93], [-3.1, 0.52, 2.9]])
    gvs = np.array([0.06, 0.03, 0.047])
    for i in range(3):
        _, ticks = get_grid_uniform(None, gmin[i], gmax[i], voxel_size=gvs[i])
        out[f"grid{i}_x"], out[f"grid{i}_y"], out[f"grid{i}_z"] = ticks
        print("grid", i, [len(t) for t in ticks])
    out.update(grid_min=gmin, grid_max=gmax, grid_vs=gvs)

    # ---- face mask
    V, F = 500, 1500
    vert_mask = rng.random(V) < 0.35
    faces = rng.integers(0, V, (F, 3))
    out.update(face_vert_mask=vert_mask, face_faces=faces, face_seen=get_face_mask(None, vert_mask, faces))

    # ---- world -> local
    pose = look_at(np.array([0.4, 3.7, 1.1]), np.array([1.5, 3.2, 5.0])).astype(np.float32)
    lp = rng.uniform(-4, 8, (1000, 3)).astype(np.float32)
    out.update(local_pts=lp, local_pose=pose, local_out=convert_to_local_pts2(torch.from_numpy(lp), torch.from_numpy(pose)).numpy())

    path = os.path.join(HERE, "scene_mesh.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < LIMIT, os.path.getsize(path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
