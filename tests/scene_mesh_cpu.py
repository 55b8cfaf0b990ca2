"""numpy / CPU-torch restatement of the scene mesher (include/mipsf_fuse.h, mipsfusion_amd/scene_mesh.py) in the
shape the upstream has it (model/Mesher.py:405-669, vis/math_helper.py): [n, m] matrices over n points and m sub-maps, one
keyframe at a time over all points.  It is a checker, not the product; numpy and torch only.

Sub-maps are any objects with the attributes of ``mipsfusion_amd.scene_mesh.SubMap``.  Models are evaluated on ``device``
(the CPU by default; the GPU tests pass the device so that both sides see the same network output)."""
import numpy as np
import torch

from . import mcubes_cpu as mc

F32 = np.float32
AMBIG_PX = 1e-2          # fp32 evaluation of |u| <~ 1e3 px is good to about 1e-3 px; ten times that
AMBIG_M = 1e-5
AMBIG_CAP = 0.005


def intrinsics(K):
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.ndim == 2 else tuple(K)


# ------------------------------------------------------------------------------------------------------------ grid
def get_grid_uniform(xyz_min, xyz_max, padding=0.05, voxel_size=0.05):
    """Mesher.py:43-54: floor division, linspace; -> the three tick arrays (float64)"""
    ticks = []
    for d in range(3):
        res = ((xyz_max[d] + padding) - (xyz_min[d] - padding)) // voxel_size
        ticks.append(np.linspace(xyz_min[d] - padding, xyz_max[d] + padding, int(res)))
    return ticks


def grid_points(ticks):
    """[X*Y*Z, 3] float64 in [X,Y,Z] order, z fastest"""
    return np.stack(np.meshgrid(*ticks, indexing="ij"), -1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------ visibility
def w2c_of(kf_c2w):
    return torch.inverse(torch.as_tensor(np.asarray(kf_c2w.detach().cpu() if torch.is_tensor(kf_c2w) else kf_c2w)).to(torch.float32))


def point_mask(points, kf_c2w, kf_max_depth, K, W, H, edge=20):
    """Mesher.py:247-281 with the upstream's torch expressions, one keyframe at a time (the upstream holds all k at once)"""
    pts = torch.as_tensor(np.asarray(points)).to(torch.float32)
    fx, fy, cx, cy = intrinsics(K)
    Kt = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], dtype=torch.float32)
    w2c = w2c_of(kf_c2w)
    md = torch.as_tensor(np.asarray(kf_max_depth, np.float32))
    seen = torch.zeros(pts.shape[0], dtype=torch.bool)
    for j in range(w2c.shape[0]):
        cam = torch.sum(pts[:, None, :] * w2c[j, None, :3, :3], -1) + w2c[j, None, :3, 3]
        z = cam[:, 2].clone()
        p = cam.clone().unsqueeze(-1)
        p[:, 0] *= -1
        uv = (Kt @ p).squeeze(-1)
        uv = (uv[:, :2] / (uv[:, -1:] + 1e-5)).float()
        m1 = (uv[:, 0] < W - edge) * (uv[:, 0] > edge) * (uv[:, 1] < H - edge) * (uv[:, 1] > edge)
        m1 = m1 & (z < 0)
        az = torch.abs(z)
        seen = torch.logical_or(seen, m1 & ((az > 0) * (az < md[j])))
    return seen.numpy()


def ambiguous_points(points, kf_c2w, kf_max_depth, K, W, H, edge=20):
    """float64: a point is ambiguous when no keyframe sees it with every test passed by more than the margin, and some
    keyframe sees it with the tests relaxed by the margin.  (A subset of 'some u, v or z within the margin of a threshold':
    a near-threshold value that cannot change the answer does not excuse a point.)"""
    pts = np.asarray(points, F32).astype(np.float64)
    fx, fy, cx, cy = intrinsics(K)
    w2c = w2c_of(kf_c2w).numpy().astype(np.float64)
    md = np.asarray(kf_max_depth, F32).astype(np.float64)
    sure = np.zeros(len(pts), bool)
    maybe = np.zeros(len(pts), bool)
    for j in range(w2c.shape[0]):
        cam = pts @ w2c[j, :3, :3].T + w2c[j, :3, 3]
        z = cam[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (fx * -cam[:, 0] + cx * z) / (z + 1e-5)
            v = (fy * cam[:, 1] + cy * z) / (z + 1e-5)

        def tests(mp, mz):
            return ((u < W - edge - mp) & (u > edge + mp) & (v < H - edge - mp) & (v > edge + mp) & (z < -mz)
                    & (np.abs(z) > mz) & (np.abs(z) < md[j] - mz))
        sure |= tests(AMBIG_PX, AMBIG_M)
        maybe |= tests(-AMBIG_PX, -AMBIG_M)
    return maybe & ~sure


# --------------------------------------------------------------------------------------------------------- weights
def pdf_gauss(x, mu=0., sigma=1.):
    k1 = 1 / (sigma * np.sqrt(2 * np.pi))
    m1 = (x - mu) / sigma
    return k1 * np.exp(-0.5 * m1 ** 2)


def dist_weight(pts32, centroid):
    """compute_dist_to_center + convert_dist_to_weight (math_helper.py:58-72) -> weights fp32, max_dist"""
    dist = np.linalg.norm(pts32 - np.asarray(centroid, F32)[None], axis=-1)
    max_dist = np.max(np.absolute(dist))
    return pdf_gauss(np.absolute(dist), 0., max_dist / 3.).astype(F32), max_dist


def compute_weights(entropy, dist_w, mask):
    """math_helper.py:79-96: [n,m] weights, rows normalised to 1 where some sub-map holds and the sum is positive"""
    m = mask.astype(F32)
    raw = (np.exp(-10. * entropy) * m) * (dist_w * m)
    norms = np.sum(raw, axis=-1, keepdims=True)
    ok = (np.sum(m, -1, keepdims=True) > 0) & (norms > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, raw / norms, np.zeros_like(raw))


def blend(values, entropy, dist_w, mask):
    """Mesher.py:522-526: clip, weights, weighted sum over the sub-maps"""
    w = compute_weights(np.clip(entropy, 0, 10000.), dist_w, mask)
    return np.sum(values * w, axis=-1), w


# ----------------------------------------------------------------------------------------------------------- boxes
def in_aabb(p64, aabb):
    aabb = np.asarray(aabb, np.float64)
    return np.all((p64 >= aabb[:, 0]) & (p64 <= aabb[:, 1]), -1)


def in_obb(p64, obb):
    """|(p - centre) . axis_i| <= extent_i / 2, axis i = column i of R (float64, products summed left to right)"""
    c, R, ext = (np.asarray(t, np.float64) for t in obb)
    d = p64 - c
    ok = np.ones(len(p64), bool)
    for i in range(3):
        s = (d[:, 0] * R[0, i] + d[:, 1] * R[1, i]) + d[:, 2] * R[2, i]
        ok &= np.abs(s) <= ext[i] / 2
    return ok


def voxel_occupancy(points, vox_size=0.5, expand_scale=1.2, shrink_scale=0.8):
    """Mesher.py:80-95 with open3d's voxel grid restated (UNPINNED): the points, and the points scaled about their mean,
    on a grid with origin = min - vox/2 and index = floor((p - origin) / vox) -> (origin [3], vox, occupied bool [a,b,c])"""
    p = np.asarray(points, np.float64)
    centre = p.mean(0)
    allp = np.concatenate([p] + [centre + s * (p - centre) for s in (expand_scale, shrink_scale) if s is not None], 0)
    origin = allp.min(0) - vox_size / 2
    idx = np.floor((allp - origin) / vox_size).astype(np.int64)
    occ = np.zeros(tuple(idx.max(0) + 1), bool)
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    return origin, float(vox_size), occ


def in_occupancy(p64, bounds):
    origin, vox, occ = bounds
    origin, occ = np.asarray(origin, np.float64), np.asarray(occ.cpu() if torch.is_tensor(occ) else occ)
    idx = np.floor((p64 - origin) / vox).astype(np.int64)
    ok = np.all((idx >= 0) & (idx < np.array(occ.shape)), -1)
    out = np.zeros(len(p64), bool)
    out[ok] = occ[idx[ok, 0], idx[ok, 1], idx[ok, 2]]
    return out


def in_bounding_geometry(p64, sm):
    if sm.bounds is not None:
        return in_occupancy(p64, sm.bounds)
    return in_obb(p64, sm.obb) if sm.obb is not None else in_aabb(p64, sm.aabb)


# ---------------------------------------------------------------------------------------------------------- fusion
def normalise_cfg(config):
    """-> sub, div (float64 [3]): (local - sub) / div, Mesher.py:480-484"""
    if config["grid"].get("use_bound_normalize", True):
        bb = np.array(config["mapping"]["bound"], np.float64)
        return bb[:, 0], bb[:, 1] - bb[:, 0]
    L = np.array(config["mapping"]["localMLP_max_len"], np.float64)
    return -L, 2 * L


def local_normalised(pts32, first_kf_c2w, config):
    """Mesher.py:476-484: fp32 world -> fp32 local (convert_to_local_pts2), then the float64 normalisation"""
    w2l = w2c_of(first_kf_c2w)
    p = torch.from_numpy(np.ascontiguousarray(pts32, F32))
    local = torch.sum(p[:, None, :] * w2l[None, :3, :3], -1) + w2l[None, :3, 3]
    out = local.to(torch.float64)
    if config["grid"]["tcnn_encoding"]:
        sub, div = normalise_cfg(config)
        out = (out - torch.from_numpy(sub)) / torch.from_numpy(div)
    return out


def query(fn, pts_norm, device, batch=1024 * 64):
    with torch.no_grad():
        outs = [fn(pts_norm[i:i + batch].to(device)).detach().cpu() for i in range(0, pts_norm.shape[0], batch)]
    return torch.cat(outs, 0).to(torch.float32).numpy() if outs else np.zeros((0, 10), F32)


def submap_masks(p64, sm, K, W, H, edge=20):
    """-> box bool [n] (the axis-aligned box), mask bool [n] (oriented box & seen by the sub-map's keyframes), ambiguous"""
    box = in_aabb(p64, sm.aabb)
    mask = np.zeros(len(p64), bool)
    amb = np.zeros(len(p64), bool)
    idx = np.where(box)[0]
    p32 = p64[idx].astype(F32)
    inside = in_obb(p32.astype(np.float64), sm.obb) if sm.obb is not None else np.ones(len(idx), bool)
    mask[idx] = inside & point_mask(p32, sm.kf_c2w, sm.kf_max_depth, K, W, H, edge)
    amb[idx] = inside & ambiguous_points(p32, sm.kf_c2w, sm.kf_max_depth, K, W, H, edge)
    return box, mask, amb


def fuse_volume(submaps, config, K, voxel_size=None, padding=0.05, device="cpu"):
    """Mesher.py:447-534 -> dict(ticks, volume [X,Y,Z] with -inf where marching is masked out, tsdf [X,Y,Z] with -1 where
    nothing is seen, ambiguous [X,Y,Z])"""
    voxel_size = config["mesh"]["voxel_final"] if voxel_size is None else voxel_size
    W, H = config["cam"]["W"], config["cam"]["H"]
    aabbs = np.stack([np.asarray(sm.aabb, np.float64) for sm in submaps])
    ticks = get_grid_uniform(aabbs[:, :, 0].min(0), aabbs[:, :, 1].max(0), padding, voxel_size)
    pts = grid_points(ticks)
    n, m = len(pts), len(submaps)
    g_box, g_mask, g_amb = (np.zeros((n, m), bool) for _ in range(3))
    g_ent, g_dw = np.zeros((n, m), F32), np.zeros((n, m), F32)
    g_sdf = np.full((n, m), -1, F32)
    for i, sm in enumerate(submaps):
        g_box[:, i], g_mask[:, i], g_amb[:, i] = submap_masks(pts, sm, K, W, H)
        idx = np.where(g_box[:, i])[0]
        p32 = pts[idx].astype(F32)
        raw = query(sm.model.query_sdf_entropy_prob, local_normalised(p32, sm.first_kf_c2w, config), device)
        g_sdf[idx, i], g_ent[idx, i] = raw[:, 0], raw[:, 1]
        g_dw[idx, i] = dist_weight(p32, sm.centroid)[0]
    final = g_mask.any(-1)
    weighted, _ = blend(g_sdf, g_ent, g_dw, g_mask)
    tsdf = np.where(final, weighted, F32(-1)).astype(F32)
    volume = np.where(g_box.any(-1) & final, tsdf, F32(-np.inf)).astype(F32)
    shape = tuple(len(t) for t in ticks)
    return {"ticks": ticks, "volume": volume.reshape(shape), "tsdf": tsdf.reshape(shape), "ambiguous": g_amb.any(-1).reshape(shape)}


def blend_colors(vertices, submaps, config, K, device="cpu"):
    """Mesher.py:591-663 -> rgb fp32 [V,3]"""
    W, H = config["cam"]["W"], config["cam"]["H"]
    V, m = len(vertices), len(submaps)
    mask = np.zeros((V, m), bool)
    ent, dw = np.zeros((V, m), F32), np.zeros((V, m), F32)
    rgb = np.zeros((V, m, 3), F32)
    for i, sm in enumerate(submaps):
        box, mask[:, i], _ = submap_masks(vertices, sm, K, W, H)
        idx = np.where(box)[0]
        if not len(idx):
            continue
        p32 = vertices[idx].astype(F32)
        raw = query(sm.model.query_color_sdf, local_normalised(p32, sm.first_kf_c2w, config), device)
        rgb[idx, i] = 1 / (1 + np.exp(-raw[:, :3]))
        ent[idx, i] = raw[:, 4]
        dw[idx, i] = dist_weight(p32, sm.centroid)[0]
    w = compute_weights(np.clip(ent, 0, 10000.), dw, mask)
    return np.sum(rgb * w[:, :, None], axis=1).astype(F32)


# -------------------------------------------------------------------------------------------------------- clean-up
def face_mask(vert_mask, faces):
    """Mesher.py:223-231, the loose form: a face goes only if all three of its vertices are unset"""
    return ~np.all(~np.asarray(vert_mask, bool)[faces], -1)


def face_pairs(faces):
    """pairs of faces that share an edge (an edge of more than two faces chains them) -> int64 [E,2]"""
    F = len(faces)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)
    key = np.sort(e, 1)
    owner = np.tile(np.arange(F), 3)
    order = np.lexsort((owner, key[:, 1], key[:, 0]))
    key, owner = key[order], owner[order]
    same = np.all(key[1:] == key[:-1], -1)
    return np.stack([owner[:-1][same], owner[1:][same]], -1)


def component_labels(faces):
    """label = the smallest face of the edge-connected component (UNPINNED restatement of trimesh's split)"""
    F = len(faces)
    lab = np.arange(F)
    pairs = face_pairs(faces) if F else np.zeros((0, 2), np.int64)
    while len(pairs):
        m = np.minimum(lab[pairs[:, 0]], lab[pairs[:, 1]])
        new = lab.copy()
        np.minimum.at(new, pairs[:, 0], m)
        np.minimum.at(new, pairs[:, 1], m)
        while not np.array_equal(new[new], new):
            new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def face_areas(vertices, faces):
    t = np.asarray(vertices, np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=-1)


def keep_large_components(vertices, faces, min_area):
    """-> keep bool [F], labels"""
    lab = component_labels(faces)
    area = np.zeros(len(faces))
    np.add.at(area, lab, face_areas(vertices, faces))
    return area[lab] > min_area, lab


def compact(vertices, faces, *per_vertex):
    used = np.zeros(len(vertices), bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return (vertices[used], new_id[faces]) + tuple(p[used] for p in per_vertex)


def clean_up(vertices, faces, submaps, config, K, min_component_area=0.5):
    """Mesher.py:547-577: unseen faces, small components, faces outside every bounding geometry; unreferenced vertices go"""
    W, H = config["cam"]["W"], config["cam"]["H"]
    c2w = np.concatenate([np.asarray(sm.kf_c2w.cpu() if torch.is_tensor(sm.kf_c2w) else sm.kf_c2w) for sm in submaps], 0)
    md = np.concatenate([np.asarray(sm.kf_max_depth.cpu() if torch.is_tensor(sm.kf_max_depth) else sm.kf_max_depth) for sm in submaps], 0)
    seen = point_mask(vertices, c2w, md, K, W, H)
    faces = faces[face_mask(seen, faces)]
    faces = faces[keep_large_components(vertices, faces, min_component_area)[0]]
    inside = np.zeros(len(vertices), bool)
    for sm in submaps:
        inside |= in_bounding_geometry(vertices, sm)
    faces = faces[face_mask(inside, faces)]
    return compact(vertices, faces)


def world_vertices(v_voxel, ticks):
    """Mesher.py:537-543: spacing = second tick gap, origin = first tick"""
    spacing = np.array([t[2] - t[1] for t in ticks])
    return v_voxel * spacing[None] + np.array([t[0] for t in ticks])[None]


def scene_mesh_from_volume(volume, ticks, submaps, config, K, min_component_area=0.5, truncation=3.0, render_color=True,
                           device="cpu"):
    v, f = mc.marching_cubes(np.ascontiguousarray(volume, F32), 0.0, truncation)
    v = world_vertices(v, ticks)
    v, f = clean_up(v, f, submaps, config, K, min_component_area)
    return v, f, (blend_colors(v, submaps, config, K, device) if render_color else None)


# ------------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
CAMERA = {"K": (320.0, 320.0, 319.5, 239.5), "W": 640, "H": 480}
# (seed, points, keyframes): ragged sizes from one point to above 2^20, one keyframe to 300
VIS_CASES = [(0, 1, 1), (1, 63, 3), (2, 64, 12), (3, 65, 1), (4, 1000, 300), (5, 4097, 37), (6, 70001, 16), (7, (1 << 20) + 77, 5),
             (8, 250000, 64), (9, 12345, 100), (10, 5000, 300), (11, 333, 2)]


def look_at(eye, target):
    """camera-to-world, the camera looking along its -z axis (a point in front of it has z < 0 in the camera frame)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    back = (eye - target) / np.linalg.norm(eye - target)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(back, right), back, eye
    return m


def visibility_case(seed, n, k):
    """-> points fp32 [n,3] (inside, behind and far outside the frusta), c2w fp32 [k,4,4], max_depth fp32 [k] (one is 0)"""
    rng = np.random.default_rng(1000 + seed)
    c2w = np.stack([look_at(rng.uniform(-1, 1, 3) + [0, 0, 4.0 * (j % 3)], rng.uniform(-3, 3, 3) + [0, 0, 4.0 * (j % 3) + 3])
                    for j in range(k)]).astype(F32)
    far = rng.random(n) < 0.2
    pts = np.where(far[:, None], rng.uniform(-60, 60, (n, 3)), rng.uniform(-6, 6, (n, 3)) + [0, 0, 5]).astype(F32)
    md = rng.uniform(2.0, 7.0, k).astype(F32)
    if k > 1:
        md[k // 2] = 0.0
    return pts, c2w, md


# ---------------------------------------------------------------- analytic sub-maps and keyframes for the tests and the benchmark
class Analytic:
    """a sub-map given by functions of the WORLD position: undoes the normalisation and the local frame in float64"""

    def __init__(self, config, first_kf_c2w, sdf, entropy, rgb=None):
        self.sub, self.div = (torch.from_numpy(t) for t in normalise_cfg(config))
        self.pose = torch.as_tensor(np.asarray(first_kf_c2w), dtype=torch.float64)
        self.sdf, self.entropy, self.rgb = sdf, entropy, rgb

    def world(self, p):
        local = p.to(torch.float64) * self.div.to(p.device) + self.sub.to(p.device)
        pose = self.pose.to(p.device)
        return local @ pose[:3, :3].T + pose[:3, 3]

    def query_color_sdf(self, p):
        w = self.world(p)
        out = torch.zeros((p.shape[0], 10), dtype=torch.float64, device=p.device)
        if self.rgb is not None:
            out[:, :3] = self.rgb(w)
        out[:, 3], out[:, 4] = self.sdf(w), self.entropy(w)
        return out

    def query_sdf_entropy_prob(self, p):
        return self.query_color_sdf(p)[..., 3:]


def sphere(centre, radius):
    return lambda w: torch.clamp((torch.linalg.norm(w - torch.tensor(centre, dtype=w.dtype, device=w.device), dim=-1) - radius) / 0.5, -1, 1)


def wavy_entropy(a, b):
    return lambda w: a + b * torch.sin(3.0 * w[:, 0]) * torch.cos(2.0 * w[:, 2])


def ring_of_keyframes(centre, n, seed, radius=0.6):
    rng = np.random.default_rng(seed)
    c2w = np.stack([look_at(np.asarray(centre) + rng.uniform(-radius, radius, 3), np.asarray(centre) + 3.0 * np.array(
        [np.cos(2 * np.pi * j / n), 0.3 * np.sin(5.0 * j), np.sin(2 * np.pi * j / n)])) for j in range(n)]).astype(np.float32)
    return c2w, rng.uniform(2.0, 4.0, n).astype(np.float32)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
