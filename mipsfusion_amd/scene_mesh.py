"""The scene as one mesh: the reference's ``Mesher.extract_mesh_jointly`` (model/Mesher.py:405-669) on the device.

One dense grid is laid over the union of the sub-maps' boxes.  Every sub-map's SDF and entropy are queried at the grid points of
its box and blended per voxel with the weights ``exp(-10 entropy) * gauss(distance to the sub-map's centroid)``, restricted to
sub-maps whose keyframes saw the point; the blended volume is marched, faces that no keyframe saw, small components and what
lies outside every sub-map's bounding geometry are dropped, and the vertex colours are blended with the same weights.
Kernels: ``csrc/fuse.hip`` behind ``include/mipsf_fuse.h``; marching cubes: ``mesh.marching_cubes``.  DESIGN.md 4.13.

Deliberate differences from the reference:

* The reference marches the primal grid with scikit-image (Lewiner) under a mask and cleans up with trimesh and open3d.  Here the
  fused volume is marched by this library's one extractor, the dual-grid one of DESIGN.md 4.12, with the masked voxels at
  ``-inf``.  Vertices are not comparable with the reference's one by one, and the third-party steps are restated, not pinned:
  components are edge-connected sets of faces, the occupancy set of ``voxel_occupancy`` has origin = min - vox/2 and index =
  floor((p - origin) / vox).
* open3d's minimal oriented box is not reproduced: ``SubMap.obb`` is an input and ``submap_from_mesh`` leaves it at the AABB.
* The reference normalises the weights over the sub-maps and then sums; here ``num / den`` is formed once per voxel, which
  differs by rounding only.

Memory: two fp32 words and one flag byte of state per voxel plus the fp32 volume, and chunk buffers of ``CHUNK`` points;
nothing grows with the number of sub-maps or keyframes.  CPU tensors raise, as everywhere in the product path.
"""
import ctypes as C
import math
from typing import Any, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, mesh
from .inference import query_in_batches

CHUNK = 1 << 20                 # grid points per query chunk: [CHUNK,3] float64 coordinates + the model's [CHUNK,7] output
QUERY_BATCH = 1024 * 64


class SubMap(NamedTuple):
    """what the reference pulls out of kfSet / slam for one sub-map"""
    model: Any                              # JointEncoding, or any object with query_sdf_entropy_prob / query_color_sdf
    first_kf_c2w: Any                       # [4,4] world pose of the sub-map's first keyframe
    kf_c2w: Any                             # [k,4,4] world poses of its keyframes
    kf_max_depth: Any                       # [k] largest stored depth of each keyframe
    aabb: Any                               # [3,2] (the reference: AABB of the 1.1-scaled sub-mesh)
    obb: Optional[Tuple[Any, Any, Any]]     # (centre [3], R [3,3] with the axes as columns, extent [3]) or None = the AABB
    centroid: Any                           # [3]
    bounds: Optional[Tuple[Any, float, Any]] = None    # voxel_occupancy(...) for the final filter; None = obb


class FusedVolume(NamedTuple):
    volume: torch.Tensor                    # fp32 [X,Y,Z]: the blended SDF, -inf where marching is switched off
    ticks: Tuple[np.ndarray, np.ndarray, np.ndarray]       # float64 tick arrays
    tsdf: torch.Tensor                      # fp32 [X,Y,Z]: the blended SDF, -1 where no sub-map saw the voxel


def _np64(t) -> np.ndarray:
    return np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64)


def _intrinsics(K):
    K = _np64(K)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.ndim == 2 else tuple(K)


def _w2c(c2w) -> torch.Tensor:
    """fp32 inverse on the host, as ``kf_pose_c2w.inverse()`` of the reference (a few small matrices)"""
    c2w = c2w.detach().cpu() if torch.is_tensor(c2w) else torch.as_tensor(np.asarray(c2w))
    return torch.inverse(c2w.to(torch.float32))


def keyframe_table(kf_c2w, kf_max_depth, device):
    """-> (fp32 [max(k,1),16] records of include/mipsf_fuse.h: world->camera 3x4, max depth; k)"""
    w2c = _w2c(kf_c2w).reshape(-1, 4, 4)
    k = w2c.shape[0]
    md = kf_max_depth.detach().cpu() if torch.is_tensor(kf_max_depth) else torch.as_tensor(np.asarray(kf_max_depth))
    tab = torch.zeros((max(k, 1), _lib.FUSE_KF_FLOATS), dtype=torch.float32)
    tab[:k, :12] = w2c[:, :3, :].reshape(k, 12)
    tab[:k, 12] = md.to(torch.float32).reshape(k)
    return tab.to(device), k


def keyframe_max_depth(rays: torch.Tensor, kf_ids) -> torch.Tensor:
    """the largest stored depth of each keyframe (``DeviceRayDB.rays[j, :, 6]``, Mesher.py:263,273), taken on the device"""
    return rays[torch.as_tensor(kf_ids, dtype=torch.int64, device=rays.device), :, 6].amax(1)


def _camera(table, k, K, W, H, edge):
    fx, fy, cx, cy = _intrinsics(K)
    cam = _lib.FuseCamera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, cam.edge = fx, fy, cx, cy, W, H, edge
    cam.k, cam.keyframes = k, _lib.dptr(table)
    return cam


class _Grid:
    """three float64 tick arrays on the device and an index sub-box: the grid description of include/mipsf_fuse.h"""

    def __init__(self, ticks, device):
        self.ticks = tuple(np.ascontiguousarray(t, np.float64) for t in ticks)
        self.dev = tuple(torch.from_numpy(t).to(device) for t in self.ticks)
        self.dims = tuple(len(t) for t in self.ticks)
        if min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] >= 1 << 31:
            raise RuntimeError(f"a grid of {self.dims} points is empty or has 2^31 points or more")

    def index_box(self, aabb):
        """ticks with lo <= t <= hi per axis (an AABB on a linspace grid is an index box) -> lo [3], size [3]"""
        aabb = _np64(aabb)
        lo = [int(np.searchsorted(t, aabb[d, 0], "left")) for d, t in enumerate(self.ticks)]
        hi = [int(np.searchsorted(t, aabb[d, 1], "right")) for d, t in enumerate(self.ticks)]
        return lo, [max(0, h - l) for l, h in zip(lo, hi)]

    def points(self, lo=None, size=None, first=0, n=None):
        lo = (0, 0, 0) if lo is None else lo
        size = self.dims if size is None else size
        p = _lib.FusePoints()
        p.points = None
        for d in range(3):
            p.ticks[d], p.dims[d], p.lo[d], p.size[d] = _lib.dptr(self.dev[d], torch.float64), self.dims[d], lo[d], size[d]
        p.first, p.n = first, size[0] * size[1] * size[2] - first if n is None else n
        return p


def _list_points(pts: torch.Tensor, first=0, n=None):
    p = _lib.FusePoints()
    p.points = _lib.dptr(pts)
    p.first, p.n = first, pts.shape[0] - first if n is None else n
    return p


def _visibility(pts_desc, n, cam, device) -> torch.Tensor:
    seen = torch.empty(n, dtype=torch.uint8, device=device)
    a = _lib.FuseVisibilityArgs.new(pts=pts_desc, cam=cam, seen=_lib.dptr(seen, torch.uint8))
    _lib.check(_lib.lib().mipsf_fuse_visibility(C.byref(a), _lib.stream_ptr()), "fuse_visibility")
    return seen


def _device_points(points) -> torch.Tensor:
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError("scene_mesh runs on the GPU only (no CPU fallback): pass a tensor on the device")
    return points.to(torch.float32).contiguous()


@torch.no_grad()
def point_mask(points: torch.Tensor, kf_c2w, kf_max_depth, K, W, H, edge=20) -> torch.Tensor:
    """Mesher.py:247-281: whether each point [n,3] (narrowed to fp32 as there) is seen by at least one keyframe -> bool [n]"""
    pts = _device_points(points)
    with torch.cuda.device(pts.device):
        table, k = keyframe_table(kf_c2w, kf_max_depth, pts.device)
        return _visibility(_list_points(pts), pts.shape[0], _camera(table, k, K, W, H, edge), pts.device).bool()


@torch.no_grad()
def grid_point_mask(ticks, kf_c2w, kf_max_depth, K, W, H, edge=20, lo=None, size=None, device="cuda") -> torch.Tensor:
    """``point_mask`` over the index sub-box (lo, size) of the grid the ticks span, without storing its points -> bool [size]"""
    device = torch.device(device)
    with torch.cuda.device(device):
        grid = _Grid(ticks, device)
        desc = grid.points(lo, size)
        table, k = keyframe_table(kf_c2w, kf_max_depth, device)
        seen = _visibility(desc, desc.n, _camera(table, k, K, W, H, edge), device)
        return seen.bool().reshape(tuple(desc.size))


# ------------------------------------------------------------------------------------------------------------ fusion
def get_grid_uniform(xyz_min, xyz_max, padding=0.05, voxel_size=0.05):
    """Mesher.py:43-54 (floor division, ``linspace``) -> the three float64 tick arrays"""
    out = []
    for d in range(3):
        res = ((xyz_max[d] + padding) - (xyz_min[d] - padding)) // voxel_size
        out.append(np.linspace(xyz_min[d] - padding, xyz_max[d] + padding, int(res)))
    return tuple(out)


def _normalisation(config):
    """(local - sub) / div in float64 (Mesher.py:480-484); identity without ``tcnn_encoding``"""
    if not config["grid"]["tcnn_encoding"]:
        return np.zeros(3), np.ones(3)
    if config["grid"].get("use_bound_normalize", True):
        bb = np.array(config["mapping"]["bound"], np.float64)
        return bb[:, 0], bb[:, 1] - bb[:, 0]
    L = np.array(config["mapping"]["localMLP_max_len"], np.float64)
    return -L, 2 * L


def _local_points(desc, first_kf_c2w, config, device) -> torch.Tensor:
    out = torch.empty((desc.n, 3), dtype=torch.float64, device=device)
    a = _lib.FuseLocalArgs.new(pts=desc, out=_lib.dptr(out, torch.float64))
    a.w2l[:] = _w2c(first_kf_c2w)[:3, :].reshape(12).tolist()
    sub, div = _normalisation(config)
    a.sub[:], a.div[:] = sub.tolist(), div.tolist()
    _lib.check(_lib.lib().mipsf_fuse_local_points(C.byref(a), _lib.stream_ptr()), "fuse_local_points")
    return out


def _gauss(max_dist: float):
    """sigma = max_dist / 3 and 1 / (sigma sqrt(2 pi)) (math_helper.py:47-72)"""
    sigma = float(max_dist) / 3.0
    if not sigma > 0:
        raise RuntimeError("a sub-map whose points all coincide with its centroid has no distance weight")
    return sigma, 1.0 / (sigma * math.sqrt(2 * math.pi))


def _accumulate(desc, cam, sm: SubMap, raw, value_col, entropy_col, channels, sigmoid, max_dist, num, den, flags, rows=None):
    a = _lib.FuseAccumulateArgs.new(pts=desc, cam=cam, rows=_lib.dptr(rows, torch.int32), n_rows=den.shape[0], channels=channels,
                                    sigmoid=sigmoid, value_stride=raw.shape[1], entropy_stride=raw.shape[1],
                                    num=_lib.dptr(num), den=_lib.dptr(den), flags=_lib.dptr(flags, torch.uint8))
    base = _lib.dptr(raw)
    a.values, a.entropy = base + 4 * value_col, base + 4 * entropy_col
    if sm.obb is not None:
        centre, R, extent = (_np64(t) for t in sm.obb)
        a.use_obb = 1
        a.obb_centre[:], a.obb_axes[:], a.obb_half[:] = centre.tolist(), R.reshape(9).tolist(), (extent / 2).tolist()
    a.centroid[:] = np.asarray(_np64(sm.centroid), np.float32).tolist()
    a.sigma, a.gauss_k = _gauss(max_dist)
    _lib.check(_lib.lib().mipsf_fuse_accumulate(C.byref(a), _lib.stream_ptr()), "fuse_accumulate")


def _finalize(num, den, flags, out, volume, channels):
    a = _lib.FuseFinalizeArgs.new(n=den.shape[0], channels=channels, num=_lib.dptr(num), den=_lib.dptr(den),
                                  flags=_lib.dptr(flags, torch.uint8), out=_lib.dptr(out), volume=_lib.dptr(volume))
    _lib.check(_lib.lib().mipsf_fuse_finalize(C.byref(a), _lib.stream_ptr()), "fuse_finalize")


def _query(fn, pts, rank, world) -> torch.Tensor:
    raw = query_in_batches(fn, pts, QUERY_BATCH, rank, world)
    if not raw.is_cuda:
        raise RuntimeError("scene_mesh runs on the GPU only (no CPU fallback): the model returned a CPU tensor")
    return raw.to(torch.float32).contiguous()


def _box_max_dist(grid: _Grid, lo, size, centroid) -> float:
    """the largest fp32 distance from the centroid over the sub-box: it is reached at the corner that is farthest on every
    axis, because the fp32 norm is monotone in each |difference| (``np.max`` over the sub-map's valid points in the reference)"""
    c = np.asarray(_np64(centroid), np.float32)
    far = np.zeros(3, np.float32)
    for d in range(3):
        ends = grid.ticks[d][[lo[d], lo[d] + size[d] - 1]].astype(np.float32)
        far[d] = np.abs(ends - c[d]).max()
    return float(np.linalg.norm(far))


def _device_of(submaps, device):
    if device is not None:
        return torch.device(device)
    for sm in submaps:
        params = getattr(sm.model, "parameters", None)
        p = next(params(), None) if params is not None else None
        if p is not None:
            return p.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def fuse_volume(submaps: Sequence[SubMap], config, K, voxel_size=None, padding=0.05, rank=0, world=1, device=None,
                chunk=CHUNK) -> FusedVolume:
    """Mesher.py:447-534 on the device: the grid over the union of the sub-maps' boxes and the blended SDF on it."""
    device = _device_of(submaps, device)
    if device.type != "cuda":
        raise RuntimeError("scene_mesh runs on the GPU only (no CPU fallback)")
    voxel_size = config["mesh"]["voxel_final"] if voxel_size is None else voxel_size
    W, H = config["cam"]["W"], config["cam"]["H"]
    aabbs = np.stack([_np64(sm.aabb) for sm in submaps])
    with torch.cuda.device(device):
        grid = _Grid(get_grid_uniform(aabbs[:, :, 0].min(0), aabbs[:, :, 1].max(0), padding, voxel_size), device)
        N = grid.dims[0] * grid.dims[1] * grid.dims[2]
        num = torch.zeros(N, dtype=torch.float32, device=device)
        den = torch.zeros(N, dtype=torch.float32, device=device)
        flags = torch.zeros(N, dtype=torch.uint8, device=device)
        for sm in submaps:
            lo, size = grid.index_box(sm.aabb)
            n_box = size[0] * size[1] * size[2]
            if n_box == 0:
                continue
            table, k = keyframe_table(sm.kf_c2w, sm.kf_max_depth, device)
            cam = _camera(table, k, K, W, H, 20)
            max_dist = _box_max_dist(grid, lo, size, sm.centroid)
            for first in range(0, n_box, chunk):
                desc = grid.points(lo, size, first, min(chunk, n_box - first))
                raw = _query(sm.model.query_sdf_entropy_prob, _local_points(desc, sm.first_kf_c2w, config, device), rank, world)
                _accumulate(desc, cam, sm, raw, 0, 1, 1, 0, max_dist, num, den, flags)
                del raw
        tsdf = torch.empty(N, dtype=torch.float32, device=device)
        volume = torch.empty(N, dtype=torch.float32, device=device)
        _finalize(num, den, flags, tsdf, volume, 1)
    return FusedVolume(volume.reshape(grid.dims), grid.ticks, tsdf.reshape(grid.dims))


@torch.no_grad()
def blend_colors(vertices: torch.Tensor, submaps: Sequence[SubMap], config, K, rank=0, world=1) -> torch.Tensor:
    """Mesher.py:591-663: per-vertex colour (float64 [V,3] world vertices on the device) -> fp32 [V,3] in 0..1"""
    device = vertices.device
    V = vertices.shape[0]
    W, H = config["cam"]["W"], config["cam"]["H"]
    with torch.cuda.device(device):
        num = torch.zeros((V, 3), dtype=torch.float32, device=device)
        den = torch.zeros(V, dtype=torch.float32, device=device)
        out = torch.empty((V, 3), dtype=torch.float32, device=device)
        for sm in submaps:
            aabb = torch.from_numpy(_np64(sm.aabb)).to(device)
            rows = torch.nonzero(((vertices >= aabb[:, 0]) & (vertices <= aabb[:, 1])).all(-1))[:, 0]
            if rows.numel() == 0:
                continue
            pts = vertices[rows].to(torch.float32).contiguous()
            centroid = torch.from_numpy(np.asarray(_np64(sm.centroid), np.float32)).to(device)
            d = pts - centroid
            max_dist = float(torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
            if not max_dist > 0:
                continue
            table, k = keyframe_table(sm.kf_c2w, sm.kf_max_depth, device)
            desc = _list_points(pts)
            raw = _query(sm.model.query_color_sdf, _local_points(desc, sm.first_kf_c2w, config, device), rank, world)
            _accumulate(desc, _camera(table, k, K, W, H, 20), sm, raw, 0, 4, 3, 1, max_dist, num, den, None,
                        rows.to(torch.int32).contiguous())
        if V:
            _finalize(num, den, None, out, None, 3)
    return out


# ---------------------------------------------------------------------------------------------------------- clean-up
def face_pairs(faces: torch.Tensor) -> torch.Tensor:
    """pairs of faces that share an edge (an edge of more than two faces chains them) -> int32 [E,2]; index plumbing in torch"""
    F = faces.shape[0]
    f = faces.to(torch.int64)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    V = int(f.max()) + 1 if F else 1
    key = e.min(1)[0] * V + e.max(1)[0]
    owner = torch.arange(F, device=faces.device).repeat(3)
    key, order = torch.sort(key * F + owner)                     # by edge, then by face: the result does not depend on a tie rule
    owner = owner[order]
    same = (key[1:] // F) == (key[:-1] // F)
    return torch.stack([owner[:-1][same], owner[1:][same]], -1).to(torch.int32).contiguous()


@torch.no_grad()
def label_components(faces: torch.Tensor, max_rounds: int = 4, stats: Optional[dict] = None) -> torch.Tensor:
    """label of every face = the smallest face of its edge-connected component -> int32 [F] (mipsf_fuse_label_components);
    ``stats`` receives the number of calls and of rounds in which a label moved"""
    F = faces.shape[0]
    dev = faces.device
    with torch.cuda.device(dev):
        labels = torch.empty(F, dtype=torch.int32, device=dev)
        if F == 0:
            return labels
        if F * (int(faces.max()) + 1) ** 2 >= 1 << 62:
            raise RuntimeError("label_components: too many faces and vertices for the 64-bit edge keys")
        pairs = face_pairs(faces)
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        moved_before, resume = 0, 0
        while True:
            a = _lib.FuseLabelArgs.new(F=F, E=pairs.shape[0], pairs=_lib.dptr(pairs, torch.int32), labels=_lib.dptr(labels, torch.int32),
                                       counts=_lib.dptr(counts, torch.int32), max_rounds=max_rounds, resume=resume)
            _lib.check(_lib.lib().mipsf_fuse_label_components(C.byref(a), _lib.stream_ptr()), "fuse_label_components")
            moved = int(counts[1])
            if stats is not None:
                stats["calls"], stats["rounds"] = stats.get("calls", 0) + 1, moved
            if moved - moved_before < max_rounds:
                return labels
            moved_before, resume = moved, 1                     # every round moved a label: go on from where it stands
            max_rounds = min(64, 2 * max_rounds)


def face_areas(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    t = vertices.to(torch.float64)[faces.to(torch.int64)]
    return 0.5 * torch.linalg.norm(torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), dim=-1)


def keep_large_components(vertices, faces, min_component_area):
    """-> keep bool [F]: faces of components whose area (float64, summed in face order) exceeds the threshold; labels"""
    labels = label_components(faces).to(torch.int64)
    F = faces.shape[0]
    if F == 0:
        return torch.zeros(0, dtype=torch.bool, device=faces.device), labels
    lab_sorted, order = torch.sort(labels, stable=True)
    cs = torch.cumsum(face_areas(vertices, faces)[order], 0)
    last = torch.ones(F, dtype=torch.bool, device=faces.device)
    last[:-1] = lab_sorted[1:] != lab_sorted[:-1]
    ends = torch.nonzero(last)[:, 0]
    total = cs[ends]
    total[1:] = total[1:] - cs[ends[:-1]]
    area = torch.zeros(F, dtype=torch.float64, device=faces.device)
    area[lab_sorted[ends]] = total
    return area[labels] > min_component_area, labels


def voxel_occupancy(points, vox_size=0.5, expand_scale=1.2, shrink_scale=0.8):
    """Mesher.py:80-95 with open3d's voxel grid restated (unpinned): the points together with the points scaled about their
    mean, on a grid with origin = min - vox/2 and index = floor((p - origin) / vox) -> (origin float64 [3], vox, occupied bool
    [a,b,c]); points on the device give an occupancy on the device."""
    p = _np64(points)                       # a set-up step on a point cloud: numpy on the host, whatever device the points are on
    centre = p.mean(0)
    allp = np.concatenate([p] + [centre + s * (p - centre) for s in (expand_scale, shrink_scale) if s is not None], 0)
    origin = allp.min(0) - vox_size / 2
    idx = np.floor((allp - origin) / vox_size).astype(np.int64)
    occ = np.zeros(tuple(idx.max(0) + 1), bool)
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    occ = torch.from_numpy(occ)
    return origin, float(vox_size), occ.to(points.device) if torch.is_tensor(points) else occ


def _inside_bounding_geometry(vertices: torch.Tensor, sm: SubMap) -> torch.Tensor:
    dev = vertices.device
    if sm.bounds is not None:
        origin, vox, occ = sm.bounds
        occ = torch.as_tensor(occ).to(dev)
        idx = torch.floor((vertices - torch.from_numpy(_np64(origin)).to(dev)) / vox).to(torch.int64)
        ok = ((idx >= 0) & (idx < torch.tensor(occ.shape, device=dev))).all(-1)
        idx = idx.clamp(min=0)
        idx = torch.minimum(idx, torch.tensor(occ.shape, device=dev) - 1)
        return ok & occ[idx[:, 0], idx[:, 1], idx[:, 2]]
    if sm.obb is not None:
        centre, R, extent = (torch.from_numpy(_np64(t)).to(dev) for t in sm.obb)
        d = vertices - centre
        ok = torch.ones(vertices.shape[0], dtype=torch.bool, device=dev)
        for i in range(3):
            ok &= ((d[:, 0] * R[0, i] + d[:, 1] * R[1, i]) + d[:, 2] * R[2, i]).abs() <= extent[i] / 2
        return ok
    aabb = torch.from_numpy(_np64(sm.aabb)).to(dev)
    return ((vertices >= aabb[:, 0]) & (vertices <= aabb[:, 1])).all(-1)


def _loose(vert_mask: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """get_face_mask (Mesher.py:223-231), the loose form: a face goes only if all three of its vertices are unset"""
    return vert_mask[faces].any(-1)


@torch.no_grad()
def clean_up(vertices: torch.Tensor, faces: torch.Tensor, submaps: Sequence[SubMap], config, K, min_component_area=0.5):
    """Mesher.py:547-577 on the device: world vertices float64 [V,3], faces int64 [F,3] -> the same, cleaned and compacted"""
    W, H = config["cam"]["W"], config["cam"]["H"]
    dev = vertices.device
    c2w = torch.cat([torch.as_tensor(sm.kf_c2w).detach().cpu().reshape(-1, 4, 4) for sm in submaps], 0)
    md = torch.cat([torch.as_tensor(sm.kf_max_depth).detach().cpu().reshape(-1) for sm in submaps], 0)
    seen = point_mask(vertices, c2w, md, K, W, H) if vertices.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
    faces = faces[_loose(seen, faces)]
    faces = faces[keep_large_components(vertices, faces, min_component_area)[0]]
    inside = torch.zeros(vertices.shape[0], dtype=torch.bool, device=dev)
    for sm in submaps:
        inside |= _inside_bounding_geometry(vertices, sm)
    faces = faces[_loose(inside, faces)]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    new_id = torch.cumsum(used, 0) - 1
    return vertices[used], new_id[faces]


# ------------------------------------------------------------------------------------------------------- the interface
@torch.no_grad()
def extract_scene_mesh(submaps: Sequence[SubMap], config, K, voxel_size=None, render_color=True, min_component_area=0.5,
                       truncation=3.0, mesh_savepath="", rank=0, world=1, padding=0.05, device=None, on_volume=None) -> mesh.Mesh:
    """``Mesher.extract_mesh_jointly``: one mesh of the whole scene.  ``rank, world`` shard the model queries as ``extract_mesh``
    does (every rank extracts the same mesh; rank 0 writes the file); ``on_volume(FusedVolume)`` sees the volume before it is
    marched."""
    fused = fuse_volume(submaps, config, K, voxel_size, padding, rank, world, device)
    if on_volume is not None:
        on_volume(fused)
    v, f = mesh.marching_cubes(fused.volume, 0.0, truncation, return_device=True)
    dev = v.device
    # Mesher.py:537-543: spacing = the second tick gap, origin = the first tick
    spacing = torch.tensor([t[2] - t[1] for t in fused.ticks], dtype=torch.float64, device=dev)
    origin = torch.tensor([t[0] for t in fused.ticks], dtype=torch.float64, device=dev)
    v = v * spacing + origin
    v, f = clean_up(v, f, submaps, config, K, min_component_area)
    color = blend_colors(v, submaps, config, K, rank, world).cpu().numpy() if render_color else None
    out = mesh.Mesh(v.cpu().numpy(), f.cpu().numpy(), color)
    if mesh_savepath and rank == 0:
        mesh.save_ply(mesh_savepath, out.vertices, out.faces, out.vertex_colors)
    return out


def submap_from_mesh(model, sub_mesh, first_kf_c2w, kf_c2w, kf_max_depth, scale=1.1) -> SubMap:
    """Mesher.py:429-445: centroid = the mean of the sub-mesh's vertices (fp32), aabb = the box of the vertices scaled by
    ``scale`` about it; ``obb`` stays None (open3d's minimal oriented box is not reproduced)."""
    v = _np64(sub_mesh.vertices if hasattr(sub_mesh, "vertices") else sub_mesh)
    centre = v.mean(0)
    scaled = centre + scale * (v - centre)
    return SubMap(model, first_kf_c2w, kf_c2w, kf_max_depth, np.stack([scaled.min(0), scaled.max(0)], -1), None,
                  centre.astype(np.float32), None)
