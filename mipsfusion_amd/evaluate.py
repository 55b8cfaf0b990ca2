"""How good a mesh is: accuracy, completion and completion ratio against a ground-truth mesh, the way the NICE-SLAM / Co-SLAM
evaluation computes them (sample each surface uniformly by area, take every sample's distance to the nearest sample of the other
surface, form means and the share below a threshold).  Upstream has no evaluation code.  Every step is a HIP kernel of
``csrc/eval.hip`` (C ABI: include/mipsf_eval.h) on top of the grid of ``csrc/icp.hip``:

    sample_surface          area-uniform, stratified, reproducible samples of a triangle mesh
    nearest_distance        the exact nearest neighbour of every source point, with no radius
    distance_stats          squared distances -> sums, maximum and counts, one read-back
    reconstruction_metrics  the three above on both meshes -> ReconMetrics
    cull_to_views           the faces some keyframe saw (applied to both meshes before scoring, as the published protocol does),
                            with the protocol's occlusion test on request (mesh_render.py)

The samples and the neighbours EQUAL those of the float64 restatement in tests/eval_cpu.py: areas are integers, the random numbers
a counter-based integer hash, the distances the float64 expression of include/mipsf_icp.h ordered by (distance, index).
Distances are cloud to cloud, not point to triangle: 200 000 samples of a 99 m^2 room lie about 2 cm apart, and a mean distance
cannot fall far below the samples' spacing however good the mesh is.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import pose_corrector as pc

SAMPLE_ERRORS = {_lib.EVAL_NO_AREA: "the mesh has no area (every face is degenerate or has an index out of range)",
                 _lib.EVAL_AREA_OVERFLOW: "the mesh's area is 2^23 m^2 or more"}


class ReconMetrics(NamedTuple):
    accuracy: float                 # mean distance reconstruction -> ground truth, metres
    completion: float               # mean distance ground truth -> reconstruction, metres
    completion_ratio: float         # share of ground-truth samples within `threshold` of the reconstruction
    accuracy_ratio: float           # share of reconstruction samples within `threshold` of the ground truth
    chamfer: float                  # (accuracy + completion) / 2
    accuracy_max: float
    completion_max: float
    area_rec: float                 # m^2, in units of 2^-40
    area_gt: float
    n_samples: int
    threshold: float


class DistanceStats(NamedTuple):
    sum_d: float
    sum_d2: float
    max_d: float
    within: int
    finite: int


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("mipsfusion_amd.evaluate runs on the GPU only (no CPU fallback exists)")
    return torch.device("cuda", torch.cuda.current_device())


def _split(mesh, faces=None):
    """(mesh) or (vertices, faces) -> (vertices, faces); a mesh is anything with .vertices and .faces (mesh.Mesh) or the pair
    (vertices, faces) itself, as synth.box_room_mesh returns it"""
    if faces is None:
        if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
            return mesh.vertices, mesh.faces
        if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
            return mesh[0], mesh[1]
        raise TypeError("expected a mesh with .vertices and .faces, a pair (vertices, faces), or vertices and faces")
    return mesh, faces


def _to_device(a, dtype, cols, what) -> torch.Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what}: expected [n,{cols}], got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(_device())
    return t.to(dtype).contiguous()


def _mesh_tensors(vertices, faces):
    v = _to_device(vertices, torch.float32, 3, "vertices")
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces))
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces: expected [F,3], got {tuple(f.shape)}")
    if f.numel() and (int(f.max()) > 2**31 - 1 or int(f.min()) < -2**31):
        raise ValueError("faces: an index does not fit int32")
    return v, f.to(v.device).to(torch.int32).contiguous()


def _ws_bytes(which: int, n: int) -> int:
    v = int(_lib.lib().mipsf_eval_workspace_bytes(which, n))
    if v == 0:
        raise RuntimeError(f"mipsf_eval_workspace_bytes({which}, {n}): out of range")
    return v


# --------------------------------------------------------------------------------------------------------------- enqueue only
def sample_enqueue(vertices: torch.Tensor, faces: torch.Tensor, n: int, seed: int = 0, points=None, face_of=None):
    """-> (points fp32 [n,3], face_of int32 [n], record uint8 [32] = mipsf_eval_sample_record), all on the device; nothing is
    read back.  When the record's status is not 0 the outputs were left as they were.  vertices fp32 [V,3], faces int32 [F,3]."""
    _lib.dptr(vertices, torch.float32), _lib.dptr(faces, torch.int32)
    V, F, n = vertices.shape[0], faces.shape[0], int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    dev = vertices.device
    with torch.cuda.device(dev):
        points = torch.empty(max(n, 1), 3, dtype=torch.float32, device=dev)[:n] if points is None else points
        face_of = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n] if face_of is None else face_of
        if tuple(points.shape) != (n, 3) or tuple(face_of.shape) != (n,):
            raise ValueError("points / face_of: expected [n,3] / [n]")
        record = torch.zeros(_lib.EVAL_SAMPLE_RECORD_BYTES, dtype=torch.uint8, device=dev)
        ws = pc._bytes(_ws_bytes(_lib.EVAL_WS_SAMPLE, F), dev)
        a = _lib.EvalSampleArgs.new(V=V, F=F, n=n, seed=int(seed) & 0xFFFFFFFF, vertices=vertices.data_ptr(), faces=faces.data_ptr(),
                                    points=_lib.dptr(points), face_of=_lib.dptr(face_of, torch.int32), record=record.data_ptr(),
                                    workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_eval_sample(C.byref(a), _lib.stream_ptr()), "eval_sample")
    return points, face_of, record


def nearest_enqueue(source: torch.Tensor, target: torch.Tensor, max_cells: Optional[int] = None, min_edge: float = 0.0):
    """-> (index int32 [m], d2 float64 [m]) on the device; source, target fp32 [.,3]"""
    pc._points(source, "source"), pc._points(target, "target")
    m, dev = source.shape[0], source.device
    with torch.cuda.device(dev):
        grid, cells = pc.bin_enqueue(target, min_edge, max_cells)
        index = torch.empty(max(m, 1), dtype=torch.int32, device=dev)[:m]
        d2 = torch.empty(max(m, 1), dtype=torch.float64, device=dev)[:m]
        a = _lib.EvalNearestArgs.new(n_source=m, n_target=target.shape[0], max_cells=cells, source=source.data_ptr(),
                                     grid=grid.data_ptr(), index=index.data_ptr(), d2=d2.data_ptr())
        _lib.check(_lib.lib().mipsf_eval_nearest(C.byref(a), _lib.stream_ptr()), "eval_nearest")
    return index, d2


def stats_enqueue(d2: torch.Tensor, threshold: float) -> torch.Tensor:
    """squared distances float64 [n] -> record uint8 [64] = mipsf_eval_stats_record on the device"""
    _lib.dptr(d2, torch.float64)
    if d2.dim() != 1:
        raise ValueError(f"d2: expected [n], got {tuple(d2.shape)}")
    dev = d2.device
    with torch.cuda.device(dev):
        record = torch.zeros(_lib.EVAL_STATS_RECORD_BYTES, dtype=torch.uint8, device=dev)
        ws = pc._bytes(_ws_bytes(_lib.EVAL_WS_STATS, d2.shape[0]), dev)
        a = _lib.EvalStatsArgs.new(n=d2.shape[0], d2=d2.data_ptr(), threshold=float(threshold), record=record.data_ptr(),
                                   workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_eval_stats(C.byref(a), _lib.stream_ptr()), "eval_stats")
    return record


def read_sample_record(record: torch.Tensor) -> "_lib.EvalSampleRecord":
    return _lib.EvalSampleRecord.from_buffer_copy(record.cpu().numpy().tobytes())


def read_stats_record(record: torch.Tensor) -> DistanceStats:
    r = _lib.EvalStatsRecord.from_buffer_copy(record.cpu().numpy().tobytes())
    return DistanceStats(r.sum_d, r.sum_d2, math.sqrt(r.max_d2), int(r.within), int(r.finite))


# --------------------------------------------------------------------------------------------------------------- public
def sample_surface(vertices, faces=None, n: int = 200_000, seed: int = 0):
    """n area-uniform samples of a mesh -> (points fp32 [n,3], face_of int32 [n], area in m^2), tensors on the device.
    ``sample_surface(mesh, n=...)`` or ``sample_surface(vertices, faces, n)``; numpy arrays or tensors.  Stratified: sample k
    falls into the k-th of n equal shares of the cumulative area, so every face gets its share to within two samples.  The same
    arguments give the same bytes.  Raises ValueError for a mesh without faces or without area (one 32-byte read-back)."""
    v, f = _mesh_tensors(*_split(vertices, faces))
    if f.shape[0] == 0:
        raise ValueError("sample_surface: a mesh without faces has no surface to sample")
    points, face_of, record = sample_enqueue(v, f, n, seed)
    rec = read_sample_record(record)
    if rec.status != _lib.EVAL_OK:
        raise ValueError("sample_surface: " + SAMPLE_ERRORS.get(rec.status, f"status {rec.status}"))
    return points, face_of, float(rec.area)


def nearest_distance(source, target, max_cells: Optional[int] = None, min_edge: float = 0.0):
    """-> (index int32 [m]: the nearest target point of every source point, d2 float64 [m]: its squared distance), however far
    away it is; -1 and inf only for an empty target.  Exact: the float64 distance of include/mipsf_icp.h, ties to the lower
    index; neither max_cells nor min_edge (the grid over the target) reaches a result.  Written for a reconstruction against its
    ground truth: a point R cells away from the target costs O(R^3) cell visits."""
    s, t = _to_device(source, torch.float32, 3, "source"), _to_device(target, torch.float32, 3, "target")
    return nearest_enqueue(s, t.to(s.device), max_cells, min_edge)


def distance_stats(d2, threshold: float) -> DistanceStats:
    """squared distances float64 [n] (device) -> DistanceStats; entries that are not finite are counted out of everything but n"""
    return read_stats_record(stats_enqueue(d2, threshold))


def reconstruction_metrics(mesh_rec, mesh_gt, n_samples: int = 200_000, threshold: float = 0.05, seed: int = 0) -> ReconMetrics:
    """Accuracy / completion / completion ratio of a reconstruction against its ground truth (metres; both meshes in the same
    frame, culled the same way beforehand: cull_to_views).  n_samples points per mesh, streams `seed` and `seed + 1`."""
    if n_samples < 1:
        raise ValueError("n_samples must be positive")
    p_rec, _, area_rec = sample_surface(mesh_rec, n=n_samples, seed=seed)
    p_gt, _, area_gt = sample_surface(mesh_gt, n=n_samples, seed=seed + 1)
    p_gt = p_gt.to(p_rec.device)
    rec_to_gt = stats_enqueue(nearest_enqueue(p_rec, p_gt)[1], threshold)
    gt_to_rec = stats_enqueue(nearest_enqueue(p_gt, p_rec)[1], threshold)
    acc, comp = read_stats_record(rec_to_gt), read_stats_record(gt_to_rec)
    accuracy, completion = acc.sum_d / n_samples, comp.sum_d / n_samples
    return ReconMetrics(accuracy, completion, comp.within / n_samples, acc.within / n_samples, 0.5 * (accuracy + completion),
                        acc.max_d, comp.max_d, area_rec, area_gt, int(n_samples), float(threshold))


def cull_to_views(mesh, kf_c2w, kf_max_depth, K, W, H, edge=20, occlusion=False, occluder=None, eps=None):
    """The faces whose three vertices some keyframe saw -> mesh.Mesh with the same vertices.
    occlusion=False (upstream's culling, which has no occlusion test): scene_mesh.point_mask -- inside the image by `edge` pixels,
    in front of the camera, nearer than the keyframe's largest depth.
    occlusion=True (the published protocol): mesh_render.visible_points -- the same frustum test in float64 and, besides, not more
    than `eps` metres behind the depth image of `occluder` rendered from that keyframe (the mesh itself when occluder is None; the
    ground truth when both meshes are to be culled alike).  `eps` has no default: the published value is not on record here."""
    from . import mesh as mesh_mod
    from . import scene_mesh
    vertices, faces = _split(mesh)
    v, f = _mesh_tensors(vertices, faces)
    if occlusion:
        from . import mesh_render
        if eps is None:
            raise ValueError("cull_to_views(occlusion=True) needs eps: how far behind the rendered depth a vertex still counts as seen")
        depth, _ = mesh_render.render_mesh_depth(mesh if occluder is None else occluder, kf_c2w, K, H, W)
        seen = mesh_render.visible_points(v, depth, kf_c2w, kf_max_depth, K, edge, eps)
    else:
        if occluder is not None or eps is not None:
            raise ValueError("cull_to_views: occluder and eps belong to occlusion=True")
        seen = scene_mesh.point_mask(v, kf_c2w, kf_max_depth, K, W, H, edge)
    fl = f.to(torch.int64)
    ok = (fl >= 0).all(1) & (fl < v.shape[0]).all(1)
    keep = torch.zeros(f.shape[0], dtype=torch.bool, device=f.device)
    keep[ok] = seen[fl[ok]].all(1)
    kept, = mesh_mod.filter_faces(f[keep])
    colors = getattr(mesh, "vertex_colors", None)
    return mesh_mod.Mesh(np.asarray(vertices.detach().cpu() if torch.is_tensor(vertices) else vertices, dtype=np.float64),
                         kept.cpu().numpy().astype(np.int64), colors)
