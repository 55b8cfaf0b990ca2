"""A triangle mesh as per-pixel depth from camera poses, and the two uses the NICE-SLAM / Co-SLAM evaluation has for it: depth L1
between the rendered reconstruction and the rendered ground truth, and the occlusion test of the culling.  The published recipes
render with a host library; here every step is a HIP kernel of ``csrc/raster.hip`` (C ABI: include/mipsf_raster.h):

    render_mesh_depth   mesh + poses -> depth fp32 [n,H,W] (0 = nothing hit) and face int32 [n,H,W] (-1 = nothing hit)
    depth_l1            two meshes rendered from the same views -> DepthMetrics
    visible_points      which points some view sees, in front of a depth stack (evaluate.cull_to_views(occlusion=True))

The depth words and the face indices EQUAL those of the float64 restatement in tests/raster_cpu.py: the rule is fixed operation by
operation in the header, the winner of a pixel is an integer minimum.  It also serves as a third synthetic scene source: depth
frames of any mesh, where ``synth`` renders its two analytic scenes only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import pose_corrector as pc
from .evaluate import _mesh_tensors, _split
from .scene_mesh import _intrinsics

WORKSPACE_CAP = 256 << 20          # bytes of keys and counts one launch may ask for (render_mesh_depth cuts the views to fit)


class DepthMetrics(NamedTuple):
    l1: float                        # mean over the views of sum_all / (H*W): the published number (a miss counts as depth 0), metres
    l1_both: float                   # sum of |difference| over the pixels both meshes hit / their number; nan when there are none
    both: float                      # shares of all pixels of all views; the four add up to 1
    rec_only: float
    gt_only: float
    neither: float
    l1_per_view: Tuple[float, ...]
    l1_both_per_view: Tuple[float, ...]
    n_views: int
    pixels: int                      # H * W


def _poses(c2w, dev) -> torch.Tensor:
    if not torch.is_tensor(c2w):
        c2w = torch.stack([torch.as_tensor(p) for p in c2w]) if isinstance(c2w, (list, tuple)) else torch.as_tensor(np.asarray(c2w))
    if c2w.dim() == 2:
        c2w = c2w[None]
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4):
        raise ValueError(f"c2w: expected [n,4,4], got {tuple(c2w.shape)}")
    return c2w.to(dev).to(torch.float32).contiguous()


def _ws_bytes(which: int, n: int, F: int, H: int, W: int) -> int:
    if min(n, F, H, W) < 0 or max(n, F, H, W) >= 1 << 32:
        raise RuntimeError(f"mipsf_raster_workspace_bytes({which}, {n}, {F}, {H}, {W}): out of range")
    v = int(_lib.lib().mipsf_raster_workspace_bytes(which, n, F, H, W))
    if v == 0:
        raise RuntimeError(f"mipsf_raster_workspace_bytes({which}, {n}, {F}, {H}, {W}): out of range "
                           f"(at most {_lib.RASTER_MAX_SIDE} pixels a side, {_lib.RASTER_MAX_PIXELS} pixels and "
                           f"{_lib.RASTER_MAX_ITEMS} (view, face) pairs a launch, at least one of each)")
    return v


# --------------------------------------------------------------------------------------------------------------- enqueue only
def render_enqueue(vertices: torch.Tensor, faces: torch.Tensor, poses: torch.Tensor, K, H: int, W: int, near: float = 0.0,
                   far: float = math.inf, depth=None, face=None, workspace=None, stages: int = 0):
    """One launch of mipsf_raster_depth -> (depth fp32 [n,H,W], face int32 [n,H,W]) on the device; nothing is read back.
    vertices fp32 [V,3], faces int32 [F,3], poses fp32 [n,4,4], all on the device."""
    _lib.dptr(vertices, torch.float32), _lib.dptr(faces, torch.int32), _lib.dptr(poses, torch.float32)
    fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
    V, F, n, H, W = vertices.shape[0], faces.shape[0], poses.shape[0], int(H), int(W)
    dev = vertices.device
    with torch.cuda.device(dev):
        depth = torch.empty(max(n * H * W, 1), dtype=torch.float32, device=dev)[:n * H * W].view(n, H, W) if depth is None else depth
        face = torch.empty(max(n * H * W, 1), dtype=torch.int32, device=dev)[:n * H * W].view(n, H, W) if face is None else face
        if tuple(depth.shape) != (n, H, W) or tuple(face.shape) != (n, H, W):
            raise ValueError("depth / face: expected [n,H,W]")
        # what is out of range has no workspace size: a granule is handed over and the library refuses with its own message
        size = int(_lib.lib().mipsf_raster_workspace_bytes(_lib.RASTER_WS_DEPTH, n, F, H, W)) if max(n, F, H, W) < 1 << 32 else 0
        ws = pc._bytes(max(size, 16), dev) if workspace is None else workspace
        a = _lib.RasterDepthArgs.new(V=V, F=F, n=n, H=H, W=W, stages=int(stages), fx=fx, fy=fy, cx=cx, cy=cy, near=float(near),
                                     far=float(far), vertices=vertices.data_ptr(), faces=faces.data_ptr(), poses=poses.data_ptr(),
                                     depth=_lib.dptr(depth), face=_lib.dptr(face, torch.int32),
                                     workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_raster_depth(C.byref(a), _lib.stream_ptr()), "raster_depth")
    return depth, face


def l1_enqueue(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """two depth stacks fp32 [n,H,W] on the device -> records uint8 [n,64] = mipsf_raster_l1_record per view, on the device"""
    _lib.dptr(a, torch.float32), _lib.dptr(b, torch.float32)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError(f"depth stacks: expected two of [n,H,W], got {tuple(a.shape)} and {tuple(b.shape)}")
    n, H, W = a.shape
    dev = a.device
    with torch.cuda.device(dev):
        records = torch.zeros(max(n, 1), _lib.RASTER_L1_RECORD_BYTES, dtype=torch.uint8, device=dev)[:n]
        size = int(_lib.lib().mipsf_raster_workspace_bytes(_lib.RASTER_WS_L1, n, 0, H, W))
        ws = pc._bytes(max(size, 16), dev)
        args = _lib.RasterL1Args.new(n=n, H=H, W=W, a=a.data_ptr(), b=b.data_ptr(), records=records.data_ptr(), workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_raster_l1(C.byref(args), _lib.stream_ptr()), "raster_l1")
    return records


def visible_enqueue(points: torch.Tensor, depth: torch.Tensor, poses: torch.Tensor, max_depth: torch.Tensor, K, edge: float,
                    eps: float) -> torch.Tensor:
    """-> seen uint8 [m] on the device; points fp32 [m,3], depth fp32 [n,H,W], poses fp32 [n,4,4], max_depth fp32 [n]"""
    pc._points(points, "points")
    _lib.dptr(depth, torch.float32), _lib.dptr(poses, torch.float32), _lib.dptr(max_depth, torch.float32)
    if depth.dim() != 3 or tuple(poses.shape) != (depth.shape[0], 4, 4) or tuple(max_depth.shape) != (depth.shape[0],):
        raise ValueError("expected depth [n,H,W], poses [n,4,4], max_depth [n]")
    fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
    m, (n, H, W), dev = points.shape[0], depth.shape, points.device
    with torch.cuda.device(dev):
        seen = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)[:m]
        a = _lib.RasterVisibleArgs.new(m=m, n=n, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, edge=float(edge), eps=float(eps),
                                       points=points.data_ptr(), depth=depth.data_ptr(), poses=poses.data_ptr(),
                                       max_depth=max_depth.data_ptr(), seen=seen.data_ptr())
        _lib.check(_lib.lib().mipsf_raster_visible(C.byref(a), _lib.stream_ptr()), "raster_visible")
    return seen


def read_l1_records(records: torch.Tensor):
    raw = records.cpu().numpy().tobytes()
    size = _lib.RASTER_L1_RECORD_BYTES
    return [_lib.RasterL1Record.from_buffer_copy(raw[k * size:(k + 1) * size]) for k in range(records.shape[0])]


# --------------------------------------------------------------------------------------------------------------- public
def views_per_launch_for(n: int, F: int, H: int, W: int, cap: int = WORKSPACE_CAP) -> int:
    """the most views of one launch whose keys (8 bytes a pixel) and counts (8 bytes a face) fit `cap` bytes and the header's limits"""
    per_view = 8 * (H * W + F) + 1
    most = min(cap // per_view, _lib.RASTER_MAX_PIXELS // max(H * W, 1), _lib.RASTER_MAX_ITEMS // max(F, 1))
    return int(max(1, min(n, most)))


def render_mesh_depth(mesh, c2w, K, H: int, W: int, near: float = 0.0, far: float = math.inf, views_per_launch: Optional[int] = None):
    """-> (depth fp32 [n,H,W], face int32 [n,H,W]) on the device: the z-depth of the nearest face along every pixel's ray and that
    face's index; 0 and -1 where nothing is hit between `near` and `far`.  mesh: anything with .vertices and .faces, or the pair;
    c2w [n,4,4] or [4,4], camera to world in the datasets' OpenGL convention; K a 3x3 matrix or (fx, fy, cx, cy).  The mesh is
    two-sided.  The views are cut into launches of `views_per_launch` (by default as many as fit WORKSPACE_CAP); the cut does not
    reach a result."""
    v, f = _mesh_tensors(*_split(mesh))
    poses = _poses(c2w, v.device)
    n, H, W = poses.shape[0], int(H), int(W)
    if n == 0 or f.shape[0] == 0 or H * W <= 0:
        raise ValueError(f"render_mesh_depth: {n} views, {f.shape[0]} faces, {H} x {W} pixels: there must be at least one of each")
    per = views_per_launch_for(n, f.shape[0], H, W) if views_per_launch is None else int(views_per_launch)
    if per < 1:
        raise ValueError("views_per_launch must be positive")
    with torch.cuda.device(v.device):
        _ws_bytes(_lib.RASTER_WS_DEPTH, min(per, n), f.shape[0], H, W)                # refuses what is out of range before anything runs
        depth = torch.empty(n, H, W, dtype=torch.float32, device=v.device)
        face = torch.empty(n, H, W, dtype=torch.int32, device=v.device)
        for k in range(0, n, per):
            render_enqueue(v, f, poses[k:k + per], K, H, W, near, far, depth[k:k + per], face[k:k + per])
    return depth, face


def metrics_from_records(recs, H: int, W: int) -> DepthMetrics:
    """the per-view records of mipsf_raster_l1 -> DepthMetrics, combined on the host with math.fsum"""
    n, hw = len(recs), H * W
    per_view = tuple(r.sum_all / hw for r in recs)
    per_view_both = tuple(r.sum_both / r.both if r.both else math.nan for r in recs)
    both = sum(int(r.both) for r in recs)
    total = n * hw
    return DepthMetrics(math.fsum(per_view) / n, math.fsum(r.sum_both for r in recs) / both if both else math.nan, both / total,
                        sum(int(r.rec_only) for r in recs) / total, sum(int(r.gt_only) for r in recs) / total,
                        sum(int(r.neither) for r in recs) / total, per_view, per_view_both, n, hw)


def depth_l1(mesh_rec, mesh_gt, c2w, K, H: int, W: int, near: float = 0.0, far: float = math.inf) -> DepthMetrics:
    """Depth L1 of a reconstruction against its ground truth: both meshes rendered from the same views, the mean absolute
    difference of the depth images (metres; both meshes in the same frame).  One read-back of 64 bytes per view."""
    d_rec, _ = render_mesh_depth(mesh_rec, c2w, K, H, W, near, far)
    d_gt, _ = render_mesh_depth(mesh_gt, c2w, K, H, W, near, far)
    return metrics_from_records(read_l1_records(l1_enqueue(d_rec, d_gt.to(d_rec.device))), int(H), int(W))


def visible_points(points, depth, c2w, max_depth, K, edge: float, eps: float) -> torch.Tensor:
    """-> bool [m] on the device: whether some view sees each point: inside the image by `edge` pixels, in front of the camera,
    nearer than the view's max_depth, and not more than `eps` behind the depth image at its pixel (a pixel of depth 0 occludes
    nothing).  depth fp32 [n,H,W] as render_mesh_depth gives it."""
    from .evaluate import _to_device
    p = _to_device(points, torch.float32, 3, "points")
    poses = _poses(c2w, p.device)
    md = (max_depth if torch.is_tensor(max_depth) else torch.as_tensor(np.asarray(max_depth))).to(p.device).to(torch.float32).reshape(-1)
    return visible_enqueue(p, depth.to(p.device).to(torch.float32).contiguous(), poses, md.contiguous(), K, edge, eps).bool()
