"""A triangle mesh as per-pixel depth from camera poses, and the two uses the NICE-SLAM / Co-SLAM evaluation has for it: depth L1
between the rendered reconstruction and the rendered ground truth, and the occlusion test of the culling.  The published recipes
render with a host library; here every step is a HIP kernel of ``csrc/raster.hip`` (C ABI: include/mipsf_raster.h):

    render_mesh_depth   mesh + poses -> depth fp32 [n,H,W] (0 = nothing hit) and face int32 [n,H,W] (-1 = nothing hit)
    depth_l1            two meshes rendered from the same views -> DepthMetrics
    visible_points      which points some view sees, in front of a depth stack (evaluate.cull_to_views(occlusion=True))

and, on top of the face image, the kernels of ``csrc/shade.hip`` (C ABI: include/mipsf_shade.h):

    vertex_normals      area-weighted normals of a mesh's vertices, the sum of every vertex in ascending face index
    render_mesh         mesh + poses -> MeshRender: depth, face, interpolated vertex colour, world-frame normals, head-lit shading
    mesh_render_metrics the rendered colour against captured frames (image_metrics) and the depth beside it

The depth words and the face indices EQUAL those of the float64 restatement in tests/raster_cpu.py: the rule is fixed operation by
operation in the header, the winner of a pixel is an integer minimum; the colour, normal and shaded words and the vertex normals
EQUAL those of tests/shade_cpu.py the same way.  It also serves as a third synthetic scene source: depth
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


# --------------------------------------------------------------------------------------------------------------- shading
class MeshRender(NamedTuple):
    depth: torch.Tensor              # fp32 [n,H,W], 0 = nothing hit: render_mesh_depth's
    face: torch.Tensor               # int32 [n,H,W], -1 = nothing hit: render_mesh_depth's
    color: Optional[torch.Tensor]    # fp32 [n,H,W,3]: the vertex colours interpolated, the background where nothing is hit; None without colours
    normals: Optional[torch.Tensor]  # fp32 [n,H,W,3]: unit normals in the world frame, turned towards the camera; 0 0 0 where there is none
    shaded: Optional[torch.Tensor]   # fp32 [n,H,W]: |cos| of the angle between the normal and the pixel's ray, 0 where there is no normal


class MeshRenderMetrics(NamedTuple):
    image: "object"                  # image_metrics.ImageMetrics of the rendered colour against the captured one, both times the mask
    depth_l1: float                  # mean over the views of depth_l1_per_view, metres
    depth_l1_per_view: Tuple[float, ...]     # mean |rendered - captured| over the masked pixels of a view; nan when there are none
    coverage: float                  # the share of all pixels the mask keeps
    n_views: int


SHADE_MODES = {"flat": _lib.SHADE_FLAT, "smooth": _lib.SHADE_SMOOTH}


def _mesh_parts(mesh):
    """-> ((vertices, faces), vertex colours or None): a mesh with .vertices, .faces and maybe .vertex_colors (mesh.Mesh), a pair
    (vertices, faces), or a triple (vertices, faces, colours)"""
    if not hasattr(mesh, "vertices") and isinstance(mesh, (tuple, list)) and len(mesh) == 3:
        return (mesh[0], mesh[1]), mesh[2]
    return _split(mesh), getattr(mesh, "vertex_colors", None)


def vertex_normals_enqueue(vertices: torch.Tensor, faces: torch.Tensor, out=None, workspace=None) -> torch.Tensor:
    """One launch of mipsf_shade_vertex_normals -> normals fp32 [V,3] on the device; nothing is read back.  vertices fp32 [V,3],
    faces int32 [F,3], on the device."""
    _lib.dptr(vertices, torch.float32), _lib.dptr(faces, torch.int32)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"expected vertices [V,3] and faces [F,3], got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    with torch.cuda.device(dev):
        out = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)[:V] if out is None else out
        if tuple(out.shape) != (V, 3):
            raise ValueError("normals: expected [V,3]")
        # what is out of range has no workspace size: a granule is handed over and the library refuses with its own message
        size = int(_lib.lib().mipsf_shade_workspace_bytes(_lib.SHADE_WS_VERTEX_NORMALS, V, F)) if max(V, F) < 1 << 32 else 0
        ws = pc._bytes(max(size, 16), dev) if workspace is None else workspace
        a = _lib.ShadeVertexNormalsArgs.new(V=V, F=F, vertices=vertices.data_ptr(), faces=faces.data_ptr(), normals=_lib.dptr(out),
                                            workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_shade_vertex_normals(C.byref(a), _lib.stream_ptr()), "shade_vertex_normals")
    return out


def vertex_normals(mesh) -> np.ndarray:
    """-> fp32 [V,3] on the host: the unit normal of every vertex, the sum of the incident faces' cross products (so weighted by
    area) in ascending face index; 0 0 0 for a vertex no face names or whose faces cancel.  A face with an index out of range or a
    vertex that is not finite adds nothing.  One read-back."""
    v, f = _mesh_tensors(*_mesh_parts(mesh)[0])
    return vertex_normals_enqueue(v, f).cpu().numpy()


def shade_enqueue(vertices: torch.Tensor, faces: torch.Tensor, poses: torch.Tensor, K, face: torch.Tensor, colors=None, vertex_normals=None,
                  mode: int = _lib.SHADE_FLAT, background=(0.0, 0.0, 0.0), color=None, normals=None, shaded=None, record=None):
    """One launch of mipsf_shade_pixels over a face image int32 [n,H,W] -> record uint64 [2] (hits, shaded) on the device; nothing
    is read back.  color fp32 [n,H,W,3], normals fp32 [n,H,W,3] and shaded fp32 [n,H,W] are written when given; colors and
    vertex_normals fp32 [V,3]; everything on the device."""
    _lib.dptr(vertices, torch.float32), _lib.dptr(faces, torch.int32), _lib.dptr(poses, torch.float32), _lib.dptr(face, torch.int32)
    if face.dim() != 3 or face.shape[0] != poses.shape[0]:
        raise ValueError(f"face image: expected [n,H,W] with n = {poses.shape[0]}, got {tuple(face.shape)}")
    fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
    V, F, (n, H, W), dev = vertices.shape[0], faces.shape[0], face.shape, vertices.device
    for t, shape, what in ((colors, (V, 3), "colors"), (vertex_normals, (V, 3), "vertex_normals"), (color, (n, H, W, 3), "color"),
                           (normals, (n, H, W, 3), "normals"), (shaded, (n, H, W), "shaded")):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected {shape}, got {tuple(t.shape)}")
    with torch.cuda.device(dev):
        record = torch.empty(_lib.SHADE_RECORD_WORDS, dtype=torch.int64, device=dev) if record is None else record
        a = _lib.ShadePixelsArgs.new(V=V, F=F, n=n, H=H, W=W, flags=int(mode), fx=fx, fy=fy, cx=cx, cy=cy,
                                     background=(C.c_float * 3)(*[float(b) for b in background]), vertices=vertices.data_ptr(),
                                     faces=faces.data_ptr(), poses=poses.data_ptr(), face=face.data_ptr(), colors=_lib.dptr(colors),
                                     vertex_normals=_lib.dptr(vertex_normals), color=_lib.dptr(color), normals=_lib.dptr(normals),
                                     shaded=_lib.dptr(shaded), record=_lib.dptr(record, torch.int64))
        _lib.check(_lib.lib().mipsf_shade_pixels(C.byref(a), _lib.stream_ptr()), "shade_pixels")
    return record


def render_mesh(mesh, c2w, K, H: int, W: int, near: float = 0.0, far: float = math.inf, normals: Optional[str] = "smooth",
                background=(0.0, 0.0, 0.0), views_per_launch: Optional[int] = None) -> MeshRender:
    """-> MeshRender of device tensors: what the mesh looks like from every pose.  depth and face are render_mesh_depth's own (the
    same call).  color [n,H,W,3] interpolates the mesh's vertex colours over the face a pixel's ray hits and is `background` where it
    hits nothing; None for a mesh without colours.  normals [n,H,W,3] are unit vectors in the world frame, turned towards the camera
    (the mesh is two-sided): "smooth" interpolates the area-weighted vertex normals (vertex_normals), "flat" takes the face's own,
    None skips normals and shaded.  shaded [n,H,W] is the grey head-lit image: |cos| of the angle between the normal and the
    pixel's ray.  A pixel nothing is hit at, or whose normal has no direction, has normal 0 0 0 and shaded 0.  mesh: anything with
    .vertices, .faces and maybe .vertex_colors (mesh.Mesh), a pair, or a triple with the colours.  The views are cut into launches
    as render_mesh_depth cuts them; the cut does not reach a byte.  Nothing is read back."""
    if normals is not None and normals not in SHADE_MODES:
        raise ValueError(f"normals: expected 'smooth', 'flat' or None, got {normals!r}")
    pair, colors = _mesh_parts(mesh)
    v, f = _mesh_tensors(*pair)
    poses = _poses(c2w, v.device)
    n, H, W = poses.shape[0], int(H), int(W)
    depth, face = render_mesh_depth((v, f), poses, K, H, W, near, far, views_per_launch)
    per = views_per_launch_for(n, f.shape[0], H, W) if views_per_launch is None else int(views_per_launch)
    with torch.cuda.device(v.device):
        cols = None if colors is None else _to_colors(colors, v)
        vn = vertex_normals_enqueue(v, f) if normals == "smooth" else None
        color = torch.empty(n, H, W, 3, dtype=torch.float32, device=v.device) if cols is not None else None
        nrm = torch.empty(n, H, W, 3, dtype=torch.float32, device=v.device) if normals is not None else None
        shaded = torch.empty(n, H, W, dtype=torch.float32, device=v.device) if normals is not None else None
        if color is not None or nrm is not None:
            part = lambda t, k: None if t is None else t[k:k + per]                          # noqa: E731
            for k in range(0, n, per):
                shade_enqueue(v, f, poses[k:k + per], K, face[k:k + per], cols, vn, SHADE_MODES.get(normals, _lib.SHADE_FLAT), background,
                              part(color, k), part(nrm, k), part(shaded, k))
    return MeshRender(depth, face, color, nrm, shaded)


def _to_colors(colors, v: torch.Tensor) -> torch.Tensor:
    c = colors if torch.is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(colors))
    if tuple(c.shape) != tuple(v.shape):
        raise ValueError(f"vertex colours: expected {tuple(v.shape)}, got {tuple(c.shape)}")
    return c.to(v.device).to(torch.float32).contiguous()


def mesh_render_metrics(mesh, c2w, K, rgb, depth=None, near: float = 0.0, far: float = math.inf, background=(0.0, 0.0, 0.0),
                        data_range: float = 1.0, ms_ssim: bool = True, views_per_launch: Optional[int] = None) -> MeshRenderMetrics:
    """The coloured mesh rendered from the poses and scored against the captured frames rgb [n,H,W,3] (and depth [n,H,W], if
    given): ``image_metrics.image_metrics`` of the rendered colour against rgb with `mask` = the pixels the mesh hits (and, when
    depth is given, that have captured depth > 0), and the mean |rendered - captured| depth over those pixels (``l1_enqueue`` of the
    two stacks, both zeroed outside the mask; nan without captured depth).  As image_metrics' docstring says, its mask MULTIPLIES
    both images and the means then run over ALL pixels: a frame the mesh covers half of has half its pixels equal (0 against 0), so
    PSNR and SSIM are comparable only between renders of similar coverage, which `coverage` reports.  This function has no image
    arithmetic of its own.  MS-SSIM needs sides above 160 (``ms_ssim=False`` skips it, as in image_metrics)."""
    from . import image_metrics as im
    pair, colors = _mesh_parts(mesh)
    if colors is None:
        raise ValueError("mesh_render_metrics: the mesh has no vertex colours")
    gt = torch.as_tensor(np.asarray(rgb)) if not torch.is_tensor(rgb) else rgb
    if gt.dim() == 3:
        gt = gt[None]
    n, H, W = int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2])
    r = render_mesh((pair[0], pair[1], colors), c2w, K, H, W, near, far, None, background, views_per_launch)
    dev = r.depth.device
    if r.depth.shape[0] != n:
        raise ValueError(f"mesh_render_metrics: {r.depth.shape[0]} poses and {n} frames")
    mask = r.face >= 0
    gt_d = None
    if depth is not None:
        gt_d = (torch.as_tensor(np.asarray(depth)) if not torch.is_tensor(depth) else depth).to(dev).to(torch.float32).reshape(n, H, W)
        mask = mask & (gt_d > 0)
    image = im.image_metrics(r.color, gt.to(dev), data_range, ms_ssim, mask)
    per_view = tuple(math.nan for _ in range(n))
    if gt_d is not None:
        zero = torch.zeros_like(r.depth)
        recs = read_l1_records(l1_enqueue(torch.where(mask, r.depth, zero).contiguous(), torch.where(mask, gt_d, zero).contiguous()))
        per_view = tuple(q.sum_all / int(q.both) if q.both else math.nan for q in recs)
    return MeshRenderMetrics(image, math.fsum(per_view) / n, per_view, float(mask.sum()) / (n * H * W), n)
