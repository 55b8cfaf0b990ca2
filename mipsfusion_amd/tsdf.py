"""Depth frames fused into a dense TSDF volume on the GPU, and the volume as a mesh.  The step between depth images and a volume:
the rendered-depth meshing protocol of the papers that followed the reference (render depth from the neural map at the estimated
poses, TSDF-fuse the images, march), the classical baseline (fuse the sensor depth), and a stand-in ground truth for a sequence
that has none.  Upstream fuses with a host library; here it is the kernel of ``csrc/tsdf.hip`` (C ABI: include/mipsf_tsdf.h;
DESIGN.md 4.19):

    TSDFVolume                 the state (tsdf, weight, optionally colour, all on the device) and integrate / volume / extract_mesh,
                               raycast (the volume as depth, normal and colour images) and track (a depth frame registered
                               against such images); kernels of ``csrc/tsdf_track.hip``, C ABI include/mipsf_track.h, DESIGN.md 4.21
                               track(rgb=...) adds a photometric row per pair against the ray cast's colour, which holds the pose
                               along walls: ``csrc/track_color.hip``, include/mipsf_track_color.h, DESIGN.md 4.23
                               deintegrate / reintegrate take fused views out again and fuse them at new poses, the step after a
                               loop closure: ``csrc/tsdf_remove.hip``, include/mipsf_deintegrate.h, DESIGN.md 4.26
    tsdf_odometry              depth frames -> poses: every frame registered against the ray cast of the volume, then fused
    tsdf_mesh_from_frames      depth frames + poses -> mesh.Mesh
    mesh_from_rendered_depth   model + poses -> rendered depth -> mesh.Mesh

The tsdf, weight and colour words EQUAL those of the float64 restatement in tests/tsdf_cpu.py: the rule is fixed operation by
operation in the header and a voxel takes its views in ascending order, whatever the cut into calls.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .mesh import Mesh, marching_cubes, save_ply
from .mesh_render import _poses
from .scene_mesh import _intrinsics


class TSDFCounts(NamedTuple):
    updates: int                     # (voxel, view) pairs that updated, over the calls of one integrate()
    observed: int                    # voxels whose weight is positive afterwards


class RemoveCounts(NamedTuple):
    removed: int                     # (voxel, view) pairs taken out, over the calls of one deintegrate()
    missing: int                     # pairs the views hit whose voxel had no positive weight left (a diagnostic, not a guarantee)
    emptied: int                     # removals that brought a voxel back to the never-observed state
    observed: int                    # voxels whose weight is positive afterwards


class ReintegrateCounts(NamedTuple):
    views_moved: int                 # views removed at their old pose and fused at their new one
    removed: RemoveCounts
    fused: TSDFCounts


class Raycast(NamedTuple):
    depth: torch.Tensor              # fp32 [n,H,W], z-depth, 0 = no hit
    normals: Optional[torch.Tensor]  # fp32 [n,H,W,3], world frame, into free space, 0 0 0 = none
    color: Optional[torch.Tensor]    # fp32 [n,H,W,3]
    hits: torch.Tensor               # int64 [2] on the device: pixels with a depth, bricks marked


class TrackResult(NamedTuple):
    pose: torch.Tensor               # fp32 [4,4], camera to world
    transformation: torch.Tensor     # float64 [4,4], the same before its rounding
    n_correspondences: int
    fitness: float                   # pairs over the usable live pixels
    inlier_rmse: float
    iterations: int


class ColorTrackResult(NamedTuple):
    pose: torch.Tensor               # the fields of TrackResult, then the photometric side of the last evaluation
    transformation: torch.Tensor
    n_correspondences: int
    fitness: float
    inlier_rmse: float
    iterations: int
    n_color: int                     # pairs that also gave a photometric row
    color_rmse: float                # of the intensity residuals, intensities in the units of rgb


# the colour term's weight against the geometric one (intensity^2 against metres^2): of 0.01, 0.1, 1 and 10 the one with the
# smallest worst final error over a lone wall, two walls and a corner of the box room
DEFAULT_COLOR_WEIGHT = 10.0


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("mipsfusion_amd.tsdf runs on the GPU only (no CPU fallback exists)")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mipsfusion_amd.tsdf runs on the GPU only (no CPU fallback exists)")
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def _images(a, dev, channels: int, what: str) -> torch.Tensor:
    """host or device, one image or a stack, a list of images -> fp32 [n,H,W] (channels = 0) or [n,H,W,3] on dev; a device fp32
    contiguous tensor is taken as it is"""
    if not torch.is_tensor(a):
        a = torch.stack([torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x) for x in a]) if isinstance(a, (list, tuple)) \
            else torch.as_tensor(np.asarray(a))
    want = 3 if channels == 0 else 4
    if a.dim() == want - 1:
        a = a[None]
    if a.dim() != want or (channels and a.shape[-1] != channels):
        raise ValueError(f"{what}: expected [n,H,W{',3' if channels else ''}] or one image, got {tuple(a.shape)}")
    return a.to(dev).to(torch.float32).contiguous()


def _moved(old: np.ndarray, new: np.ndarray, min_translation: float, min_rotation: float) -> np.ndarray:
    """fp32 poses [n,4,4] before and after -> bool [n], in float64: the translation changed by more than min_translation, or the
    rotation by more than min_rotation; with both at 0, any word of the pose differs.  The angle between two rotations is taken
    from their difference, 2 asin(|R_new - R_old|_F / (2 sqrt 2)): exact for rotation matrices, exactly 0 for equal words and
    proportional to the difference near 0, where the arc cosine of the trace turns a rounding of 1e-7 into 4e-4 rad.  A pose
    that is not finite (a lost frame, which fused nothing) on one side only counts as moved; on both sides, as not."""
    if min_translation < 0 or min_rotation < 0 or math.isnan(min_translation) or math.isnan(min_rotation):
        raise ValueError(f"min_translation {min_translation} and min_rotation {min_rotation} must not be negative")
    if min_translation == 0.0 and min_rotation == 0.0:
        return (np.ascontiguousarray(old).view(np.uint32) != np.ascontiguousarray(new).view(np.uint32)).reshape(len(old), -1).any(1)
    a, b = old.astype(np.float64), new.astype(np.float64)
    fine_a, fine_b = np.isfinite(a[:, :3]).all((1, 2)), np.isfinite(b[:, :3]).all((1, 2))
    with np.errstate(all="ignore"):
        shift = np.sqrt(((b[:, :3, 3] - a[:, :3, 3]) ** 2).sum(1))
        chord = np.sqrt(((b[:, :3, :3] - a[:, :3, :3]) ** 2).sum((1, 2)))
        turn = 2.0 * np.arcsin(np.minimum(chord / (2.0 * math.sqrt(2.0)), 1.0))
        return (fine_a != fine_b) | (fine_a & fine_b & ((shift > min_translation) | (turn > min_rotation)))


def _moved_views(poses_old: torch.Tensor, poses_new: torch.Tensor, min_translation: float, min_rotation: float) -> np.ndarray:
    """fp32 poses [n,4,4] before and after, host or device -> int64 [m]: the views ``_moved`` finds moved, ascending.  The selection
    of TSDFVolume.reintegrate and SparseTSDFVolume.reintegrate."""
    return np.nonzero(_moved(poses_old.cpu().numpy(), poses_new.cpu().numpy(), float(min_translation), float(min_rotation)))[0]


class TSDFVolume:
    """A dense TSDF volume on the device.  Voxel (i,j,k) sits at origin + voxel_size * (i,j,k) (float64, rounded to fp32 by the
    kernel); ``trunc`` is the truncation distance in metres.  tsdf is in units of trunc: 1 in free space, 0 on the surface,
    negative behind it down to -1; weight counts the views that updated the voxel, capped at ``max_weight``."""

    def __init__(self, origin, voxel_size: float, dims, trunc: float, color: bool = False, max_weight: float = math.inf, device=None):
        self.origin = np.asarray(origin, np.float64).reshape(3).copy()
        self.voxel_size, self.trunc, self.max_weight = float(voxel_size), float(trunc), float(max_weight)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f"dims: expected three positive counts, got {dims}")
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size)):
            raise ValueError(f"voxel_size {voxel_size} is not positive and finite")
        n = self.dims[0] * self.dims[1] * self.dims[2]
        if n > _lib.TSDF_MAX_VOXELS:
            raise ValueError(f"a grid of {self.dims[0]} x {self.dims[1]} x {self.dims[2]} voxels at voxel size {self.voxel_size} has "
                             f"2^31 voxels or more; choose a larger voxel size or smaller bounds")
        self.device = _device(device)
        self.ticks = tuple(self.origin[a] + self.voxel_size * np.arange(self.dims[a], dtype=np.float64) for a in range(3))
        with torch.cuda.device(self.device):
            self._ticks_dev = tuple(torch.from_numpy(t).to(self.device) for t in self.ticks)
            self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
            self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
            self.color = torch.zeros(self.dims + (3,), dtype=torch.float32, device=self.device) if color else None
        self._marks = None                   # the ray cast's brick marks (workspace of mipsf_track_raycast), made at the first cast

    def reset(self) -> None:
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()

    # ----------------------------------------------------------------------------------------------------------- enqueue only
    def integrate_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, rgb: Optional[torch.Tensor] = None,
                          depth_max: float = math.inf, record: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
        """One launch of mipsf_tsdf_integrate; nothing is read back.  depth fp32 [n,H,W], poses fp32 [n,4,4], rgb fp32 [n,H,W,3]
        or None, all on the device -> record int64 [2] on the device: (voxel, view) pairs updated, voxels with a positive weight"""
        _lib.dptr(depth), _lib.dptr(poses), _lib.dptr(rgb)
        if depth.dim() != 3 or tuple(poses.shape) != (depth.shape[0], 4, 4):
            raise ValueError(f"expected depth [n,H,W] and poses [n,4,4], got {tuple(depth.shape)} and {tuple(poses.shape)}")
        if rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"rgb: expected {tuple(depth.shape) + (3,)}, got {tuple(rgb.shape)}")
        if (rgb is None) != (self.color is None):
            raise ValueError("rgb goes with a volume made with color=True, and such a volume needs rgb")
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = depth.shape
        with torch.cuda.device(self.device):
            record = torch.empty(_lib.TSDF_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            a = _lib.TsdfIntegrateArgs.new(X=self.dims[0], Y=self.dims[1], Z=self.dims[2], n=n, H=H, W=W, flags=int(flags), fx=fx, fy=fy,
                                           cx=cx, cy=cy, trunc=self.trunc, depth_max=float(depth_max), max_weight=self.max_weight,
                                           depth=depth.data_ptr(), rgb=None if rgb is None else rgb.data_ptr(), poses=poses.data_ptr(),
                                           tsdf=_lib.dptr(self.tsdf), weight=_lib.dptr(self.weight), color=_lib.dptr(self.color),
                                           record=_lib.dptr(record, torch.int64))
            for d in range(3):
                a.ticks[d] = _lib.dptr(self._ticks_dev[d], torch.float64)
            _lib.check(_lib.lib().mipsf_tsdf_integrate(C.byref(a), _lib.stream_ptr()), "tsdf_integrate")
        return record

    def _removable(self) -> None:
        if math.isfinite(self.max_weight):
            raise ValueError(f"views cannot be removed from a volume made with max_weight {self.max_weight}: a capped running mean is a "
                             f"moving average, which has no inverse; make the volume with max_weight=inf")

    def deintegrate_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, rgb: Optional[torch.Tensor] = None,
                            depth_max: float = math.inf, record: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
        """One launch of mipsf_deintegrate_views, the inverse of integrate_enqueue for views fused with these very arguments;
        nothing is read back.  depth fp32 [n,H,W], poses fp32 [n,4,4], rgb fp32 [n,H,W,3] or None, all on the device -> record
        int64 [4] on the device: pairs removed, pairs missing, voxels emptied, voxels with a positive weight"""
        self._removable()
        _lib.dptr(depth), _lib.dptr(poses), _lib.dptr(rgb)
        if depth.dim() != 3 or tuple(poses.shape) != (depth.shape[0], 4, 4):
            raise ValueError(f"expected depth [n,H,W] and poses [n,4,4], got {tuple(depth.shape)} and {tuple(poses.shape)}")
        if rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"rgb: expected {tuple(depth.shape) + (3,)}, got {tuple(rgb.shape)}")
        if (rgb is None) != (self.color is None):
            raise ValueError("rgb goes with a volume made with color=True, and such a volume needs rgb")
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = depth.shape
        with torch.cuda.device(self.device):
            record = torch.empty(_lib.DEINTEGRATE_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            a = _lib.DeintegrateArgs.new(X=self.dims[0], Y=self.dims[1], Z=self.dims[2], n=n, H=H, W=W, flags=int(flags), fx=fx, fy=fy,
                                         cx=cx, cy=cy, trunc=self.trunc, depth_max=float(depth_max),
                                         depth=depth.data_ptr(), rgb=None if rgb is None else rgb.data_ptr(), poses=poses.data_ptr(),
                                         tsdf=_lib.dptr(self.tsdf), weight=_lib.dptr(self.weight), color=_lib.dptr(self.color),
                                         record=_lib.dptr(record, torch.int64))
            for d in range(3):
                a.ticks[d] = _lib.dptr(self._ticks_dev[d], torch.float64)
            _lib.check(_lib.lib().mipsf_deintegrate_views(C.byref(a), _lib.stream_ptr()), "deintegrate_views")
        return record

    def reintegrate_enqueue(self, depth: torch.Tensor, poses_old: torch.Tensor, poses_new: torch.Tensor, K,
                            rgb: Optional[torch.Tensor] = None, depth_max: float = math.inf, records=None, flags: int = 0):
        """deintegrate_enqueue at ``poses_old``, then integrate_enqueue at ``poses_new``, of every view given: two launches on the
        current stream, no selection and nothing read back, for use inside a captured sequence.  Device tensors as for
        integrate_enqueue; ``records`` (int64 [4], int64 [2]) keeps the two records in place -> (remove record, fuse record)"""
        self._removable()
        if tuple(poses_new.shape) != tuple(poses_old.shape):
            raise ValueError(f"poses: {tuple(poses_old.shape)} old and {tuple(poses_new.shape)} new")
        gone, fused = (None, None) if records is None else records
        gone = self.deintegrate_enqueue(depth, poses_old, K, rgb, depth_max, gone, flags)
        fused = self.integrate_enqueue(depth, poses_new, K, rgb, depth_max, fused, flags)
        return gone, fused

    def sample_enqueue(self, points: torch.Tensor) -> torch.Tensor:
        """points float64 [m,3] in index units on the device -> colour fp32 [m,3] on the device (mipsf_tsdf_sample)"""
        if self.color is None:
            raise ValueError("the volume was made without colour")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: expected [m,3], got {tuple(points.shape)}")
        m = points.shape[0]
        with torch.cuda.device(self.device):
            out = torch.empty(max(m, 1), 3, dtype=torch.float32, device=self.device)[:m]
            a = _lib.TsdfSampleArgs.new(X=self.dims[0], Y=self.dims[1], Z=self.dims[2], m=m, points=_lib.dptr(points, torch.float64),
                                        weight=_lib.dptr(self.weight), color=_lib.dptr(self.color), out=out.data_ptr())
            _lib.check(_lib.lib().mipsf_tsdf_sample(C.byref(a), _lib.stream_ptr()), "tsdf_sample")
        return out

    def raycast_enqueue(self, poses: torch.Tensor, K, H: int, W: int, near: float = 0.0, far: float = math.inf, step: Optional[float] = None,
                        min_weight: float = 1.0, normals: bool = True, color: bool = False, flags: int = 0) -> Raycast:
        """mipsf_track_raycast; nothing is read back.  poses fp32 [n,4,4] on the device -> Raycast of device tensors"""
        _lib.dptr(poses)
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
            raise ValueError(f"poses: expected [n,4,4], got {tuple(poses.shape)}")
        if color and self.color is None:
            raise ValueError("the volume was made without colour")
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = poses.shape[0], int(H), int(W)
        lib = _lib.lib()
        size = int(lib.mipsf_track_workspace_bytes(_lib.TRACK_WS_RAYCAST, *self.dims))
        if size == 0:
            raise ValueError(f"a volume of {self.dims} cannot be ray cast")
        with torch.cuda.device(self.device):
            if self._marks is None or self._marks.numel() < size:
                self._marks = torch.empty(size, dtype=torch.uint8, device=self.device)
            depth = torch.empty(n, H, W, dtype=torch.float32, device=self.device)
            nrm = torch.empty(n, H, W, 3, dtype=torch.float32, device=self.device) if normals else None
            col = torch.empty(n, H, W, 3, dtype=torch.float32, device=self.device) if color else None
            record = torch.empty(_lib.TRACK_RECORD_WORDS, dtype=torch.int64, device=self.device)
            a = _lib.TrackRaycastArgs.new(X=self.dims[0], Y=self.dims[1], Z=self.dims[2], n=n, H=H, W=W, flags=int(flags), voxel=self.voxel_size,
                                          trunc=self.trunc, fx=fx, fy=fy, cx=cx, cy=cy, near=float(near), far=float(far),
                                          step=0.5 * self.trunc if step is None else float(step), min_weight=float(min_weight),
                                          tsdf=_lib.dptr(self.tsdf), weight=_lib.dptr(self.weight),
                                          color=_lib.dptr(self.color) if color else None, poses=poses.data_ptr() if n else None,
                                          depth=depth.data_ptr() if n else None, normals=nrm.data_ptr() if normals and n else None,
                                          color_out=col.data_ptr() if color and n else None, record=_lib.dptr(record, torch.int64),
                                          workspace=self._marks.data_ptr())
            for d in range(3):
                a.origin[d] = float(self.origin[d])
            _lib.check(lib.mipsf_track_raycast(C.byref(a), _lib.stream_ptr()), "track_raycast")
        return Raycast(depth, nrm, col, record)

    def track_enqueue(self, depth: torch.Tensor, K, pose_init: torch.Tensor, pose_ref: Optional[torch.Tensor] = None,
                      model: Optional[Raycast] = None, max_dist: Optional[float] = None, max_iteration: int = 30,
                      relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, depth_max: float = math.inf, partner: bool = False,
                      rgb: Optional[torch.Tensor] = None, color_weight: Optional[float] = None, max_color_diff: float = math.inf,
                      relative_color_rmse: float = 1e-6, **raycast_kw):
        """The ray cast from pose_ref (unless ``model`` is given) and mipsf_track_register; nothing is read back.  depth fp32 [H,W],
        pose_init and pose_ref fp32 [4,4], all on the device -> (result float64 [20]: T row major, correspondences, fitness, inlier
        rmse, iterations; pose fp32 [4,4]) on the device (, partner int32 [H,W]).
        With ``rgb`` fp32 [H,W,3] on the device the ray cast also gives the model's colour and mipsf_track_register_color registers
        depth and colour (``color_weight``: DEFAULT_COLOR_WEIGHT unless given) -> (result float64 [22]: the same, then photometric
        rows and their rmse; pose) (, partner, color_partner int32 [H,W]: 1 where the pixel gave a photometric row)"""
        _lib.dptr(depth), _lib.dptr(pose_init), _lib.dptr(pose_ref), _lib.dptr(rgb)
        pose_ref = pose_init if pose_ref is None else pose_ref
        if depth.dim() != 2 or tuple(pose_init.shape) != (4, 4) or tuple(pose_ref.shape) != (4, 4):
            raise ValueError(f"expected depth [H,W] and poses [4,4], got {tuple(depth.shape)}, {tuple(pose_init.shape)}, {tuple(pose_ref.shape)}")
        H, W = depth.shape
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        if rgb is not None:
            if self.color is None:
                raise ValueError("rgb: the volume was made without colour (color=True)")
            if tuple(rgb.shape) != (H, W, 3):
                raise ValueError(f"rgb: expected {(H, W, 3)}, got {tuple(rgb.shape)}")
            if model is not None and model.color is None:
                raise ValueError("model: tracking with rgb needs a ray cast made with color=True")
            raycast_kw = dict(raycast_kw, color=True)
        if model is None:
            model = self.raycast_enqueue(pose_ref[None], K, H, W, **raycast_kw)
        if model.normals is None or tuple(model.depth.shape[-2:]) != (H, W) or model.depth.numel() != H * W:
            raise ValueError("model: one ray-cast view with normals, of the live frame's size")
        lib = _lib.lib()
        if rgb is not None:
            with torch.cuda.device(self.device):
                ws = torch.empty(int(lib.mipsf_track_workspace_bytes(_lib.TRACK_WS_REGISTER_COLOR, H, W, 0)), dtype=torch.uint8, device=self.device)
                result = torch.empty(_lib.TRACK_COLOR_RESULT_DOUBLES, dtype=torch.float64, device=self.device)
                pose = torch.empty(4, 4, dtype=torch.float32, device=self.device)
                mates = torch.empty(H, W, dtype=torch.int32, device=self.device) if partner else None
                rows = torch.empty(H, W, dtype=torch.int32, device=self.device) if partner else None
                a = _lib.TrackRegisterColorArgs.new(H=H, W=W, max_iteration=int(max_iteration), fx=fx, fy=fy, cx=cx, cy=cy, depth_max=float(depth_max),
                                                    max_dist=self.trunc if max_dist is None else float(max_dist),
                                                    relative_fitness=float(relative_fitness), relative_rmse=float(relative_rmse),
                                                    color_weight=DEFAULT_COLOR_WEIGHT if color_weight is None else float(color_weight),
                                                    max_color_diff=float(max_color_diff), relative_color_rmse=float(relative_color_rmse),
                                                    model_depth=_lib.dptr(model.depth), model_normals=_lib.dptr(model.normals),
                                                    model_color=_lib.dptr(model.color), pose_ref=pose_ref.data_ptr(), live=depth.data_ptr(),
                                                    live_color=rgb.data_ptr(), pose_init=pose_init.data_ptr(), result=result.data_ptr(),
                                                    pose_out=pose.data_ptr(), partner=_lib.dptr(mates, torch.int32),
                                                    color_partner=_lib.dptr(rows, torch.int32), workspace=ws.data_ptr())
                _lib.check(lib.mipsf_track_register_color(C.byref(a), _lib.stream_ptr()), "track_register_color")
            return (result, pose, mates, rows) if partner else (result, pose)
        with torch.cuda.device(self.device):
            ws = torch.empty(int(lib.mipsf_track_workspace_bytes(_lib.TRACK_WS_REGISTER, H, W, 0)), dtype=torch.uint8, device=self.device)
            result = torch.empty(_lib.TRACK_RESULT_DOUBLES, dtype=torch.float64, device=self.device)
            pose = torch.empty(4, 4, dtype=torch.float32, device=self.device)
            mates = torch.empty(H, W, dtype=torch.int32, device=self.device) if partner else None
            a = _lib.TrackRegisterArgs.new(H=H, W=W, max_iteration=int(max_iteration), fx=fx, fy=fy, cx=cx, cy=cy, depth_max=float(depth_max),
                                           max_dist=self.trunc if max_dist is None else float(max_dist),
                                           relative_fitness=float(relative_fitness), relative_rmse=float(relative_rmse),
                                           model_depth=_lib.dptr(model.depth), model_normals=_lib.dptr(model.normals),
                                           pose_ref=pose_ref.data_ptr(), live=depth.data_ptr(), pose_init=pose_init.data_ptr(),
                                           result=result.data_ptr(), pose_out=pose.data_ptr(),
                                           partner=_lib.dptr(mates, torch.int32), workspace=ws.data_ptr())
            _lib.check(lib.mipsf_track_register(C.byref(a), _lib.stream_ptr()), "track_register")
        return (result, pose, mates) if partner else (result, pose)

    # ----------------------------------------------------------------------------------------------------------- public
    def raycast(self, c2w, K, H: int, W: int, near: float = 0.0, far: float = math.inf, step: Optional[float] = None,
                min_weight: float = 1.0, normals: bool = True, color: bool = False) -> Raycast:
        """The volume seen from ``c2w`` ([n,4,4] or [4,4], camera to world, OpenGL convention): z-depth (0 = no surface), world
        normals pointing into free space and colour per pixel, by marching every pixel's ray through the volume in steps of
        ``step`` metres (trunc/2 by default) to the first crossing from positive to non-positive tsdf among voxels of weight
        >= min_weight.  Device tensors; nothing is read back."""
        with torch.cuda.device(self.device):
            return self.raycast_enqueue(_poses(c2w, self.device), K, H, W, near, far, step, min_weight, normals, color)

    def track(self, depth, K, pose_init, pose_ref=None, model: Optional[Raycast] = None, max_dist: Optional[float] = None,
              max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, depth_max: float = math.inf,
              rgb=None, color_weight: Optional[float] = None, max_color_diff: float = math.inf, relative_color_rmse: float = 1e-6):
        """The pose of the depth frame ``depth`` [H,W] by point-to-plane ICP against the volume's ray cast from ``pose_ref`` (by
        default ``pose_init``; or against ``model``, a one-view Raycast made from pose_ref), starting at ``pose_init``.  Pairs are
        found by projecting the live points into the model image and kept within ``max_dist`` (trunc by default).  No pyramid:
        the capture range is a few centimetres and degrees.  One read-back.  -> TrackResult.
        With ``rgb`` [H,W,3], the frame's colour, and a volume made with color=True, every pair whose projection falls into a 2 x 2
        patch of model pixels also gives a photometric row -- the model's bilinear intensity against the live pixel's, weighted by
        ``color_weight`` (DEFAULT_COLOR_WEIGHT unless given) and kept while its residual is within ``max_color_diff`` -- which holds
        the pose where depth leaves it free: along a wall, along an edge.  -> ColorTrackResult."""
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")[0]
            P0 = _poses(pose_init, self.device)[0].contiguous()
            Pr = None if pose_ref is None else _poses(pose_ref, self.device)[0].contiguous()
            if rgb is None:
                result, pose = self.track_enqueue(D, K, P0, Pr, model, max_dist, max_iteration, relative_fitness, relative_rmse, depth_max)
            else:
                C3 = _images(rgb, self.device, 3, "rgb")
                if tuple(C3.shape) != (1,) + tuple(D.shape) + (3,):
                    raise ValueError(f"rgb: expected {tuple(D.shape) + (3,)}, got {tuple(C3.shape[1:]) if C3.shape[0] == 1 else tuple(C3.shape)}")
                result, pose = self.track_enqueue(D, K, P0, Pr, model, max_dist, max_iteration, relative_fitness, relative_rmse, depth_max,
                                                  rgb=C3[0], color_weight=color_weight, max_color_diff=max_color_diff,
                                                  relative_color_rmse=relative_color_rmse)
            got = torch.cat([pose.reshape(-1).to(torch.float64), result]).cpu()
        r = got[16:]
        head = (got[:16].reshape(4, 4).to(torch.float32), r[:16].reshape(4, 4).clone(), int(r[16]), float(r[17]), float(r[18]), int(r[19]))
        return TrackResult(*head) if rgb is None else ColorTrackResult(*head, int(r[20]), float(r[21]))

    def integrate(self, depth, c2w, K, rgb=None, depth_max: float = math.inf, views_per_call: Optional[int] = None) -> TSDFCounts:
        """Fuses the views in the order given.  depth [n,H,W] or [H,W] (0 = no measurement), c2w [n,4,4] or [4,4] (camera to world,
        the datasets' OpenGL convention), K a 3x3 matrix or (fx, fy, cx, cy), rgb [n,H,W,3] in a colour volume; host or device
        arrays, lists of them too.  The views are cut into calls of ``views_per_call`` (all in one by default); the cut does not
        reach the bytes.  One read-back of 16 bytes per call."""
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")
            P = _poses(c2w, self.device)
            C3 = None if rgb is None else _images(rgb, self.device, 3, "rgb")
            n = D.shape[0]
            if P.shape[0] != n:
                raise ValueError(f"{n} depth images and {P.shape[0]} poses")
            per = max(n, 1) if views_per_call is None else int(views_per_call)
            if per < 1:
                raise ValueError("views_per_call must be positive")
            records = [self.integrate_enqueue(D[k:k + per], P[k:k + per], K, None if C3 is None else C3[k:k + per], depth_max)
                       for k in range(0, max(n, 1), per)]
            got = torch.stack(records).cpu().numpy()
        return TSDFCounts(int(got[:, 0].sum()), int(got[-1, 1]))

    def deintegrate(self, depth, c2w, K, rgb=None, depth_max: float = math.inf, views_per_call: Optional[int] = None) -> RemoveCounts:
        """Takes the views out of the volume again, in the order given: the inverse of ``integrate`` for views that were fused with
        these very images, poses, K and depth_max (the pairs of a view are found by projecting again), in a volume made without
        ``max_weight``.  The same forms of arguments as ``integrate``; the cut into calls does not reach the bytes.  What remains is
        the mean of the remaining views up to the rounding of the steps; with every view removed, the all-zero
        state exactly.  A pose with a NaN removes nothing, as it fused nothing.  ``missing`` counts pairs that found no weight to
        take from: a sign that a view was not in the volume, not a proof that the others were.  One read-back of 32 bytes a call."""
        self._removable()
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")
            P = _poses(c2w, self.device)
            C3 = None if rgb is None else _images(rgb, self.device, 3, "rgb")
            n = D.shape[0]
            if P.shape[0] != n:
                raise ValueError(f"{n} depth images and {P.shape[0]} poses")
            per = max(n, 1) if views_per_call is None else int(views_per_call)
            if per < 1:
                raise ValueError("views_per_call must be positive")
            records = [self.deintegrate_enqueue(D[k:k + per], P[k:k + per], K, None if C3 is None else C3[k:k + per], depth_max)
                       for k in range(0, max(n, 1), per)]
            got = torch.stack(records).cpu().numpy()
        return RemoveCounts(int(got[:, 0].sum()), int(got[:, 1].sum()), int(got[:, 2].sum()), int(got[-1, 3]))

    def reintegrate(self, depth, c2w_old, c2w_new, K, rgb=None, depth_max: float = math.inf, min_translation: float = 0.0,
                    min_rotation: float = 0.0) -> ReintegrateCounts:
        """Moves fused views to new poses: the views whose pose moved are removed at ``c2w_old``, in ascending order, and then fused
        at ``c2w_new``, in ascending order -- two launches on one stream and one read-back, paid for the moved views only.  The
        step after a loop closure:

            poses_new = pose_graph.rebase(poses_world, submap_of_pose, anchors_old, anchors_new)
            vol.reintegrate(depth, poses_world, poses_new, K)

        ``depth``, ``rgb``, ``c2w_old``, K and depth_max are what the views were fused with (see ``deintegrate``).  Which views
        moved is decided on the host in float64, on the fp32 poses the kernels take (poses that lie on the device are copied over,
        64 bytes a view): a view moved when its translation changed by more than ``min_translation`` metres or its rotation by
        more than ``min_rotation`` radians; with both at 0, when any word of its pose differs.  With a threshold given, equal
        poses never count as moved, and a pose that is not finite (a lost frame) counts as moved when the other one is finite:
        its view is then fused, or removed, for the first time.  ``rebase`` moves the poses of a sub-map whose anchor stayed by
        a rounding (a few 1e-7 of their entries): thresholds of 1e-6 and more leave them alone.  Unmoved views are not touched
        and cost nothing; when no view moved neither kernel is launched and no word changes, and ``observed`` is counted from
        the weights (one pass over them and a read-back).  The
        volume then holds the fusion at the new poses up to the rounding of the steps: equal weights, tsdf within 2^-21 on the
        measured cases."""
        self._removable()
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")
            P0, P1 = _poses(c2w_old, self.device), _poses(c2w_new, self.device)
            C3 = None if rgb is None else _images(rgb, self.device, 3, "rgb")
            n = D.shape[0]
            if P0.shape[0] != n or P1.shape[0] != n:
                raise ValueError(f"{n} depth images, {P0.shape[0]} old poses and {P1.shape[0]} new poses")
            if (C3 is None) != (self.color is None):
                raise ValueError("rgb goes with a volume made with color=True, and such a volume needs rgb")
            moved = _moved_views(P0, P1, min_translation, min_rotation)
            if len(moved) == 0:
                seen = int(torch.count_nonzero(self.weight > 0))
                return ReintegrateCounts(0, RemoveCounts(0, 0, 0, seen), TSDFCounts(0, seen))
            if len(moved) < n:
                pick = torch.from_numpy(moved).to(self.device)
                D, P0, P1 = D[pick], P0[pick], P1[pick]
                C3 = None if C3 is None else C3[pick]
            got = torch.cat(self.reintegrate_enqueue(D, P0, P1, K, C3, depth_max)).cpu().numpy()
        return ReintegrateCounts(len(moved), RemoveCounts(*(int(x) for x in got[:4])), TSDFCounts(int(got[4]), int(got[5])))

    def volume(self, min_weight: float = 1.0) -> torch.Tensor:
        """the marching input: tsdf where weight >= min_weight, -inf (unobserved, off for the marcher) elsewhere"""
        return torch.where(self.weight >= float(min_weight), self.tsdf, torch.full_like(self.tsdf, -math.inf))

    def extract_mesh(self, min_weight: float = 1.0, mesh_savepath: str = "") -> Mesh:
        """marching_cubes(volume(min_weight), 0, truncation=1): saturated voxels (tsdf = 1) switch their cells off like unobserved
        ones.  -> Mesh with world vertices in float64 and per-vertex colours when colour was fused."""
        if min(self.dims) < 2:
            v, f = torch.zeros(0, 3, dtype=torch.float64, device=self.device), torch.zeros(0, 3, dtype=torch.int64, device=self.device)
        else:
            with torch.cuda.device(self.device):
                v, f = marching_cubes(self.volume(min_weight), 0.0, truncation=1.0, return_device=True)
        colors = None
        if self.color is not None:
            colors = self.sample_enqueue(v.contiguous()).cpu().numpy()
        vertices = self.origin + v.cpu().numpy() * self.voxel_size
        mesh = Mesh(vertices, f.cpu().numpy(), colors)
        if mesh_savepath:
            save_ply(mesh_savepath, mesh.vertices, mesh.faces, mesh.vertex_colors)
        return mesh


def frames_bounds(depth: torch.Tensor, poses: torch.Tensor, K, depth_max: float = math.inf) -> np.ndarray:
    """the box of the back-projected usable pixels (0 < d < inf, d <= depth_max) of device depth [n,H,W] -> float64 [3,2];
    float64 on the device, six numbers read back"""
    fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
    n, H, W = depth.shape
    dev = depth.device
    jj, ii = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    dirs = torch.stack([(ii - cx) / fx, -((jj - cy) / fy), -torch.ones_like(ii)], -1)                    # [H,W,3]
    lo = torch.full((3,), math.inf, dtype=torch.float64, device=dev)
    hi = -lo
    for k in range(0, n, 8):                                                                             # 8 views at a time: 55 MB at 460 x 620
        d = depth[k:k + 8].to(torch.float64)
        ok = ((d > 0) & (d < math.inf) & (d <= depth_max))[..., None]
        P = poses[k:k + 8].to(torch.float64)
        p = torch.einsum("vhwc,vdc->vhwd", dirs * d[..., None], P[:, :3, :3]) + P[:, None, None, :3, 3]
        big = torch.full_like(p, math.inf)
        lo = torch.minimum(lo, torch.where(ok, p, big).reshape(-1, 3).amin(0))
        hi = torch.maximum(hi, torch.where(ok, p, -big).reshape(-1, 3).amax(0))
    out = torch.stack([lo, hi], 1).cpu().numpy()
    if not np.all(np.isfinite(out)):
        raise ValueError("no pixel with a usable depth: give bounds")
    return out


def tsdf_mesh_from_frames(depth, c2w, K, voxel_size: float, trunc: Optional[float] = None, rgb=None, bounds=None,
                          depth_max: float = math.inf, min_weight: float = 1.0, mesh_savepath: str = "", device=None,
                          return_volume: bool = False):
    """Depth frames -> Mesh: a volume over ``bounds`` ([3,2], by default the box of the back-projected usable pixels padded by
    trunc) with ``voxel_size``, all views fused, marched.  ``trunc`` defaults to 4 voxels.  Device tensors are used where they
    lie; ``return_volume`` adds the TSDFVolume."""
    voxel_size = float(voxel_size)
    trunc = 4.0 * voxel_size if trunc is None else float(trunc)
    dev = depth.device if torch.is_tensor(depth) and depth.is_cuda else _device(device)
    with torch.cuda.device(dev):
        D = _images(depth, dev, 0, "depth")
        P = _poses(c2w, dev)
        C3 = None if rgb is None else _images(rgb, dev, 3, "rgb")
        if bounds is None:
            b = frames_bounds(D, P, K, depth_max)
            b[:, 0] -= trunc
            b[:, 1] += trunc
        else:
            b = np.asarray(bounds.detach().cpu() if torch.is_tensor(bounds) else bounds, np.float64).reshape(3, 2)
        counts = np.ceil((b[:, 1] - b[:, 0]) / voxel_size)
        if not (np.all(np.isfinite(counts)) and np.all(counts >= 0)):
            raise ValueError(f"bounds {b.tolist()} at voxel size {voxel_size}")
        dims = [int(c) + 1 for c in counts]
        if dims[0] * dims[1] * dims[2] > _lib.TSDF_MAX_VOXELS:
            raise ValueError(f"voxel size {voxel_size} over bounds {b.tolist()} gives a grid of {dims[0]} x {dims[1]} x {dims[2]}: 2^31 voxels "
                             f"or more; choose a larger voxel size")
        vol = TSDFVolume(b[:, 0], voxel_size, dims, trunc, color=C3 is not None, device=dev)
        vol.integrate(D, P, K, C3, depth_max)
        mesh = vol.extract_mesh(min_weight, mesh_savepath)
    return (mesh, vol) if return_volume else mesh


def tsdf_odometry(depth, K, first_pose, voxel_size: float, bounds, trunc: Optional[float] = None, rgb=None, min_correspondences: int = 0,
                  device=None, color_weight: Optional[float] = None, **track_kw):
    """Frame-to-model depth odometry, the classical baseline's tracker: frame 0 is fused at ``first_pose``; every later frame is
    registered (TSDFVolume.track_enqueue, ``track_kw`` to it) against the ray cast from the previous frame's pose, starting from
    that pose, and fused at the pose found.  The walk is enqueued whole, the poses handed on between the stages on the device;
    one read-back at the end.  A frame whose registration ends with fewer than ``min_correspondences`` pairs keeps its initial
    pose, is not fused (mipsf_tsdf_integrate gets a NaN pose, which updates nothing) and has ``lost`` set in its record.
    -> (poses fp32 [n,4,4] on the host, records, TSDFVolume); a record is a dict of transformation (float64 [4,4], the
    registration's pose before its rounding; zero for frame 0), n_correspondences, fitness, inlier_rmse, iterations and lost.
    Score the poses with ``trajectory_metrics(poses, gt_c2w)`` (aligned ATE); the first pose is given, so ``align=False``
    measures the drift itself.
    ``rgb`` [n,H,W,3] is fused with the depth; the registration uses it only when ``color_weight`` is given (TSDFVolume.track's
    colour term), and the records then also hold n_color and color_rmse."""
    if color_weight is not None and rgb is None:
        raise ValueError("color_weight: tracking with colour needs rgb")
    voxel_size = float(voxel_size)
    trunc = 4.0 * voxel_size if trunc is None else float(trunc)
    dev = depth.device if torch.is_tensor(depth) and depth.is_cuda else _device(device)
    b = np.asarray(bounds.detach().cpu() if torch.is_tensor(bounds) else bounds, np.float64).reshape(3, 2)
    dims = [int(c) + 1 for c in np.ceil((b[:, 1] - b[:, 0]) / voxel_size)]
    with torch.cuda.device(dev):
        D = _images(depth, dev, 0, "depth")
        C3 = None if rgb is None else _images(rgb, dev, 3, "rgb")
        n, H, W = D.shape
        if n < 1:
            raise ValueError("no frames")
        vol = TSDFVolume(b[:, 0], voxel_size, dims, trunc, color=C3 is not None, device=dev)
        poses = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
        words = _lib.TRACK_RESULT_DOUBLES if color_weight is None else _lib.TRACK_COLOR_RESULT_DOUBLES
        results = torch.zeros(n, words, dtype=torch.float64, device=dev)
        lost = torch.zeros(n, dtype=torch.bool, device=dev)
        poses[0] = _poses(first_pose, dev)[0]
        nan_pose = torch.full((4, 4), math.nan, dtype=torch.float32, device=dev)
        vol.integrate_enqueue(D[:1], poses[:1], K, None if C3 is None else C3[:1])
        for k in range(1, n):
            prev = poses[k - 1]
            if color_weight is None:
                result, pose = vol.track_enqueue(D[k], K, prev, **track_kw)
            else:
                result, pose = vol.track_enqueue(D[k], K, prev, rgb=C3[k], color_weight=color_weight, **track_kw)
            bad = result[16] < float(min_correspondences)
            poses[k] = torch.where(bad, prev, pose)
            results[k], lost[k] = result, bad
            vol.integrate_enqueue(D[k:k + 1], torch.where(bad, nan_pose, pose)[None], K, None if C3 is None else C3[k:k + 1])
        got = torch.cat([poses.reshape(n, 16).to(torch.float64), results, lost[:, None].to(torch.float64)], 1).cpu()
    records = [{"transformation": r[16:32].reshape(4, 4).clone(), "n_correspondences": int(r[32]), "fitness": float(r[33]),
                "inlier_rmse": float(r[34]), "iterations": int(r[35]), "lost": bool(r[-1])} for r in got]
    if color_weight is not None:
        for rec, r in zip(records, got):
            rec["n_color"], rec["color_rmse"] = int(r[36]), float(r[37])
    return got[:, :16].reshape(n, 4, 4).to(torch.float32), records, vol


@torch.no_grad()
def mesh_from_rendered_depth(model, rays_d_cam, poses_local, first_kf_c2w, H: int, W: int, K, voxel_size: float,
                             trunc: Optional[float] = None, color: bool = True, bounds=None, depth_max: float = math.inf,
                             min_weight: float = 1.0, mesh_savepath: str = "", ray_batch_size: int = 10000, return_volume: bool = False):
    """The rendered-depth meshing protocol: inference.render_full_img per local pose with no depth guidance, the images fused at
    first_kf_c2w @ pose_local, the volume marched.  No arithmetic of its own."""
    from .inference import render_full_img
    dev = model.embed_fn.params.device
    local = _poses(poses_local, dev)
    first = torch.as_tensor(np.asarray(first_kf_c2w) if not torch.is_tensor(first_kf_c2w) else first_kf_c2w).to(dev).to(torch.float32)
    images = [render_full_img(model, rays_d_cam, p, None, int(H), int(W), ray_batch_size) for p in local]
    depth = torch.stack([d for _, d in images]).to(torch.float32)
    rgb = torch.stack([c for c, _ in images]).to(torch.float32) if color else None
    return tsdf_mesh_from_frames(depth, first @ local, K, voxel_size, trunc, rgb, bounds, depth_max, min_weight, mesh_savepath,
                                 device=dev, return_volume=return_volume)
