"""The TSDF volume of ``tsdf.py`` kept only where a depth pixel put a surface: a virtual grid of bricks of 8 x 8 x 16 voxels that may
hold 2^31 voxels and more, an index grid with one word per brick, and a pool of ``capacity_bricks`` brick-sized slots.  A brick gets
a slot when a depth pixel of a fused view lands within ``band`` of it; only allocated bricks are fused, ray cast and gathered.  The
kernels are those of ``csrc/sparse.hip`` (C ABI: include/mipsf_sparse.h):

    SparseTSDFVolume               the state (index grid, pool of tsdf, weight, optionally colour; all on the device) and integrate /
                                   to_dense / extract_mesh / extract_mesh_bricks / raycast / track / reset; with ``history=True``
                                   also deintegrate / reintegrate, which take fused views out again and fuse them at new poses
                                   (``csrc/sparse_remove.hip``, include/mipsf_sparse_remove.h)
    sparse_tsdf_mesh_from_frames   depth frames + poses -> mesh.Mesh, the namesake of tsdf_mesh_from_frames
    sparse_tsdf_odometry           depth frames -> poses, the namesake of tsdf_odometry

Every output is the dense volume's rule read over the dense state with the voxels of unallocated bricks left at zero, and EQUALS the
float64 restatement in tests/sparse_cpu.py.  ``extract_mesh`` goes through ``to_dense``: a window of the grid as a TSDFVolume, below
2^31 voxels a marching call.  ``extract_mesh_bricks`` marches the allocated bricks themselves (csrc/sparse_mesh.hip,
include/mipsf_sparse_mesh.h): the whole volume in one call whatever the size of the virtual grid, and EQUALS
tests/sparse_mesh_cpu.py.  ``release`` gives slots back -- the bricks outside a box, or the bricks ``deintegrate`` emptied -- closes the
holes in place and can hand the released bricks to a ``BrickArchive``; ``restore`` brings an archive back (csrc/sparse_release.hip,
include/mipsf_sparse_release.h), and EQUALS tests/sparse_release_cpu.py.  Until ``release`` is called nothing is
freed.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .mesh import Mesh, filter_faces, save_ply
from .mesh_render import _poses
from .scene_mesh import _intrinsics
from .tsdf import Raycast, TSDFVolume, _device, _images, _moved_views, frames_bounds

BRICK = _lib.TSDF_BRICK


class SparseTSDFCounts(NamedTuple):
    updates: int                     # (voxel, view) pairs that updated, over the calls of one integrate()
    observed: int                    # voxels whose weight is positive afterwards
    marked: int                      # bricks the views marked, summed over the calls
    new: int                         # bricks that got a slot
    dropped: int                     # bricks that wanted a slot when the pool was full, summed over the calls
    bricks_in_use: int               # slots in use afterwards


class SparseRemoveCounts(NamedTuple):
    removed: int                     # (voxel, view) pairs taken out, over the calls of one deintegrate()
    missing: int                     # pairs the views hit whose voxel had no positive weight left (a diagnostic, not a guarantee)
    emptied: int                     # removals that brought a voxel back to the never-observed state
    observed: int                    # voxels whose weight is positive afterwards
    bricks_emptied: int              # slots in use without such a voxel afterwards (they keep their slots until release(empty=True))


class SparseReintegrateCounts(NamedTuple):
    views_moved: int                 # views removed at their old pose and fused at their new one
    removed: SparseRemoveCounts
    fused: SparseTSDFCounts
    view_ids: np.ndarray             # int64 [n]: the ids the views have now, new for the moved ones


class ReleaseCounts(NamedTuple):
    candidates: int                  # slots in use for which an enabled predicate held
    released: int                    # of those, slots given back
    released_outside: int            # released slots whose brick lay outside the box
    released_empty: int              # released slots without a voxel of positive weight (a slot may count in both)
    deferred: int                    # candidates the archive had no room for: they stay in the volume
    moved: int                       # slots moved to close the holes
    bricks_in_use: int               # slots in use afterwards


class RestoreCounts(NamedTuple):
    listed: int                      # entries of the archive
    invalid: int                     # entries whose brick is not a brick of the grid (the unwritten entries of an archive hold -1)
    duplicates: int                  # valid entries that lost their brick to an entry with a lower index
    occupied: int                    # bricks listed that have a slot already: they keep their words
    restored: int                    # bricks that got a slot and their entry's words
    dropped: int                     # bricks that got none: the pool was full
    bricks_in_use: int               # slots in use afterwards


class BrickArchive:
    """Bricks taken out of a SparseTSDFVolume by ``release``: per entry the brick (its linear index in the volume's brick grid; -1
    in an entry nothing was written to), ``born`` when the volume keeps a history, and all the words of the slot.  ``n`` is the count
    of entries written, None while it has not been read back (``release_enqueue``); the tensors may live on the device or, after
    ``cpu()``, on the host."""

    def __init__(self, bricks, born, tsdf, weight, color, n=None):
        self.bricks, self.born, self.tsdf, self.weight, self.color, self.n = bricks, born, tsdf, weight, color, n

    @staticmethod
    def empty(capacity: int, color: bool, history: bool, device) -> "BrickArchive":
        capacity = int(capacity)
        return BrickArchive(torch.full((capacity,), -1, dtype=torch.int32, device=device),
                            torch.full((capacity,), -1, dtype=torch.int32, device=device) if history else None,
                            torch.zeros((capacity,) + BRICK, dtype=torch.float32, device=device),
                            torch.zeros((capacity,) + BRICK, dtype=torch.float32, device=device),
                            torch.zeros((capacity,) + BRICK + (3,), dtype=torch.float32, device=device) if color else None)

    def __len__(self) -> int:
        return int(self.bricks.shape[0])

    def _each(self, f, n=None) -> "BrickArchive":
        return BrickArchive(*(None if t is None else f(t) for t in (self.bricks, self.born, self.tsdf, self.weight, self.color)),
                            n=self.n if n is None else n)

    def first(self, n: int) -> "BrickArchive":
        """the first n entries (views of the same storage), as the entries written"""
        n = int(n)
        return self._each(lambda t: t[:n], n=n)

    def cpu(self) -> "BrickArchive":
        return self._each(lambda t: t.cpu())

    def to(self, device) -> "BrickArchive":
        return self._each(lambda t: t.to(device))

    @staticmethod
    def cat(archives) -> "BrickArchive":
        """the entries of several archives in the order given (``restore`` lets the first of two entries of a brick win)"""
        archives = list(archives)
        if not archives:
            raise ValueError("cat: no archives")
        a0 = archives[0]
        if any((a.born is None) != (a0.born is None) or (a.color is None) != (a0.color is None) for a in archives):
            raise ValueError("cat: archives with and without born, or with and without color")
        known = all(a.n is not None for a in archives)
        parts = [a.first(a.n) if a.n is not None else a for a in archives]
        return BrickArchive(*(None if getattr(a0, k) is None else torch.cat([getattr(a, k) for a in parts]) for k in ("bricks", "born", "tsdf", "weight", "color")),
                            n=sum(a.n for a in archives) if known else None)


class SparseTSDFVolume:
    """A brick-sparse TSDF volume on the device.  Voxel (i,j,k) of the virtual grid ``dims`` sits at origin + voxel_size * (i,j,k);
    ``trunc``, ``max_weight`` and the words are those of TSDFVolume.  ``capacity_bricks`` slots of 1024 voxels are allocated at once
    (8 KB a slot, 20 KB with colour); ``band`` (trunc by default) is how far in front of and behind a depth pixel bricks are
    allocated.  With ``history`` the volume also keeps, per slot, the id of the first view the slot took (``born``; the id of a
    view is the count of views handed to integrate_enqueue before it, ``views_fused`` on the host and ``serial`` on the device), which
    is what ``deintegrate`` and ``reintegrate`` need; without it nothing of the volume or its launches changes."""

    def __init__(self, origin, voxel_size: float, dims, trunc: float, capacity_bricks: int, color: bool = False, max_weight: float = math.inf,
                 band: Optional[float] = None, device=None, history: bool = False):
        self.origin = np.asarray(origin, np.float64).reshape(3).copy()
        self.voxel_size, self.trunc, self.max_weight = float(voxel_size), float(trunc), float(max_weight)
        self.band = self.trunc if band is None else float(band)
        self.dims = tuple(int(d) for d in dims)
        self.capacity = int(capacity_bricks)
        if len(self.dims) != 3 or min(self.dims) < 1 or max(self.dims) >= 1 << 32:
            raise ValueError(f"dims: expected three positive counts, got {dims}")
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size)):
            raise ValueError(f"voxel_size {voxel_size} is not positive and finite")
        if not (self.band >= 0 and math.isfinite(self.band)):
            raise ValueError(f"band {band} is negative, infinite or not a number")
        self.bricks = tuple(-(-d // b) for d, b in zip(self.dims, BRICK))
        if self.bricks[0] * self.bricks[1] * self.bricks[2] > _lib.SPARSE_MAX_BRICKS:
            raise ValueError(f"a grid of {self.dims[0]} x {self.dims[1]} x {self.dims[2]} voxels has 2^31 bricks or more; choose a larger "
                             f"voxel size or smaller bounds")
        if not 1 <= self.capacity <= _lib.SPARSE_MAX_CAPACITY:
            raise ValueError(f"capacity_bricks {capacity_bricks}: from 1 to {_lib.SPARSE_MAX_CAPACITY}")
        self.steps = int(math.ceil(self.band / self.voxel_size))
        self.device = _device(device)
        self.ticks = tuple(self.origin[a] + self.voxel_size * np.arange(self.dims[a], dtype=np.float64) for a in range(3))
        self.history, self.views_fused, self.last_view_ids = bool(history), 0, np.zeros(0, np.int64)
        self.born = self.serial = None
        self.bricks_in_use: Optional[int] = 0       # the host's mirror of `count`: what the last read-back saw; None after an enqueue-only call
        self._release_scratch = None
        lib = _lib.lib()
        with torch.cuda.device(self.device):
            dev = self.device
            self._ticks_dev = tuple(torch.from_numpy(t).to(dev) for t in self.ticks)
            self.table = torch.full(self.bricks, -1, dtype=torch.int32, device=dev)
            self.slot_brick = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
            self.count = torch.zeros(1, dtype=torch.int32, device=dev)
            self.tsdf = torch.zeros((self.capacity,) + BRICK, dtype=torch.float32, device=dev)
            self.weight = torch.zeros((self.capacity,) + BRICK, dtype=torch.float32, device=dev)
            self.color = torch.zeros((self.capacity,) + BRICK + (3,), dtype=torch.float32, device=dev) if color else None
            self._birth = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
            self._mark = torch.empty(self.bricks, dtype=torch.int32, device=dev)
            self._scan = torch.empty(int(lib.mipsf_sparse_scan_words(*self.dims)), dtype=torch.int32, device=dev)
            if self.history:                 # uint32 words: -1 is MIPSF_SPARSE_UNBORN
                self.born = torch.full((self.capacity,), -1, dtype=torch.int32, device=dev)
                self.serial = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bind()

    def _bind(self) -> None:
        """the volume as the C ABI takes it (mipsf_sparse_volume), from the tensors as they are now"""
        g = _lib.SparseVolume()
        g.X, g.Y, g.Z, g.capacity, g.voxel = self.dims[0], self.dims[1], self.dims[2], self.capacity, self.voxel_size
        with torch.cuda.device(self.device):
            for d in range(3):
                g.origin[d] = float(self.origin[d])
                g.ticks[d] = _lib.dptr(self._ticks_dev[d], torch.float64)
            g.table, g.slot_brick = _lib.dptr(self.table, torch.int32), _lib.dptr(self.slot_brick, torch.int32)
            g.birth, g.count = _lib.dptr(self._birth, torch.int32), _lib.dptr(self.count, torch.int32)
            g.tsdf, g.weight, g.color = _lib.dptr(self.tsdf), _lib.dptr(self.weight), _lib.dptr(self.color)
        self._vol = g

    def reset(self) -> None:
        self.table.fill_(-1)
        self.count.zero_()
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()
        if self.history:
            self.born.fill_(-1)
            self.serial.zero_()
        self.views_fused, self.last_view_ids, self.bricks_in_use = 0, np.zeros(0, np.int64), 0

    def sync_views(self) -> int:
        """Reads the device's count of fused views into ``views_fused`` (one read-back of 4 bytes): for callers that replay a captured
        integrate_enqueue, which moves the device's word and not the host's -> views_fused"""
        self._historied()
        self.views_fused = int(self.serial.item()) & 0xFFFFFFFF
        return self.views_fused

    # ----------------------------------------------------------------------------------------------------------- enqueue only
    def _views(self, depth, poses, rgb):
        _lib.dptr(depth), _lib.dptr(poses), _lib.dptr(rgb)
        if depth.dim() != 3 or tuple(poses.shape) != (depth.shape[0], 4, 4):
            raise ValueError(f"expected depth [n,H,W] and poses [n,4,4], got {tuple(depth.shape)} and {tuple(poses.shape)}")
        if rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"rgb: expected {tuple(depth.shape) + (3,)}, got {tuple(rgb.shape)}")
        if (rgb is None) != (self.color is None):
            raise ValueError("rgb goes with a volume made with color=True, and such a volume needs rgb")

    def allocate_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, depth_max: float = math.inf,
                         record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mipsf_sparse_allocate; nothing is read back -> record int64 [4] on the device: bricks marked, new, dropped, in use"""
        _lib.dptr(depth), _lib.dptr(poses)
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = depth.shape
        with torch.cuda.device(self.device):
            record = torch.empty(_lib.SPARSE_ALLOC_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            a = _lib.SparseAllocateArgs.new(n=n, H=H, W=W, steps=self.steps, fx=fx, fy=fy, cx=cx, cy=cy, depth_max=float(depth_max), band=self.band,
                                            vol=self._vol, depth=depth.data_ptr() if n else None, poses=poses.data_ptr() if n else None,
                                            mark=self._mark.data_ptr(), scan=self._scan.data_ptr(), record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_allocate(C.byref(a), _lib.stream_ptr()), "sparse_allocate")
        self.bricks_in_use = None
        return record

    def fuse_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, rgb: Optional[torch.Tensor] = None, depth_max: float = math.inf,
                     record: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
        """mipsf_sparse_integrate over the slots in use, with the births the last allocate_enqueue left; nothing is read back
        -> record int64 [2] on the device"""
        self._views(depth, poses, rgb)
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = depth.shape
        with torch.cuda.device(self.device):
            record = torch.empty(_lib.TSDF_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            a = _lib.SparseIntegrateArgs.new(n=n, H=H, W=W, flags=int(flags), fx=fx, fy=fy, cx=cx, cy=cy, trunc=self.trunc,
                                             depth_max=float(depth_max), max_weight=self.max_weight, vol=self._vol,
                                             depth=depth.data_ptr() if n else None, rgb=None if rgb is None or not n else rgb.data_ptr(),
                                             poses=poses.data_ptr() if n else None, record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_integrate(C.byref(a), _lib.stream_ptr()), "sparse_integrate")
        return record

    def integrate_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, rgb: Optional[torch.Tensor] = None,
                          depth_max: float = math.inf, flags: int = 0):
        """Allocates for the views, then fuses them; nothing is read back.  depth fp32 [n,H,W], poses fp32 [n,4,4], rgb fp32
        [n,H,W,3] or None, all on the device -> (record int64 [2]: pairs updated, voxels observed; record int64 [4]: bricks marked,
        new, dropped, in use), both on the device"""
        self._views(depth, poses, rgb)
        if not self.history:
            alloc = self.allocate_enqueue(depth, poses, K, depth_max)
            return self.fuse_enqueue(depth, poses, K, rgb, depth_max, flags=flags), alloc
        n = depth.shape[0]
        if self.views_fused + n > _lib.SPARSE_MAX_VIEW_ID:
            raise ValueError(f"{n} views after {self.views_fused}: view ids end at {_lib.SPARSE_MAX_VIEW_ID}")
        alloc = self.allocate_enqueue(depth, poses, K, depth_max)
        self.stamp_enqueue(n)
        return self.fuse_enqueue(depth, poses, K, rgb, depth_max, flags=flags), alloc

    def stamp_enqueue(self, n: int) -> None:
        """mipsf_sparse_stamp between allocate_enqueue and fuse_enqueue of the same ``n`` views: the slots that take their first view
        get its id, the device's ``serial`` and the host's ``views_fused`` move on by n, and ``last_view_ids`` holds the ids of the n
        views; nothing is read back"""
        self._historied()
        with torch.cuda.device(self.device):
            a = _lib.SparseStampArgs.new(n=int(n), vol=self._vol, born=_lib.dptr(self.born, torch.int32), serial=_lib.dptr(self.serial, torch.int32))
            _lib.check(_lib.lib().mipsf_sparse_stamp(C.byref(a), _lib.stream_ptr()), "sparse_stamp")
        self.last_view_ids = self.views_fused + np.arange(int(n), dtype=np.int64)
        self.views_fused += int(n)

    def _historied(self) -> None:
        if not self.history:
            raise ValueError("history: the volume was made with history=False and does not know which views a brick holds; make it with history=True")

    def _removable(self) -> None:
        self._historied()
        if math.isfinite(self.max_weight):
            raise ValueError(f"views cannot be removed from a volume made with max_weight {self.max_weight}: a capped running mean is a "
                             f"moving average, which has no inverse; make the volume with max_weight=inf")

    def deintegrate_enqueue(self, depth: torch.Tensor, poses: torch.Tensor, K, view_ids: torch.Tensor, rgb: Optional[torch.Tensor] = None,
                            depth_max: float = math.inf, record: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
        """One call of mipsf_sparse_deintegrate, the inverse of integrate_enqueue for views fused with these very arguments under
        the ids ``view_ids`` (int32 or uint32 [n], the words of the unsigned ids, on the device); nothing is read back and nothing is
        freed -> record int64 [5] on the device: pairs removed, pairs missing, voxels emptied, voxels with a positive weight, slots in
        use without one"""
        self._removable()
        self._views(depth, poses, rgb)
        n, H, W = depth.shape
        if not torch.is_tensor(view_ids) or view_ids.dtype not in (torch.int32, torch.uint32) or tuple(view_ids.shape) != (n,):
            raise ValueError(f"view_ids: expected an int32 or uint32 tensor [{n}] on the device, got "
                             f"{(view_ids.dtype, tuple(view_ids.shape)) if torch.is_tensor(view_ids) else type(view_ids).__name__}")
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        with torch.cuda.device(self.device):
            record = torch.empty(_lib.SPARSE_REMOVE_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            a = _lib.SparseDeintegrateArgs.new(n=n, H=H, W=W, flags=int(flags), fx=fx, fy=fy, cx=cx, cy=cy, trunc=self.trunc, depth_max=float(depth_max),
                                               vol=self._vol, depth=depth.data_ptr() if n else None,
                                               rgb=None if rgb is None or not n else rgb.data_ptr(), poses=poses.data_ptr() if n else None,
                                               view_ids=_lib.dptr(view_ids, view_ids.dtype) if n else None,
                                               born=_lib.dptr(self.born, torch.int32), record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_deintegrate(C.byref(a), _lib.stream_ptr()), "sparse_deintegrate")
        return record

    def reintegrate_enqueue(self, depth: torch.Tensor, poses_old: torch.Tensor, poses_new: torch.Tensor, K, view_ids: torch.Tensor,
                            rgb: Optional[torch.Tensor] = None, depth_max: float = math.inf, flags: int = 0):
        """deintegrate_enqueue at ``poses_old`` under ``view_ids``, then integrate_enqueue at ``poses_new``, of every view given: no
        selection and nothing read back.  The views get fresh ids (``last_view_ids``) -> (remove record int64 [5], fuse record
        int64 [2], allocation record int64 [4]), on the device"""
        self._removable()
        if tuple(poses_new.shape) != tuple(poses_old.shape):
            raise ValueError(f"poses: {tuple(poses_old.shape)} old and {tuple(poses_new.shape)} new")
        gone = self.deintegrate_enqueue(depth, poses_old, K, view_ids, rgb, depth_max, flags=flags)
        fused, alloc = self.integrate_enqueue(depth, poses_new, K, rgb, depth_max, flags=flags)
        return gone, fused, alloc

    def gather_enqueue(self, lo, hi) -> TSDFVolume:
        """mipsf_sparse_gather: the window lo <= index < hi as a TSDFVolume; nothing is read back"""
        lo, hi = tuple(int(x) for x in lo), tuple(int(x) for x in hi)
        if len(lo) != 3 or len(hi) != 3 or any(not 0 <= a < b <= d for a, b, d in zip(lo, hi, self.dims)):
            raise ValueError(f"window {lo} .. {hi} of a grid of {self.dims}")
        n = tuple(b - a for a, b in zip(lo, hi))
        if n[0] * n[1] * n[2] > _lib.TSDF_MAX_VOXELS:
            raise ValueError(f"a window of {n[0]} x {n[1]} x {n[2]} voxels has 2^31 voxels or more; take it in parts (to_dense(lo, hi))")
        out = TSDFVolume(self.origin + self.voxel_size * np.asarray(lo, np.float64), self.voxel_size, n, self.trunc, self.color is not None,
                         self.max_weight, self.device)
        # the window's voxels keep the positions they have in the virtual grid, to the last bit
        out.ticks = tuple(self.ticks[d][lo[d]:hi[d]] for d in range(3))
        out._ticks_dev = tuple(self._ticks_dev[d][lo[d]:hi[d]] for d in range(3))
        with torch.cuda.device(self.device):
            a = _lib.SparseGatherArgs.new(vol=self._vol, tsdf=_lib.dptr(out.tsdf), weight=_lib.dptr(out.weight), color=_lib.dptr(out.color))
            for d in range(3):
                a.lo[d], a.hi[d] = lo[d], hi[d]
            _lib.check(_lib.lib().mipsf_sparse_gather(C.byref(a), _lib.stream_ptr()), "sparse_gather")
        return out

    def raycast_enqueue(self, poses: torch.Tensor, K, H: int, W: int, near: float = 0.0, far: float = math.inf, step: Optional[float] = None,
                        min_weight: float = 1.0, normals: bool = True, color: bool = False, flags: int = 0) -> Raycast:
        """mipsf_sparse_raycast; nothing is read back.  poses fp32 [n,4,4] on the device -> Raycast of device tensors"""
        _lib.dptr(poses)
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
            raise ValueError(f"poses: expected [n,4,4], got {tuple(poses.shape)}")
        if color and self.color is None:
            raise ValueError("the volume was made without colour")
        fx, fy, cx, cy = (float(x) for x in _intrinsics(K))
        n, H, W = poses.shape[0], int(H), int(W)
        with torch.cuda.device(self.device):
            depth = torch.empty(n, H, W, dtype=torch.float32, device=self.device)
            nrm = torch.empty(n, H, W, 3, dtype=torch.float32, device=self.device) if normals else None
            col = torch.empty(n, H, W, 3, dtype=torch.float32, device=self.device) if color else None
            record = torch.empty(_lib.TRACK_RECORD_WORDS, dtype=torch.int64, device=self.device)
            a = _lib.SparseRaycastArgs.new(n=n, H=H, W=W, flags=int(flags), trunc=self.trunc, fx=fx, fy=fy, cx=cx, cy=cy, near=float(near),
                                           far=float(far), step=0.5 * self.trunc if step is None else float(step), min_weight=float(min_weight),
                                           vol=self._vol, poses=poses.data_ptr() if n else None, depth=depth.data_ptr() if n else None,
                                           normals=nrm.data_ptr() if normals and n else None,
                                           color_out=col.data_ptr() if color and n else None, record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_raycast(C.byref(a), _lib.stream_ptr()), "sparse_raycast")
        return Raycast(depth, nrm, col, record)

    # the registration takes any ray-cast images: TSDFVolume's two methods run as they are, on this volume's raycast_enqueue
    track_enqueue = TSDFVolume.track_enqueue
    track = TSDFVolume.track

    # ----------------------------------------------------------------------------------------------------------- public
    def integrate(self, depth, c2w, K, rgb=None, depth_max: float = math.inf, views_per_call: Optional[int] = None) -> SparseTSDFCounts:
        """Allocates bricks for the views and fuses them in the order given; the arguments are those of TSDFVolume.integrate.  The
        views are cut into calls of ``views_per_call`` (all in one by default, at most 65535); while nothing is dropped the cut does
        not reach the bytes of any brick, only the numbering of the slots.  One read-back of 48 bytes per call."""
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")
            P = _poses(c2w, self.device)
            C3 = None if rgb is None else _images(rgb, self.device, 3, "rgb")
            n = D.shape[0]
            if P.shape[0] != n:
                raise ValueError(f"{n} depth images and {P.shape[0]} poses")
            per = min(max(n, 1), _lib.SPARSE_MAX_VIEWS) if views_per_call is None else int(views_per_call)
            if per < 1:
                raise ValueError("views_per_call must be positive")
            records = [torch.cat(self.integrate_enqueue(D[k:k + per], P[k:k + per], K, None if C3 is None else C3[k:k + per], depth_max))
                       for k in range(0, max(n, 1), per)]
            got = torch.stack(records).cpu().numpy()
        if self.history:
            self.last_view_ids = self.views_fused - n + np.arange(n, dtype=np.int64)
        self.bricks_in_use = int(got[-1, 5])
        return SparseTSDFCounts(int(got[:, 0].sum()), int(got[-1, 1]), int(got[:, 2].sum()), int(got[:, 3].sum()), int(got[:, 4].sum()),
                                int(got[-1, 5]))

    def _ids(self, view_ids, n: int) -> np.ndarray:
        """view ids as the caller has them (a list, an array, a tensor) -> int64 [n] on the host, each the id of a fused view"""
        ids = np.asarray(view_ids.detach().cpu() if torch.is_tensor(view_ids) else view_ids).reshape(-1)
        if len(ids) != n or (n and ids.dtype.kind not in "iu"):
            raise ValueError(f"view_ids: expected {n} integer ids, one a view, got {len(ids)} of type {ids.dtype}")
        ids = ids.astype(np.int64)
        if n and (ids.min() < 0 or ids.max() >= self.views_fused):
            raise ValueError(f"view_ids: ids from {int(ids.min())} to {int(ids.max())}, but the volume has fused views 0 .. {self.views_fused - 1} only")
        return ids

    def _ids_dev(self, ids: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(self.device)

    def deintegrate(self, depth, c2w, K, view_ids, rgb=None, depth_max: float = math.inf, views_per_call: Optional[int] = None) -> SparseRemoveCounts:
        """Takes the views out of the volume again, in the order given: the inverse of ``integrate`` for views that were fused with
        these very images, poses, K and depth_max under the ids ``view_ids`` (``last_view_ids`` after their ``integrate``), in a
        volume made with ``history=True`` and without ``max_weight``.  A brick gives up the views it took -- those with an id from
        its ``born`` on -- and no others.  The same forms of arguments as ``integrate``; the cut into calls does not reach the bytes.
        What remains is the mean of the remaining views up to the rounding of the steps; with every view removed,
        the all-zero words exactly.  Nothing is freed here: an emptied brick keeps its slot (``bricks_emptied``) until
        ``release(empty=True)`` gives it back.  One read-back."""
        self._removable()
        with torch.cuda.device(self.device):
            D = _images(depth, self.device, 0, "depth")
            P = _poses(c2w, self.device)
            C3 = None if rgb is None else _images(rgb, self.device, 3, "rgb")
            n = D.shape[0]
            if P.shape[0] != n:
                raise ValueError(f"{n} depth images and {P.shape[0]} poses")
            ids = self._ids_dev(self._ids(view_ids, n))
            per = min(max(n, 1), _lib.SPARSE_MAX_VIEWS) if views_per_call is None else int(views_per_call)
            if per < 1:
                raise ValueError("views_per_call must be positive")
            records = [self.deintegrate_enqueue(D[k:k + per], P[k:k + per], K, ids[k:k + per], None if C3 is None else C3[k:k + per], depth_max)
                       for k in range(0, max(n, 1), per)]
            got = torch.stack(records).cpu().numpy()
        return SparseRemoveCounts(int(got[:, 0].sum()), int(got[:, 1].sum()), int(got[:, 2].sum()), int(got[-1, 3]), int(got[-1, 4]))

    def reintegrate(self, depth, c2w_old, c2w_new, K, view_ids, rgb=None, depth_max: float = math.inf, min_translation: float = 0.0,
                    min_rotation: float = 0.0) -> SparseReintegrateCounts:
        """Moves fused views to new poses, as TSDFVolume.reintegrate does and with its selection of the moved views (on the host, in
        float64: translation above ``min_translation`` or rotation above ``min_rotation``; with both at 0 any differing word): the
        moved views are removed at ``c2w_old`` under their ``view_ids``, bricks are allocated for them at ``c2w_new`` and they are
        fused there, under fresh ids.  The step after a loop closure:

            poses_new = pose_graph.rebase(poses_world, submap_of_pose, anchors_old, anchors_new)
            ids = vol.reintegrate(depth, poses_world, poses_new, K, ids).view_ids

        It costs the moved views only, and one read-back; when no view moved nothing is launched and no word changes (the counts
        then come from one pass over the weights)."""
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
            ids = self._ids(view_ids, n)
            moved = _moved_views(P0, P1, min_translation, min_rotation)
            if len(moved) == 0:
                live = (self.weight.view(self.capacity, -1) > 0)
                seen, full, used = (int(x) for x in torch.stack([live.sum(), live.any(1).sum(), self.count[0].to(torch.int64)]).tolist())
                used = min(used, self.capacity)
                return SparseReintegrateCounts(0, SparseRemoveCounts(0, 0, 0, seen, used - full), SparseTSDFCounts(0, seen, 0, 0, 0, used), ids)
            if len(moved) > _lib.SPARSE_MAX_VIEWS:
                raise ValueError(f"{len(moved)} views moved, at most {_lib.SPARSE_MAX_VIEWS} a call: reintegrate them in parts")
            if len(moved) < n:
                pick = torch.from_numpy(moved).to(self.device)
                D, P0, P1 = D[pick], P0[pick], P1[pick]
                C3 = None if C3 is None else C3[pick]
            got = torch.cat(self.reintegrate_enqueue(D, P0, P1, K, self._ids_dev(ids[moved]), C3, depth_max)).cpu().numpy()
            ids = ids.copy()
            ids[moved] = self.last_view_ids
            self.bricks_in_use = int(got[10])
        return SparseReintegrateCounts(len(moved), SparseRemoveCounts(*(int(x) for x in got[:5])),
                                       SparseTSDFCounts(int(got[5]), int(got[6]), int(got[7]), int(got[8]), int(got[9]), int(got[10])), ids)

    # ----------------------------------------------------------------------------------------------------------- release, restore
    def release_enqueue(self, box: Optional[torch.Tensor] = None, empty: bool = False, archive_capacity: Optional[int] = None,
                        record: Optional[torch.Tensor] = None, into: Optional["BrickArchive"] = None):
        """mipsf_sparse_release; nothing is read back.  ``box``: float64 [6] on the device, lo[3] then hi[3] in world metres: the bricks
        whose voxel centres all lie outside it are released (a NaN releases nothing); ``empty``: the slots without a voxel of positive
        weight are.  With ``archive_capacity`` the released bricks go to a BrickArchive of that many entries and no more are released
        than it holds (``into``: a BrickArchive of the caller's to write to, for a captured graph that is replayed; its entries are the
        capacity) -> record int64 [7] on the device (ReleaseCounts' fields), or (record, BrickArchive)"""
        flags = (_lib.SPARSE_RELEASE_OUTSIDE if box is not None else 0) | (_lib.SPARSE_RELEASE_EMPTY if empty else 0)
        if not flags:
            raise ValueError("release: give a box, or empty=True, or both")
        if box is not None and (not torch.is_tensor(box) or box.dtype != torch.float64 or box.numel() != 6):
            raise ValueError("box: expected a float64 tensor of 6 values on the device, lo[3] then hi[3]")
        arch = None
        with torch.cuda.device(self.device):
            if into is not None:
                if (into.born is None) != (not self.history) or (into.color is None) != (self.color is None):
                    raise ValueError("into: the archive's born and color must be there exactly when the volume has history and colour")
                if archive_capacity is not None and int(archive_capacity) != len(into):
                    raise ValueError(f"archive_capacity {archive_capacity} with an archive of {len(into)} entries")
                flags |= _lib.SPARSE_RELEASE_ARCHIVE
                arch = into
            elif archive_capacity is not None:
                if not 0 <= int(archive_capacity) <= _lib.SPARSE_MAX_CAPACITY:
                    raise ValueError(f"archive_capacity {archive_capacity}: from 0 to {_lib.SPARSE_MAX_CAPACITY}")
                flags |= _lib.SPARSE_RELEASE_ARCHIVE
                arch = BrickArchive.empty(int(archive_capacity), self.color is not None, self.history, self.device)
            if self._release_scratch is None:
                self._release_scratch = torch.empty(int(_lib.lib().mipsf_sparse_release_scratch_words(self.capacity)) // 2 + 1, dtype=torch.int64,
                                                    device=self.device)
            record = torch.empty(_lib.SPARSE_RELEASE_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            some = arch is not None and len(arch) > 0
            a = _lib.SparseReleaseArgs.new(flags=flags, archive_capacity=len(arch) if arch is not None else 0, vol=self._vol,
                                           born=_lib.dptr(self.born, torch.int32), box=None if box is None else _lib.dptr(box.contiguous(), torch.float64),
                                           arch_brick=_lib.dptr(arch.bricks, torch.int32) if some else None,
                                           arch_born=_lib.dptr(arch.born, torch.int32) if some else None,
                                           arch_tsdf=_lib.dptr(arch.tsdf) if some else None, arch_weight=_lib.dptr(arch.weight) if some else None,
                                           arch_color=_lib.dptr(arch.color) if some else None,
                                           scratch=_lib.dptr(self._release_scratch, torch.int64), record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_release(C.byref(a), _lib.stream_ptr()), "sparse_release")
        self.bricks_in_use = None
        return record if arch is None else (record, arch)

    def _box(self, keep_box) -> torch.Tensor:
        """a [3,2] array of (lo, hi) per axis, or a tensor of 6 float64 (lo[3], hi[3]) -> float64 [6] on the device"""
        if torch.is_tensor(keep_box) and keep_box.is_cuda and keep_box.dtype == torch.float64 and keep_box.numel() == 6:
            return keep_box.reshape(6).contiguous()
        b = np.asarray(keep_box.detach().cpu() if torch.is_tensor(keep_box) else keep_box, np.float64)
        if b.shape == (6,):
            return torch.from_numpy(b.copy()).to(self.device)
        if b.shape != (3, 2):
            raise ValueError(f"keep_box: expected [3,2] (lo and hi per axis) or 6 float64 (lo[3], hi[3]), got {b.shape}")
        return torch.from_numpy(np.concatenate([b[:, 0], b[:, 1]])).to(self.device)

    def release(self, keep_box=None, empty: bool = False, archive: bool = False):
        """Gives slots back: the bricks that lie wholly outside ``keep_box`` ([3,2] world metres, or a device tensor of 6 float64)
        and, with ``empty``, the slots ``deintegrate`` left without an observed voxel (its ``bricks_emptied``).  The holes are closed
        in place, so the slots in use stay 0 .. bricks_in_use - 1 (the numbering of the slots changes, nothing else of the survivors).
        With ``archive`` the released bricks are returned as a BrickArchive, which ``restore`` takes.  One read-back.
        -> ReleaseCounts, or (ReleaseCounts, BrickArchive)"""
        with torch.cuda.device(self.device):
            box = None if keep_box is None else self._box(keep_box)
            cap = (self.capacity if self.bricks_in_use is None else self.bricks_in_use) if archive else None
            got = self.release_enqueue(box, empty, cap)
            rec, arch = got if archive else (got, None)
            counts = ReleaseCounts(*(int(x) for x in rec.tolist()))
        self.bricks_in_use = counts.bricks_in_use
        return (counts, arch.first(counts.released)) if archive else counts

    def restore_enqueue(self, archive: BrickArchive, record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mipsf_sparse_restore of the archive's entries (its first ``n`` when that is known); nothing is read back.  The bricks get
        slots behind the ones in use, in ascending brick index, and their words; a brick that has a slot keeps what it holds
        -> record int64 [7] on the device (RestoreCounts' fields)"""
        if not isinstance(archive, BrickArchive):
            raise ValueError(f"restore: expected a BrickArchive, got {type(archive).__name__}")
        if (archive.born is None) != (not self.history):
            raise ValueError("restore: an archive with born goes with a volume made with history=True, one without with history=False")
        if (archive.color is None) != (self.color is None):
            raise ValueError("restore: an archive with color goes with a volume made with color=True, one without with color=False")
        arch = archive if archive.n is None else archive.first(archive.n)
        m = len(arch)
        if m > _lib.SPARSE_MAX_CAPACITY:
            raise ValueError(f"restore: {m} entries, at most {_lib.SPARSE_MAX_CAPACITY} a call")
        with torch.cuda.device(self.device):
            if m and arch.bricks.device != self.device:
                arch = arch.to(self.device)
            record = torch.empty(_lib.SPARSE_RESTORE_RECORD_WORDS, dtype=torch.int64, device=self.device) if record is None else record
            scratch = torch.empty(_lib.SPARSE_RESTORE_SCRATCH_WORDS // 2, dtype=torch.int64, device=self.device)
            a = _lib.SparseRestoreArgs.new(m=m, vol=self._vol, born=_lib.dptr(self.born, torch.int32),
                                           arch_brick=_lib.dptr(arch.bricks.contiguous(), torch.int32) if m else None,
                                           arch_born=_lib.dptr(arch.born.contiguous(), torch.int32) if m and arch.born is not None else None,
                                           arch_tsdf=_lib.dptr(arch.tsdf.contiguous()) if m else None,
                                           arch_weight=_lib.dptr(arch.weight.contiguous()) if m else None,
                                           arch_color=_lib.dptr(arch.color.contiguous()) if m and arch.color is not None else None,
                                           mark=self._mark.data_ptr(), scan=self._scan.data_ptr(), scratch=_lib.dptr(scratch, torch.int64),
                                           record=_lib.dptr(record, torch.int64))
            _lib.check(_lib.lib().mipsf_sparse_restore(C.byref(a), _lib.stream_ptr()), "sparse_restore")
        if m:
            self.bricks_in_use = None
        return record

    def restore(self, archive: BrickArchive) -> RestoreCounts:
        """Brings the bricks of a BrickArchive back: each gets a slot and the words it left with (and its ``born``); of two entries of
        one brick the first wins; a brick that has a slot meanwhile keeps what it holds (``occupied``); bricks that find the pool
        full are ``dropped``.  One read-back."""
        with torch.cuda.device(self.device):
            counts = RestoreCounts(*(int(x) for x in self.restore_enqueue(archive).tolist()))
        if counts.listed:
            self.bricks_in_use = counts.bricks_in_use
        return counts

    def allocated_bricks(self) -> np.ndarray:
        """the bricks in use, in slot order -> int64 [m,3] brick coordinates (one read-back of slot_brick)"""
        got = torch.cat([self.count, self.slot_brick]).cpu().numpy().astype(np.int64)
        self.bricks_in_use = min(int(got[0]), self.capacity)
        b = got[1:1 + self.bricks_in_use]
        return np.stack([b // (self.bricks[1] * self.bricks[2]), (b // self.bricks[2]) % self.bricks[1], b % self.bricks[2]], 1)

    def tight_window(self):
        """-> (lo, hi): the box of the allocated bricks in voxel indices, hi exclusive; None when nothing is allocated"""
        b = self.allocated_bricks()
        if len(b) == 0:
            return None
        size = np.asarray(BRICK, np.int64)
        return tuple(int(x) for x in b.min(0) * size), tuple(int(x) for x in np.minimum((b.max(0) + 1) * size, np.asarray(self.dims, np.int64)))

    def to_dense(self, lo=None, hi=None) -> TSDFVolume:
        """The window lo <= voxel index < hi of the volume as a dense TSDFVolume, zeros where no brick is allocated; by default the
        tight box of the allocated bricks.  Its voxels sit where they sit in this volume, so it can be marched, ray cast, tracked
        against and fused into like any other.  Refused when the window holds 2^31 voxels or more."""
        if lo is None or hi is None:
            box = self.tight_window()
            if box is None:
                box = ((0, 0, 0), tuple(min(d, b) for d, b in zip(self.dims, BRICK)))
            lo, hi = (box[0] if lo is None else lo), (box[1] if hi is None else hi)
        return self.gather_enqueue(lo, hi)

    def extract_mesh(self, min_weight: float = 1.0, window=None, mesh_savepath: str = "") -> Mesh:
        """TSDFVolume.extract_mesh of to_dense(*window) (``window`` = (lo, hi); the tight box by default): vertices in world
        coordinates, colours when colour was fused."""
        lo, hi = (None, None) if window is None else window
        return self.to_dense(lo, hi).extract_mesh(min_weight, mesh_savepath)

    # ----------------------------------------------------------------------------------------------------------- brick by brick
    def _mesh_args(self, min_weight: float):
        """mipsf_sparse_mesh_count enqueued -> (argument block, cases uint8 [capacity,1024], offsets int32 [capacity + 1])"""
        lib = _lib.lib()
        cases = torch.empty(self.capacity, _lib.SPARSE_BRICK_VOXELS, dtype=torch.uint8, device=self.device)
        offsets = torch.empty(self.capacity + 1, dtype=torch.int32, device=self.device)
        scan = torch.empty(int(lib.mipsf_sparse_mesh_scan_words(self.capacity)) // 2, dtype=torch.int64, device=self.device)
        a = _lib.SparseMeshArgs.new(min_weight=float(min_weight), vol=self._vol, cases=_lib.dptr(cases, torch.uint8),
                                    offsets=_lib.dptr(offsets, torch.int32), scan=_lib.dptr(scan, torch.int64))
        _lib.check(lib.mipsf_sparse_mesh_count(C.byref(a), _lib.stream_ptr()), "sparse_mesh_count")
        return a, cases, offsets

    def brick_soup_enqueue(self, min_weight: float = 1.0, return_cells: bool = False):
        """The triangle soup of the allocated bricks in slot order (mipsf_sparse_mesh_count, one read-back of the triangle count T,
        mipsf_sparse_mesh_emit) -> soup fp32 [T,3,3] in the coordinates of each brick's block (the brick plus one voxel on every side:
        index units minus the brick's base (8bx-1, 8by-1, 16bz-1)), tri_slot int32 [T], offsets int32 [capacity + 1] (the first
        triangle of every slot; offsets[capacity] = T) (, the cell within the brick int32 [T]); all on the device."""
        with torch.cuda.device(self.device):
            a, cases, offsets = self._mesh_args(min_weight)
            T = int(offsets[-1]) & 0xFFFFFFFF               # the one read-back the soup's size needs
            if T > _lib.SPARSE_MESH_MAX_TRIS:
                raise RuntimeError(f"the soup of the bricks has {T} triangles or more, at most {_lib.SPARSE_MESH_MAX_TRIS} can be welded")
            soup = torch.empty((T, 3, 3), dtype=torch.float32, device=self.device)
            tri_slot = torch.empty((T,), dtype=torch.int32, device=self.device)
            cells = torch.empty((T,), dtype=torch.int32, device=self.device) if return_cells else None
            if T:
                a.soup, a.tri_slot, a.cell_ids, a.capacity_tris = _lib.dptr(soup), _lib.dptr(tri_slot, torch.int32), _lib.dptr(cells, torch.int32), T
                _lib.check(_lib.lib().mipsf_sparse_mesh_emit(C.byref(a), _lib.stream_ptr()), "sparse_mesh_emit")
        return (soup, tri_slot, offsets) + ((cells,) if return_cells else ())

    def weld_bricks(self, soup: torch.Tensor, tri_slot: torch.Tensor, max_rounds: int = 2):
        """mipsf_sparse_mesh_weld: the soup of brick_soup_enqueue welded on the global 1e-5 grid -> vertices float64 [V,3] in index
        units of the virtual grid, numbered by first appearance, faces int32 [T,3]; one read-back (V) per attempt, as mesh.weld"""
        T = soup.shape[0]
        with torch.cuda.device(self.device):
            scratch = torch.empty(_lib.buffer_size(_lib.SIZE_MCUBES_WELD_WORDS, T) // 2 + 1, dtype=torch.int64, device=self.device)
            vertices = torch.empty((3 * T, 3), dtype=torch.float64, device=self.device)
            faces = torch.empty((T, 3), dtype=torch.int32, device=self.device)
            counts = torch.empty(4, dtype=torch.int32, device=self.device)
            while True:
                a = _lib.SparseMeshWeldArgs.new(T=T, capacity_tris=T, max_rounds=max_rounds, vol=self._vol, soup=_lib.dptr(soup) if T else None,
                                                tri_slot=_lib.dptr(tri_slot, torch.int32) if T else None, scratch=_lib.dptr(scratch, torch.int64),
                                                vertices=_lib.dptr(vertices, torch.float64) if T else None,
                                                faces=_lib.dptr(faces, torch.int32) if T else None, counts=_lib.dptr(counts, torch.int32))
                _lib.check(_lib.lib().mipsf_sparse_mesh_weld(C.byref(a), _lib.stream_ptr()), "sparse_mesh_weld")
                V, moved, unplaced, _ = counts.tolist()
                if unplaced:
                    raise RuntimeError(f"sparse_mesh_weld: {unplaced} soup vertices without a brick or with a cell outside the weld grid")
                if moved < max_rounds:
                    break
                if max_rounds >= 64:
                    raise RuntimeError("sparse_mesh_weld: labels still moving after 64 rounds (a chain of more than 64 weld cells)")
                max_rounds = min(64, 4 * max_rounds)            # a chain of clusters longer than the rounds: go on
        return vertices[:V], faces

    def sample_enqueue(self, points: torch.Tensor) -> torch.Tensor:
        """points float64 [m,3] in index units of the virtual grid, on the device -> colour fp32 [m,3] on the device
        (mipsf_sparse_sample)"""
        if self.color is None:
            raise ValueError("the volume was made without colour")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: expected [m,3], got {tuple(points.shape)}")
        m = points.shape[0]
        with torch.cuda.device(self.device):
            out = torch.empty(max(m, 1), 3, dtype=torch.float32, device=self.device)[:m]
            a = _lib.SparseSampleArgs.new(m=m, vol=self._vol, points=_lib.dptr(points, torch.float64), out=out.data_ptr())
            _lib.check(_lib.lib().mipsf_sparse_sample(C.byref(a), _lib.stream_ptr()), "sparse_sample")
        return out

    def extract_mesh_bricks(self, min_weight: float = 1.0, mesh_savepath: str = "") -> Mesh:
        """The mesh of the WHOLE volume, marched brick by brick: no dense window is formed and the virtual grid may hold 2^31 voxels
        and more (a side of at most 21474 voxels: the weld's cells are 32-bit).  The marching volume is tsdf where the brick has a
        slot and weight >= min_weight, off elsewhere; isovalue 0, truncation 1 and the face filters are TSDFVolume.extract_mesh's.
        Two read-backs, the triangle count and the vertex count.  -> Mesh with world vertices in float64 (origin + index * voxel_size,
        the index exact), faces int64, and per-vertex colours when colour was fused."""
        with torch.cuda.device(self.device):
            soup, tri_slot, _ = self.brick_soup_enqueue(min_weight)
            v, f = self.weld_bricks(soup, tri_slot)
            f = filter_faces(f)[0].to(torch.int64)
            colors = None if self.color is None else self.sample_enqueue(v.contiguous()).cpu().numpy()
        mesh = Mesh(self.origin + v.cpu().numpy() * self.voxel_size, f.cpu().numpy(), colors)
        if mesh_savepath:
            save_ply(mesh_savepath, mesh.vertices, mesh.faces, mesh.vertex_colors)
        return mesh

    def raycast(self, c2w, K, H: int, W: int, near: float = 0.0, far: float = math.inf, step: Optional[float] = None,
                min_weight: float = 1.0, normals: bool = True, color: bool = False) -> Raycast:
        """TSDFVolume.raycast over the allocated bricks; a voxel of an unallocated brick is unobserved.  Device tensors; nothing is
        read back."""
        with torch.cuda.device(self.device):
            return self.raycast_enqueue(_poses(c2w, self.device), K, H, W, near, far, step, min_weight, normals, color)


def _grid(bounds, voxel_size: float):
    b = np.asarray(bounds.detach().cpu() if torch.is_tensor(bounds) else bounds, np.float64).reshape(3, 2)
    counts = np.ceil((b[:, 1] - b[:, 0]) / voxel_size)
    if not (np.all(np.isfinite(counts)) and np.all(counts >= 0)):
        raise ValueError(f"bounds {b.tolist()} at voxel size {voxel_size}")
    return b, [int(c) + 1 for c in counts]


def sparse_tsdf_mesh_from_frames(depth, c2w, K, voxel_size: float, capacity_bricks: int, trunc: Optional[float] = None, rgb=None, bounds=None,
                                 depth_max: float = math.inf, min_weight: float = 1.0, mesh_savepath: str = "", device=None,
                                 return_volume: bool = False, band: Optional[float] = None, views_per_call: Optional[int] = None,
                                 bricks: bool = False):
    """tsdf_mesh_from_frames with a SparseTSDFVolume of ``capacity_bricks`` slots: the grid over ``bounds`` may hold 2^31 voxels and
    more; the mesh is marched over the tight box of the allocated bricks, which must hold fewer, or with ``bricks`` brick by brick
    (extract_mesh_bricks), which has no such limit.  Bricks dropped for want of slots are an error here: the mesh would have holes."""
    voxel_size = float(voxel_size)
    trunc = 4.0 * voxel_size if trunc is None else float(trunc)
    dev = depth.device if torch.is_tensor(depth) and depth.is_cuda else _device(device)
    with torch.cuda.device(dev):
        D = _images(depth, dev, 0, "depth")
        P = _poses(c2w, dev)
        C3 = None if rgb is None else _images(rgb, dev, 3, "rgb")
        if bounds is None:
            bounds = frames_bounds(D, P, K, depth_max)
            bounds[:, 0] -= trunc
            bounds[:, 1] += trunc
        b, dims = _grid(bounds, voxel_size)
        vol = SparseTSDFVolume(b[:, 0], voxel_size, dims, trunc, capacity_bricks, color=C3 is not None, band=band, device=dev)
        counts = vol.integrate(D, P, K, C3, depth_max, views_per_call)
        if counts.dropped:
            raise RuntimeError(f"{counts.dropped} bricks found no slot: capacity_bricks {capacity_bricks} is too small ({counts.bricks_in_use} in use)")
        mesh = vol.extract_mesh_bricks(min_weight, mesh_savepath) if bricks else vol.extract_mesh(min_weight, mesh_savepath=mesh_savepath)
    return (mesh, vol) if return_volume else mesh


def sparse_tsdf_odometry(depth, K, first_pose, voxel_size: float, bounds, capacity_bricks: int, trunc: Optional[float] = None, rgb=None,
                         min_correspondences: int = 0, device=None, color_weight: Optional[float] = None, band: Optional[float] = None,
                         keep_radius: Optional[float] = None, **track_kw):
    """tsdf_odometry over a SparseTSDFVolume: frame 0 is fused at ``first_pose``; every later frame is registered against the ray
    cast from the previous frame's pose and fused (bricks allocated first) at the pose found.  The walk is enqueued whole; one
    read-back at the end.  A lost frame is fused at a NaN pose, which allocates and updates nothing.
    -> (poses fp32 [n,4,4] on the host, records, SparseTSDFVolume); the records are tsdf_odometry's, and the last one also holds
    ``dropped`` (bricks that found no slot, over all frames) and ``bricks_in_use``.  With ``keep_radius`` (metres) the bricks that
    lie wholly outside the box [t - keep_radius, t + keep_radius] around the position t of the pose a frame was fused at are released
    after that frame's fusion, so a pool smaller than the scene follows the camera; the box is made on the device (no read-back), a
    lost frame has a NaN pose and releases nothing, every record then also holds that frame's ``dropped`` and ``released``, and the
    last one the sum ``released_total`` (its ``dropped`` stays the sum over all frames).  Without it the launches are those of before."""
    if color_weight is not None and rgb is None:
        raise ValueError("color_weight: tracking with colour needs rgb")
    voxel_size = float(voxel_size)
    trunc = 4.0 * voxel_size if trunc is None else float(trunc)
    dev = depth.device if torch.is_tensor(depth) and depth.is_cuda else _device(device)
    _, dims = _grid(bounds, voxel_size)
    b = np.asarray(bounds.detach().cpu() if torch.is_tensor(bounds) else bounds, np.float64).reshape(3, 2)
    with torch.cuda.device(dev):
        D = _images(depth, dev, 0, "depth")
        C3 = None if rgb is None else _images(rgb, dev, 3, "rgb")
        n, H, W = D.shape
        if n < 1:
            raise ValueError("no frames")
        vol = SparseTSDFVolume(b[:, 0], voxel_size, dims, trunc, capacity_bricks, color=C3 is not None, band=band, device=dev)
        poses = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
        words = _lib.TRACK_RESULT_DOUBLES if color_weight is None else _lib.TRACK_COLOR_RESULT_DOUBLES
        results = torch.zeros(n, words, dtype=torch.float64, device=dev)
        lost = torch.zeros(n, dtype=torch.bool, device=dev)
        poses[0] = _poses(first_pose, dev)[0]
        nan_pose = torch.full((4, 4), math.nan, dtype=torch.float32, device=dev)
        if keep_radius is not None and not (float(keep_radius) >= 0 and math.isfinite(float(keep_radius))):
            raise ValueError(f"keep_radius {keep_radius} is negative, infinite or not a number")
        reach = None if keep_radius is None else torch.tensor([-float(keep_radius)] * 3 + [float(keep_radius)] * 3, dtype=torch.float64, device=dev)
        released = []

        def let_go(pose):                                # the box around where the frame was fused, from the device's words
            if reach is not None:
                released.append(vol.release_enqueue(pose[:3, 3].to(torch.float64).repeat(2) + reach))
        allocs = [vol.integrate_enqueue(D[:1], poses[:1], K, None if C3 is None else C3[:1])[1]]
        let_go(poses[0])
        for k in range(1, n):
            prev = poses[k - 1]
            if color_weight is None:
                result, pose = vol.track_enqueue(D[k], K, prev, **track_kw)
            else:
                result, pose = vol.track_enqueue(D[k], K, prev, rgb=C3[k], color_weight=color_weight, **track_kw)
            bad = result[16] < float(min_correspondences)
            poses[k] = torch.where(bad, prev, pose)
            results[k], lost[k] = result, bad
            fused_at = torch.where(bad, nan_pose, pose)
            allocs.append(vol.integrate_enqueue(D[k:k + 1], fused_at[None], K, None if C3 is None else C3[k:k + 1])[1])
            let_go(fused_at)
        got = torch.cat([poses.reshape(n, 16).to(torch.float64), results] + ([torch.stack(released).to(torch.float64)] if released else [])
                        + [lost[:, None].to(torch.float64), torch.stack(allocs).to(torch.float64)], 1).cpu()
    records = [{"transformation": r[16:32].reshape(4, 4).clone(), "n_correspondences": int(r[32]), "fitness": float(r[33]),
                "inlier_rmse": float(r[34]), "iterations": int(r[35]), "lost": bool(r[-5])} for r in got]
    if color_weight is not None:
        for rec, r in zip(records, got):
            rec["n_color"], rec["color_rmse"] = int(r[36]), float(r[37])
    records[-1]["dropped"], records[-1]["bricks_in_use"] = int(got[:, -2].sum()), int(got[-1, -1])
    if released:
        at = 16 + words
        for rec, r in zip(records, got):
            rec["dropped"], rec["released"] = int(r[-2]), int(r[at + 1])
        records[-1]["dropped"], records[-1]["released_total"], records[-1]["bricks_in_use"] = int(got[:, -2].sum()), int(got[:, at + 1].sum()), int(got[-1, at + 6])
        vol.bricks_in_use = int(got[-1, at + 6])
    else:
        vol.bricks_in_use = int(got[-1, -1])
    return got[:, :16].reshape(n, 4, 4).to(torch.float32), records, vol
