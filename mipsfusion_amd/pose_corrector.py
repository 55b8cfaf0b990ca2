"""Rectifying the pose of a switch back to an earlier sub-map (upstream: PoseCorrector.py switch_pose_rectifying, which runs
open3d's ``estimate_normals()`` and point-to-plane ``registration_icp()`` on the host).  Here the clouds are built from the ray
rows that already live in HBM and every step is a HIP kernel of ``csrc/icp.hip`` (C ABI: include/mipsf_icp.h):

    cloud_from_rays      points of ray rows under their owners' poses, rows without depth compacted away in order
    estimate_normals     exact 30 nearest neighbours on a uniform grid, float64 covariance, closed-form eigenvector
    registration_icp     the whole registration loop enqueued at once; one read-back when it has finished
    switch_pose_rectifying   PoseCorrector.py:114-163 on top of the three

The registration loop restates open3d's published algorithm from reading; no open3d version is pinned anywhere upstream, and none
is installed here (tests/icp_cpu.py is the float64 restatement the kernels are held to).  Neighbour sets and pair sets EQUAL
those of a float64 host computation: all comparisons are on float64 squared distances ordered by (distance, index).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib

DEFAULT_MAX_CELLS = 1 << 21             # cells of a grid (two uint32 tables of that length); a larger extent grows the edge
EDGE_MARGIN = 1.0 + 1e-6                # cell edge over the correspondence distance (include/mipsf_icp.h: mipsf_icp_nearest)

# tracking.switch: the reference's shipped values, read with defaults (synth's configurations carry lr_rot / lr_trans / map_num only)
SWITCH_DEFAULTS = {"align_threshold": 0.05, "including_last": 0, "min_correspondence": 2000, "min_trans_dist": 0.5}


class IcpResult(NamedTuple):
    transformation: torch.Tensor        # float64 [4,4], CPU
    n_correspondences: int
    fitness: float
    inlier_rmse: float
    iterations: int
    correspondence_set: torch.Tensor    # int64 [n_correspondences, 2] (source index, target index), CPU


def _ws_bytes(which: int, n: int, cells: int = 0) -> int:
    v = int(_lib.lib().mipsf_icp_workspace_bytes(which, n, cells))
    if v == 0:
        raise RuntimeError(f"mipsf_icp_workspace_bytes({which}, {n}, {cells}): out of range")
    return v


def _bytes(n: int, dev) -> torch.Tensor:
    return torch.empty((n + 15) // 16 * 2, dtype=torch.float64, device=dev)       # 16-byte granules, 256-byte aligned by torch


def _points(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected [n,3], got {tuple(t.shape)}")
    _lib.dptr(t, torch.float32)
    return t


def _cells(max_cells: Optional[int]) -> int:
    c = DEFAULT_MAX_CELLS if max_cells is None else int(max_cells)
    if not 1 <= c <= _lib.ICP_MAX_CELLS:
        raise ValueError(f"max_cells {c} outside 1 .. {_lib.ICP_MAX_CELLS}")
    return c


# --------------------------------------------------------------------------------------------------------------- enqueue only
def cloud_enqueue(rows: torch.Tensor, owner, poses: torch.Tensor):
    """-> (points fp32 [n,3] of which the first `count` rows are the cloud, count uint32 [1] on the device).  Nothing is
    read back.  owner: int32 [n] tensor, or an int = rows per pose (row i belongs to pose i // owner)."""
    if rows.dim() != 2 or rows.shape[1] != 7:
        raise ValueError(f"rows: expected [n,7], got {tuple(rows.shape)}")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise ValueError(f"poses: expected [k,4,4], got {tuple(poses.shape)}")
    n, k = rows.shape[0], poses.shape[0]
    dev = rows.device
    points = torch.empty(max(n, 1), 3, dtype=torch.float32, device=dev)[:n]
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _bytes(_ws_bytes(_lib.ICP_WS_CLOUD, n), dev)
    per, own = 0, None
    if isinstance(owner, torch.Tensor):
        if owner.shape != (n,):
            raise ValueError(f"owner: expected [{n}], got {tuple(owner.shape)}")
        own = _lib.dptr(owner, torch.int32)
    else:
        per = int(owner)
        if per < 1:
            raise ValueError("owner: rows per pose must be positive")
    a = _lib.IcpCloudArgs.new(n=n, k=k, rows_per_owner=per, rows=_lib.dptr(rows), owner=own, poses=_lib.dptr(poses),
                              points=points.data_ptr(), count=count.data_ptr(), workspace=ws.data_ptr())
    _lib.check(_lib.lib().mipsf_icp_cloud(C.byref(a), _lib.stream_ptr()), "icp_cloud")
    return points, count


def bin_enqueue(points: torch.Tensor, min_edge: float = 0.0, max_cells: Optional[int] = None):
    """The grid of a cloud -> (opaque device buffer, max_cells).  min_edge 0: the edge follows the cloud's density."""
    _points(points, "points")
    cells = _cells(max_cells)
    grid = _bytes(_ws_bytes(_lib.ICP_WS_GRID, points.shape[0], cells), points.device)
    a = _lib.IcpBinArgs.new(n=points.shape[0], max_cells=cells, points=points.data_ptr(), min_edge=float(min_edge),
                            grid=grid.data_ptr())
    _lib.check(_lib.lib().mipsf_icp_bin(C.byref(a), _lib.stream_ptr()), "icp_bin")
    return grid, cells


def normals_enqueue(points: torch.Tensor, max_cells: Optional[int] = None, neighbours: bool = False):
    """-> normals float64 [n,3]; with neighbours=True -> (normals, int32 [n,30] neighbour indices, nearest first, -1 padded)"""
    _points(points, "points")
    n = points.shape[0]
    out = torch.empty(n, 3, dtype=torch.float64, device=points.device)
    nb = torch.empty(n, _lib.ICP_KNN, dtype=torch.int32, device=points.device) if neighbours else None
    if n:
        grid, cells = bin_enqueue(points, 0.0, max_cells)
        a = _lib.IcpNormalsArgs.new(n=n, max_cells=cells, points=points.data_ptr(), grid=grid.data_ptr(), normals=out.data_ptr(),
                                    neighbours=nb.data_ptr() if neighbours else None)
        _lib.check(_lib.lib().mipsf_icp_normals(C.byref(a), _lib.stream_ptr()), "icp_normals")
    return (out, nb) if neighbours else out


def registration_enqueue(source, target, target_normals, max_dist, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                         max_cells: Optional[int] = None):
    """The registration loop, enqueued: -> (result float64 [20] = T row major | correspondences | fitness | inlier rmse |
    iterations, partner int32 [n_source] = the target index of each source point in the last evaluation or -1), both on the
    device.  No synchronisation and no read-back: the call can be recorded into a graph and replayed on new points."""
    _points(source, "source"), _points(target, "target")
    if tuple(target_normals.shape) != tuple(target.shape):
        raise ValueError("target_normals: one normal per target point")
    _lib.dptr(target_normals, torch.float64)
    if not (0.0 <= float(max_dist) < float("inf")):
        raise ValueError(f"max_dist {max_dist}")
    dev = source.device
    ns, nt = source.shape[0], target.shape[0]
    grid, cells = bin_enqueue(target, float(max_dist) * EDGE_MARGIN, max_cells)
    result = torch.empty(_lib.ICP_RESULT_DOUBLES, dtype=torch.float64, device=dev)
    partner = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)[:ns]
    ws = _bytes(_ws_bytes(_lib.ICP_WS_REGISTER, ns), dev)
    a = _lib.IcpRegisterArgs.new(n_source=ns, n_target=nt, max_cells=cells, max_iteration=int(max_iteration),
                                 source=source.data_ptr(), grid=grid.data_ptr(), target_normals=target_normals.data_ptr(),
                                 max_dist=float(max_dist), relative_fitness=float(relative_fitness),
                                 relative_rmse=float(relative_rmse), result=result.data_ptr(), partner=partner.data_ptr(),
                                 workspace=ws.data_ptr())
    _lib.check(_lib.lib().mipsf_icp_register(C.byref(a), _lib.stream_ptr()), "icp_register")
    return result, partner


# --------------------------------------------------------------------------------------------------------------- public
def cloud_from_rays(rows: torch.Tensor, owner, poses: torch.Tensor):
    """PoseCorrector.py construct_pc / construct_pc_given_kfs without the open3d object -> (points fp32 [m,3], m): the rows
    with depth > 0 under their owners' poses, in their original order (one 4-byte read-back for m)."""
    points, count = cloud_enqueue(rows, owner, poses)
    m = int(count.item())
    return points[:m], m


def nearest_neighbours(source, target, max_dist, max_cells: Optional[int] = None):
    """-> (partner int32 [n_source]: index of the nearest target point within max_dist or -1, its float64 squared distance or
    inf): one evaluation of the registration's pairing, exposed for tests and tools."""
    _points(source, "source"), _points(target, "target")
    ns = source.shape[0]
    grid, cells = bin_enqueue(target, float(max_dist) * EDGE_MARGIN, max_cells)
    partner = torch.empty(max(ns, 1), dtype=torch.int32, device=source.device)[:ns]
    d2 = torch.empty(max(ns, 1), dtype=torch.float64, device=source.device)[:ns]
    a = _lib.IcpNearestArgs.new(n_source=ns, n_target=target.shape[0], max_cells=cells, source=source.data_ptr(),
                                grid=grid.data_ptr(), max_dist=float(max_dist), partner=partner.data_ptr(), d2=d2.data_ptr())
    _lib.check(_lib.lib().mipsf_icp_nearest(C.byref(a), _lib.stream_ptr()), "icp_nearest")
    return partner, d2


def estimate_normals(points: torch.Tensor, max_cells: Optional[int] = None) -> torch.Tensor:
    """open3d ``PointCloud.estimate_normals()`` with its default search (30 nearest neighbours, the point included) -> float64
    [m,3] unit normals of arbitrary sign; (0,0,1) for a cloud of fewer than 3 points or where no direction exists."""
    return normals_enqueue(points, max_cells)


def registration_icp(source, target, target_normals, max_dist, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                     max_cells: Optional[int] = None) -> IcpResult:
    """open3d ``registration_icp(source, target, max_dist, identity, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))``."""
    result, partner = registration_enqueue(source, target, target_normals, max_dist, max_iteration, relative_fitness,
                                           relative_rmse, max_cells)
    r = result.cpu()                                                # the one read-back the loop waits for
    partner = partner.cpu().to(torch.int64)
    src = torch.nonzero(partner >= 0).reshape(-1)
    return IcpResult(r[:16].reshape(4, 4).clone(), int(r[16]), float(r[17]), float(r[18]), int(r[19]),
                     torch.stack([src, partner[src]], 1))


def switch_settings(cfg) -> dict:
    """tracking.switch's rectification keys, the reference's shipped values where a configuration leaves them out"""
    sw = cfg.get("tracking", {}).get("switch", {}) or {}
    return {k: sw.get(k, v) for k, v in SWITCH_DEFAULTS.items()}


def nearest_keyframes(frame_points: torch.Tensor, kf_centres: torch.Tensor, limit: int = 10):
    """The upstream's choice of target keyframes when nothing better is known: at most `limit` keyframes whose camera
    centres are nearest to the mean of the frame's points -> indices into kf_centres (host list, nearest first)."""
    if frame_points.shape[0] == 0 or kf_centres.shape[0] == 0:
        return list(range(min(limit, kf_centres.shape[0])))
    d = (kf_centres.double().cpu() - frame_points.double().mean(0).cpu()).norm(dim=1)
    return torch.argsort(d, stable=True)[:limit].tolist()


def switch_pose_rectifying(ray_db, target_kf_slots, target_kf_poses, frame_rows, pose_local_this, cfg, extra_source=None):
    """PoseCorrector.py:114-163 -> (flag, n_correspondences, pose fp32 [4,4] CPU).

    ray_db: DeviceRayDB; target_kf_slots: the chosen keyframes of the sub-map switched to (the choice is host control plane,
    Manager.py:296-307); target_kf_poses [k,4,4]: their poses in that sub-map's frame; frame_rows [r,7]: the frame's down-sampled
    rows; pose_local_this [4,4]: the frame's pose in that frame; extra_source: optional (rows [e,7], owner, poses) of the
    `including_last` earlier keyframes, already expressed in the target sub-map's frame -- they come first in the source cloud, as
    upstream's merge_pc puts them.  Accepted iff the last evaluation has >= min_correspondence pairs; then the relative pose is
    replaced by the identity when its translation is >= min_trans_dist, and pose = float32(rel) @ pose_local_this."""
    st = switch_settings(cfg)
    dev = ray_db.rays.device
    slots = torch.as_tensor(target_kf_slots, dtype=torch.int64, device=dev).reshape(-1)
    pose_this = pose_local_this.detach().to(torch.float32).cpu()
    tgt_rows = ray_db.rays[slots].reshape(-1, 7).contiguous()
    tgt_poses = target_kf_poses.detach().to(dev, torch.float32).contiguous()
    target, _ = cloud_from_rays(tgt_rows, ray_db.num_rays_to_save, tgt_poses)
    source, _ = cloud_from_rays(frame_rows.reshape(-1, 7).contiguous(), max(1, frame_rows.numel() // 7),
                                pose_this.to(dev)[None].contiguous())
    if extra_source is not None and st["including_last"] > 0:
        e_rows, e_owner, e_poses = extra_source
        extra, _ = cloud_from_rays(e_rows.reshape(-1, 7).contiguous(), e_owner, e_poses.detach().to(dev, torch.float32).contiguous())
        source = torch.cat([extra, source]).contiguous()
    res = registration_icp(source, target, estimate_normals(target), st["align_threshold"])
    if res.n_correspondences < st["min_correspondence"]:
        return False, res.n_correspondences, pose_this
    rel = res.transformation.to(torch.float32)
    if float(torch.linalg.norm(rel[:3, 3])) >= st["min_trans_dist"]:
        rel = torch.eye(4, dtype=torch.float32)
    return True, res.n_correspondences, rel @ pose_this
