"""Sub-map management: when a keyframe stays in the active sub-map, expands it, opens a new one or switches back to an earlier one
(upstream: Manager.py, with its state spread over model/keyframeSet.py and the SLAM object).

The decision rules are a plain host state machine, restated branch for branch.  What they look at is geometry of the frame, and
that runs on the device: one ``mipsf_submap_frame_stats`` enqueue per keyframe turns the frame's ray rows [H*W,7] into a record
of integer counts and float32 minima / maxima (one read-back of ~3 KB instead of upstream's host copy of the depth image and
11-16 ms of host torch), and ``mipsf_submap_overlap`` does the geometry of ``find_overlapping_region`` on the rare paths that
need it.  C ABI: include/mipsf_submap.h, kernels: csrc/submap.hip, restatement: mipsfusion_amd/submap_cpu.py.

    frame_stats_enqueue / overlap_enqueue   the launches: device tensors in, device tensors out, no synchronisation, capturable
    SubmapManager                           the state and the rules; ``backend="cpu"`` computes the same records in numpy
    Decision                                what one keyframe did
    derive_schedule                         walk a sequence's keyframes -> the schedule ``GraphedSequence(schedule=...)`` takes
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import submap_cpu as sc

F32 = np.float32
EDGE = 20.0                              # Manager.py:321


# ------------------------------------------------------------------------------------------------------------- the launches
def frame_stats_enqueue(rows, pose, boxes, max_len, H, W, lat_a, lat_b, lat_c, near, far, min_cr_len, out=None):
    """-> (record int32 [_lib.SUBMAP_RECORD_WORDS] on the device, workspace): ``submap_cpu.stats_from_words`` of its words (as
    uint32) is the FrameStats.  rows [H*W,7], pose [4,4], boxes [n,6], max_len [n,3]: contiguous float32 device tensors.  Nothing
    is read back and nothing synchronises; pass the tuple a first call returned as ``out`` to keep the outputs in place."""
    from . import _lib
    if tuple(rows.shape) != (H * W, 7) or tuple(pose.shape) != (4, 4) or boxes.dim() != 2 or boxes.shape[1] != 6 \
            or tuple(max_len.shape) != (boxes.shape[0], 3):
        raise ValueError("frame stats: rows [H*W,7], pose [4,4], boxes [n,6], max_len [n,3]")
    if out is None:
        out = (torch.zeros(_lib.SUBMAP_RECORD_WORDS, dtype=torch.int32, device=rows.device),
               torch.empty(_lib.SUBMAP_WORKSPACE_BYTES // 8, dtype=torch.float64, device=rows.device))
    record, ws = out
    if record.numel() != _lib.SUBMAP_RECORD_WORDS or ws.numel() * ws.element_size() < _lib.SUBMAP_WORKSPACE_BYTES:
        raise ValueError("frame stats: `out` is not a tuple an earlier call returned")
    a = _lib.SubmapFrameStatsArgs.new(H=H, W=W, n_boxes=boxes.shape[0], lat_a_h=lat_a[0], lat_a_w=lat_a[1], lat_b_h=lat_b[0],
                                      lat_b_w=lat_b[1], lat_c_h=lat_c[0], lat_c_w=lat_c[1], near=float(near), far=float(far),
                                      min_cr_len=(C.c_float * 3)(*[float(v) for v in min_cr_len]), rows=_lib.dptr(rows),
                                      pose=_lib.dptr(pose), boxes=_lib.dptr(boxes), max_len=_lib.dptr(max_len),
                                      record=_lib.dptr(record, torch.int32), workspace=ws.data_ptr())
    _lib.check(_lib.lib().mipsf_submap_frame_stats(C.byref(a), _lib.stream_ptr()), "submap_frame_stats")
    return out


def overlap_enqueue(rows, pose, H, W, lat, intrinsics, cam_wh, target_box, table=None, related_slots=None, related_poses=None,
                    top_poses=None, edge=EDGE, out=None):
    """mipsf_submap_overlap -> dict of device tensors: ``dist`` float64 [n] when related keyframes are given (table
    [slots,R,7] float32, related_slots int32 [n], related_poses float32 [n,4,4]); ``top_kf_masks`` uint8 [k,P], ``mask_final``
    uint8 [P], ``count`` int32 [1], ``target_d`` float32 [P], ``rays_d_cam`` float32 [P,3] when ``top_poses`` [k,4,4] are given.
    No read-back, no synchronisation; ``out`` = the dict of an earlier call of the same shapes keeps the outputs in place."""
    from . import _lib
    dev, P = rows.device, lat[0] * lat[1]
    n = 0 if related_slots is None else int(related_slots.shape[0])
    k = 0 if top_poses is None else int(top_poses.shape[0])
    if tuple(rows.shape) != (H * W, 7) or tuple(pose.shape) != (4, 4):
        raise ValueError("overlap: rows [H*W,7], pose [4,4]")
    if n and (table is None or table.dim() != 3 or table.shape[2] != 7 or tuple(related_poses.shape) != (n, 4, 4)):
        raise ValueError("overlap: table [slots,R,7], related_slots [n], related_poses [n,4,4]")
    if k and tuple(top_poses.shape) != (k, 4, 4):
        raise ValueError("overlap: top_poses [k,4,4]")
    if out is None:
        out = {}
        if n:
            out["dist"] = torch.empty(n, dtype=torch.float64, device=dev)
        if k:
            out.update(top_kf_masks=torch.empty(k, P, dtype=torch.uint8, device=dev), mask_final=torch.empty(P, dtype=torch.uint8, device=dev),
                       count=torch.empty(1, dtype=torch.int32, device=dev), target_d=torch.empty(P, dtype=torch.float32, device=dev),
                       rays_d_cam=torch.empty(P, 3, dtype=torch.float32, device=dev))
    if (n and tuple(out["dist"].shape) != (n,)) or (k and tuple(out["top_kf_masks"].shape) != (k, P)):
        raise ValueError("overlap: `out` is not the dict of a call of these shapes")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    a = _lib.SubmapOverlapArgs.new(H=H, W=W, lat_h=lat[0], lat_w=lat[1], n_related=n, k=k, n_slots=table.shape[0] if n else 0,
                                   rows_per_slot=table.shape[1] if n else 0, fx=fx, fy=fy, cx=cx, cy=cy, cam_W=float(cam_wh[0]),
                                   cam_H=float(cam_wh[1]), edge=float(edge),
                                   target_box=(C.c_float * 6)(*[float(v) for v in np.asarray(target_box, F32).reshape(6)]),
                                   rows=_lib.dptr(rows), pose=_lib.dptr(pose))
    if n:
        a.table, a.related_slots, a.related_poses = _lib.dptr(table), _lib.dptr(related_slots, torch.int32), _lib.dptr(related_poses)
        a.dist = _lib.dptr(out["dist"], torch.float64)
    if k:
        a.top_poses, a.top_kf_masks, a.mask_final = _lib.dptr(top_poses), _lib.dptr(out["top_kf_masks"], torch.uint8), _lib.dptr(out["mask_final"], torch.uint8)
        a.count, a.target_d, a.rays_d_cam = _lib.dptr(out["count"], torch.int32), _lib.dptr(out["target_d"]), _lib.dptr(out["rays_d_cam"])
    _lib.check(_lib.lib().mipsf_submap_overlap(C.byref(a), _lib.stream_ptr()), "submap_overlap")
    return out


# ------------------------------------------------------------------------------------------------------------- the rules
class Decision(NamedTuple):
    flag: int                            # 1 switch to a previous sub-map, 2 unchanged, 3 new sub-map
    label: str                           # the reference's words for the branch
    keyframe: int
    bindings: tuple                      # the sub-maps the keyframe is bound to, (-1 for none) in keyframe_localMLP's order
    active: int                          # the active sub-map after the call
    boxes: np.ndarray                    # float32 [n,6] centre + length of every sub-map after the call
    stats: sc.FrameStats
    ratios: dict                         # the float32 ratios the branch looked at (cr_active, cr_mo, cr_active_new, cr_wait)
    overlap: Optional[dict]              # for a switch: target_d, rays_d_cam, mask_final, kf_ids, top_kf_masks
    rectified_pose: Optional[np.ndarray]  # for a switch: the keyframe's pose in the sub-map switched to


def _matmul(a, b):
    """upstream's float32 ``a @ b`` on the host, through the same library"""
    return (torch.from_numpy(np.ascontiguousarray(a, F32)) @ torch.from_numpy(np.ascontiguousarray(b, F32))).numpy()


def _inverse(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).inverse().numpy()


def _ratio(count, of):
    with np.errstate(invalid="ignore", divide="ignore"):
        return F32(count) / F32(of)          # 0/0 = nan, compares false


class SubmapManager:
    """The state upstream spreads over ``kfSet`` and the SLAM object, and Manager.py's rules over it.

    cfg: the reference's configuration keys (mapping.min_containing_ratio, min_containing_ratio_mo, min_containing_ratio_back,
    min_cr_localMLP_len, localMLP_max_len, localMLP_max_len_back, localMLP_num, overlapping.{n_rays_h, n_rays_w, min_pts},
    keyframe_every; cam.near, cam.far, cam.W, cam.H; sampling.kf_n_rays_h / kf_n_rays_w for the keyframes' stored rows).
    intrinsics: (fx, fy, cx, cy) of the H x W frames.  rectify(rows, pose_local_ini, pose_local_before, submap_after,
    submap_before, keyframe_ids, masks) -> (flag, n, pose) stands where upstream calls poseCorrector.switch_pose_rectifying; the
    default adapts ``mipsfusion_amd.switch_pose_rectifying``.  backend "hip": frames are device tensors and the geometry runs in
    csrc/submap.hip; "cpu": numpy (mipsfusion_amd/submap_cpu.py), for the rules alone."""

    def __init__(self, cfg, H, W, intrinsics, device="cuda", rectify=None, backend="hip", lattice_a=(150, 200), lattice_b=(15, 20),
                 max_keyframes=512):
        if backend not in ("hip", "cpu"):
            raise ValueError(f"backend {backend!r}: 'hip' or 'cpu'")
        m = cfg["mapping"]
        self.cfg, self.H, self.W, self.backend = cfg, int(H), int(W), backend
        self.intrinsics = tuple(float(v) for v in intrinsics)
        self.device = torch.device("cpu" if backend == "cpu" else device)
        self.thr, self.thr_mo, self.thr_back = (F32(m[k]) for k in ("min_containing_ratio", "min_containing_ratio_mo",
                                                                    "min_containing_ratio_back"))
        self.min_cr_len = np.asarray(m["min_cr_localMLP_len"], F32)
        self.default_max_len = np.asarray(m["localMLP_max_len"], F32)
        self.max_len_back = np.asarray(m["localMLP_max_len_back"], F32)
        self.every = int(m["keyframe_every"])
        self.near, self.far = float(cfg["cam"]["near"]), float(cfg["cam"]["far"])
        self.cam_wh = (float(cfg["cam"]["W"]), float(cfg["cam"]["H"]))
        self.lat_a, self.lat_b = tuple(lattice_a), tuple(lattice_b)
        self.lat_c = (int(m["overlapping"]["n_rays_h"]), int(m["overlapping"]["n_rays_w"]))
        self.min_pts = int(m["overlapping"]["min_pts"])
        samp = cfg.get("sampling", {})
        self.lat_kf = (int(samp.get("kf_n_rays_h", self.lat_c[0])), int(samp.get("kf_n_rays_w", self.lat_c[1])))
        for name, lat in (("A", self.lat_a), ("B", self.lat_b), ("C", self.lat_c), ("keyframe", self.lat_kf)):
            if not (1 <= lat[0] <= self.H and 1 <= lat[1] <= self.W):
                raise ValueError(f"lattice {name} is {lat[0]} x {lat[1]}, the image is {self.H} x {self.W}")
        self.near_kf_num = sc.MAX_TOP_KF
        self.rectify = rectify if rectify is not None else self._rectify_by_icp
        # keyframeSet.create_MLP_data; the tables grow past localMLP_num as modify_new_localMLP_info grows them
        self.n_submaps = 0
        self.boxes = np.zeros((0, 6), F32)
        self.max_len = np.zeros((0, 3), F32)
        self.first_kf = []                                   # keyframe id of each sub-map's first keyframe
        self.adjacent = set()                                # (i, j), i < j
        self.keyframe_submaps = np.full((max_keyframes, 2), -1, np.int64)     # keyframe_localMLP
        self.keyframe_ref = np.full(max_keyframes, -3, np.int32)              # -1 first keyframe, -2 overlapping keyframe
        self.kf_world = np.zeros((max_keyframes, 4, 4), F32)                  # kf_c2w: world poses of first keyframes
        self.kf_local = np.zeros((max_keyframes, 4, 4), F32)                  # est_c2w_data at the keyframes
        self.n_keyframes = 0                                 # collected_kf_num
        self.active, self.prev_active = 0, -1
        # Manager.create_loop_vars
        self.double_binding_counter, self.db_active, self.db_mo, self.thres_db_time = 0, -1, -1, 4
        self.wait_loop, self.id_wait, self.id_actual = False, -1, -1
        self._kf_pixels = sc.lattice_pixels(self.H, self.W, *self.lat_kf)
        R = len(self._kf_pixels)
        if backend == "hip":
            self.table = torch.zeros(max_keyframes, R, 7, dtype=torch.float32, device=self.device)
            self._kf_pixels_dev = torch.from_numpy(self._kf_pixels).to(self.device)
            self._stats_out = None
        else:
            self.table = np.zeros((max_keyframes, R, 7), F32)

    # --------------------------------------------------------------------------------------------------------- accessors
    def bindings(self):
        """keyframe -> sub-map table [n_keyframes,2] (-1 for none): what ``pose_graph.adjacent_pairs`` takes"""
        return torch.from_numpy(self.keyframe_submaps[:self.n_keyframes].copy())

    def anchors(self):
        """world poses of the sub-maps' first keyframes, float32 [n,4,4]"""
        return self.kf_world[np.asarray(self.first_kf, np.int64)].copy()

    def state(self):
        """the counters and the wait-loop triple, for traces and tests"""
        return {"active": self.active, "prev_active": self.prev_active, "double_binding_counter": self.double_binding_counter,
                "db_pair": (self.db_active, self.db_mo), "wait_loop": bool(self.wait_loop), "wait_pair": (self.id_wait, self.id_actual),
                "n_submaps": self.n_submaps}

    def dump_state(self) -> dict:
        """everything the rules remember, as numpy arrays (``load_state`` of another manager of the same configuration resumes)"""
        n = self.n_keyframes
        table = self.table[:n].cpu().numpy() if self.backend == "hip" else self.table[:n].copy()
        return {"boxes": self.boxes.copy(), "max_len": self.max_len.copy(), "first_kf": np.asarray(self.first_kf, np.int64),
                "adjacent": np.asarray(sorted(self.adjacent), np.int64).reshape(-1, 2), "keyframe_submaps": self.keyframe_submaps[:n].copy(),
                "keyframe_ref": self.keyframe_ref[:n].copy(), "kf_world": self.kf_world[:n].copy(), "kf_local": self.kf_local[:n].copy(),
                "scalars": np.asarray([self.active, self.prev_active, self.double_binding_counter, self.db_active, self.db_mo,
                                       int(self.wait_loop), self.id_wait, self.id_actual], np.int64), "table": table}

    def load_state(self, d) -> None:
        n = len(d["keyframe_ref"])
        self.boxes, self.max_len = np.array(d["boxes"], F32).reshape(-1, 6), np.array(d["max_len"], F32).reshape(-1, 3)
        self.n_submaps, self.first_kf = len(self.boxes), [int(v) for v in d["first_kf"]]
        if not (1 <= self.n_submaps <= sc.MAX_BOXES and len(self.first_kf) == self.n_submaps == len(self.max_len)):
            raise ValueError("load_state: boxes, max_len and first_kf disagree")
        self.adjacent = {(int(a), int(b)) for a, b in np.asarray(d["adjacent"]).reshape(-1, 2)}
        for name in ("keyframe_submaps", "keyframe_ref", "kf_world", "kf_local"):
            arr = getattr(self, name)
            arr[...] = -1 if name == "keyframe_submaps" else (-3 if name == "keyframe_ref" else 0)
            arr[:n] = d[name]
        self.n_keyframes = n
        (self.active, self.prev_active, self.double_binding_counter, self.db_active, self.db_mo, wl, self.id_wait,
         self.id_actual) = (int(v) for v in d["scalars"])
        self.wait_loop = bool(wl)
        if self.backend == "hip":
            self.table[:n].copy_(torch.from_numpy(np.ascontiguousarray(d["table"], F32)))
        else:
            self.table[:n] = d["table"]

    # --------------------------------------------------------------------------------------------------------- geometry
    def _rows(self, rows):
        if self.backend == "hip":
            if not (torch.is_tensor(rows) and rows.is_cuda):
                raise RuntimeError("SubmapManager(backend='hip') takes the frame's ray rows as a device tensor")
            return rows.reshape(self.H * self.W, 7).contiguous()
        return np.ascontiguousarray(rows.cpu().numpy() if torch.is_tensor(rows) else rows, F32).reshape(self.H * self.W, 7)

    def _store_keyframe(self, kf, rows):
        if kf >= len(self.keyframe_ref):
            raise RuntimeError(f"keyframe {kf}: the manager was built for {len(self.keyframe_ref)} keyframes")
        if self.backend == "hip":
            self.table[kf].copy_(rows[self._kf_pixels_dev])
        else:
            self.table[kf] = rows[self._kf_pixels]

    def _stats(self, rows, pose_world) -> sc.FrameStats:
        args = (self.H, self.W, self.lat_a, self.lat_b, self.lat_c, self.near, self.far, self.min_cr_len)
        if self.backend == "cpu":
            return sc.frame_stats(rows, pose_world, self.boxes, self.max_len, *args)
        with torch.cuda.device(self.device):
            host = torch.from_numpy(np.concatenate([pose_world.reshape(-1), self.boxes.reshape(-1), self.max_len.reshape(-1)]))
            dev = host.to(self.device)                       # one upload: pose, boxes, max_len
            n = self.n_submaps
            self._stats_out = frame_stats_enqueue(rows, dev[:16].view(4, 4), dev[16:16 + 6 * n].view(n, 6), dev[16 + 6 * n:].view(n, 3),
                                                  *args, out=self._stats_out)
            words = self._stats_out[0].cpu().numpy().view(np.uint32)      # the one read-back
        return sc.stats_from_words(words)

    def _overlap(self, rows, pose_world, target, related, related_world):
        """-> (top keyframe ids, dict of numpy arrays as submap_cpu.overlap_masks returns)"""
        top, top_world = related, related_world
        if len(related) > self.near_kf_num:
            if self.backend == "cpu":
                dist = sc.overlap_distances(rows, pose_world, self.H, self.W, self.lat_c, self.table, related, related_world)
            else:
                with torch.cuda.device(self.device):
                    out = overlap_enqueue(rows, torch.from_numpy(pose_world).to(self.device), self.H, self.W, self.lat_c, self.intrinsics,
                                          self.cam_wh, self.boxes[target], table=self.table,
                                          related_slots=torch.as_tensor(related, dtype=torch.int32).to(self.device),
                                          related_poses=torch.from_numpy(related_world).to(self.device))
                    dist = out["dist"].cpu().numpy()
            order = np.argsort(dist, kind="stable")[:self.near_kf_num]
            top, top_world = related[order], related_world[order]
        if self.backend == "cpu":
            res = sc.overlap_masks(rows, pose_world, self.H, self.W, self.lat_c, top_world, self.boxes[target], *self.intrinsics,
                                   *self.cam_wh, EDGE)
        elif len(top) == 0:                                  # no keyframe to look from, nothing to launch: nothing is seen
            sel = rows[torch.from_numpy(sc.lattice_pixels(self.H, self.W, *self.lat_c)).to(self.device)].cpu().numpy()
            P = len(sel)
            res = {"top_kf_masks": np.zeros((0, P), bool), "mask_final": np.zeros(P, bool), "count": 0, "target_d": sel[:, 6].copy(),
                   "rays_d_cam": sel[:, :3].copy()}
        else:
            with torch.cuda.device(self.device):
                out = overlap_enqueue(rows, torch.from_numpy(pose_world).to(self.device), self.H, self.W, self.lat_c, self.intrinsics,
                                      self.cam_wh, self.boxes[target], top_poses=torch.from_numpy(np.ascontiguousarray(top_world)).to(self.device))
                res = {k: v.cpu().numpy() for k, v in out.items()}
            res["top_kf_masks"], res["mask_final"] = res["top_kf_masks"].astype(bool), res["mask_final"].astype(bool)
            res["count"] = int(res["count"][0])
        return top, res

    def keyframe_world_poses(self, kf_ids):
        """keyframeSet.convert_given_world_pose: first keyframes have their world pose stored, every other keyframe is the anchor
        of the first sub-map it is bound to times its local pose"""
        out = np.zeros((len(kf_ids), 4, 4), F32)
        for j, kf in enumerate(kf_ids):
            if self.keyframe_ref[kf] == -1:
                out[j] = self.kf_world[kf]
            else:
                out[j] = _matmul(self.kf_world[self.first_kf[self.keyframe_submaps[kf, 0]]], self.kf_local[kf])
        return out

    def _rectify_by_icp(self, rows, pose_ini, pose_before, sub_after, sub_before, kf_ids, masks):
        """PoseCorrector.switch_pose_rectifying through mipsfusion_amd.pose_corrector: the chosen keyframes that see more than 200
        of the frame's points (all of them when none does) make the target cloud, in the frame of the sub-map switched to."""
        if self.backend != "hip":
            raise RuntimeError("the default rectification runs on the device: pass rectify= to SubmapManager(backend='cpu')")
        from .keyframe_rays import DeviceRayDB
        from .pose_corrector import switch_pose_rectifying
        kf_ids = np.asarray(kf_ids, np.int64)
        seen = np.count_nonzero(np.asarray(masks), axis=-1) > 200
        chosen = kf_ids[seen] if seen.any() else kf_ids
        to_local = _inverse(self.kf_world[self.first_kf[sub_after]])
        poses = np.stack([_matmul(to_local, w) for w in self.keyframe_world_poses(chosen)])
        db = DeviceRayDB(self.table.shape[0], self.table.shape[1], self.device, storage=self.table)
        with torch.cuda.device(self.device):
            flag, n, pose = switch_pose_rectifying(db, torch.from_numpy(chosen), torch.from_numpy(poses), rows[self._kf_pixels_dev].contiguous(),
                                                   torch.from_numpy(np.ascontiguousarray(pose_ini, F32)), self.cfg)
        return bool(flag), int(n), pose.numpy()

    # --------------------------------------------------------------------------------------------------------- bookkeeping
    def _new_submap(self, centre_len, kf):
        """keyframeSet.modify_new_localMLP_info (it grows its tables past localMLP_num; the C ABI stops at 64)"""
        if self.n_submaps >= sc.MAX_BOXES:
            raise RuntimeError(f"sub-map {self.n_submaps + 1}: the statistics kernel and the pose graph take at most {sc.MAX_BOXES}")
        self.boxes = np.concatenate([self.boxes, np.asarray(centre_len, F32).reshape(1, 6)])
        self.max_len = np.concatenate([self.max_len, self.default_max_len.reshape(1, 3)])
        self.first_kf.append(int(kf))
        self.n_submaps += 1
        return self.n_submaps - 1

    def _adjacent(self, a, b):
        self.adjacent.add((min(a, b), max(a, b)))

    def first_keyframe(self, rows, pose_world):
        """mipsfusion.py:160-171: the first frame opens sub-map 0 with its own surface box"""
        if self.n_keyframes:
            raise RuntimeError("first_keyframe: the manager already holds keyframes")
        rows, pose_world = self._rows(rows), np.ascontiguousarray(pose_world, F32).reshape(4, 4)
        self._store_keyframe(0, rows)
        self.boxes, self.max_len, self.n_submaps = np.zeros((1, 6), F32), self.default_max_len.reshape(1, 3).copy(), 1   # a box to count against
        stats = self._stats(rows, pose_world)
        self.boxes, self.max_len, self.n_submaps = np.zeros((0, 6), F32), np.zeros((0, 3), F32), 0
        if stats.n_valid == 0:
            raise ValueError(f"first keyframe: no pixel has {self.near} < depth < {self.far}, the surface box is empty")
        self._new_submap(np.concatenate(stats.surface), 0)
        self.kf_world[0], self.kf_local[0], self.keyframe_ref[0] = pose_world, np.eye(4, dtype=F32), -1
        self.keyframe_submaps[0, 0] = 0
        self.n_keyframes, self.active, self.prev_active = 1, 0, -1
        return stats

    # --------------------------------------------------------------------------------------------------------- Manager.py
    def process_keyframe(self, rows, pose_local, frame_id, force=False, pose_world=None) -> Decision:
        """Manager.process_keyframe for the keyframe ``frame_id // keyframe_every``; keyframes come in order.  pose_local: the
        frame's pose in the active sub-map.  pose_world: the frame's world pose where the caller has it (``derive_schedule``
        has); otherwise the active anchor times pose_local in float32, as upstream forms it."""
        if not self.n_keyframes:
            raise RuntimeError("process_keyframe: call first_keyframe first")
        kf = int(frame_id) // self.every
        if kf != self.n_keyframes:
            raise RuntimeError(f"frame {frame_id} is keyframe {kf}, the next keyframe is {self.n_keyframes}")
        rows = self._rows(rows)
        pose_local = np.ascontiguousarray(pose_local, F32).reshape(4, 4)
        self._store_keyframe(kf, rows)                       # kfSet.add_keyframe
        self.kf_local[kf] = pose_local
        active = self.active
        if pose_world is None:
            pose_world = _matmul(self.kf_world[self.first_kf[active]], pose_local)      # convert_pose_to_world
        pose_world = np.ascontiguousarray(pose_world, F32).reshape(4, 4)
        stats = self._stats(rows, pose_world)
        if stats.n_valid == 0:
            raise ValueError(f"keyframe {kf}: no pixel has {self.near} < depth < {self.far}; upstream fails here on the maximum of "
                             "an empty set of surface points")
        ctx = {"rows": rows, "pose_world": pose_world, "pose_local": pose_local, "kf": kf, "frame": int(frame_id), "stats": stats,
               "surface": np.concatenate(stats.surface), "ratios": {}, "overlap": None, "rectified": None}
        if self.wait_loop:
            flag, label = self._wait_loop(ctx, active, force)
        else:
            flag, label = self._normal(ctx, active, force)
        self.n_keyframes += 1
        if flag == 1:                                        # mipsfusion.active_submap_switch: the keyframe's pose in the new frame
            self.kf_local[kf] = ctx["rectified"]
        return Decision(flag, label, kf, tuple(int(v) for v in self.keyframe_submaps[kf]), self.active, self.boxes.copy(), stats,
                        ctx["ratios"], ctx["overlap"] if flag == 1 else None, ctx["rectified"] if flag == 1 else None)

    def _cr(self, stats, i):
        return _ratio(stats.a_clamped[i], stats.a_valid)

    def _nearest_exclude(self, given, centre, k=3):
        """find_nearest_localMLP_topK_exclude"""
        n = self.n_submaps
        if n - 1 == 0:
            return np.arange(n)
        if n - 1 <= k:
            return np.array([i for i in range(n) if i != given], np.int64)
        e = self.boxes[:, :3] - np.asarray(centre, F32)[None]
        d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        d[given] = F32(100000.0)
        return np.argsort(d, kind="stable")[:k]

    def _most_overlapping(self, stats, ids):
        """find_highest_containing_ratio: the highest lattice-B score, the first of equals"""
        return int(ids[np.argsort(-stats.b_raw[ids], kind="stable")[0]])

    def _normal(self, ctx, active, force):
        """process_keyframe_normal"""
        stats, ratios = ctx["stats"], ctx["ratios"]
        nearest = self._nearest_exclude(active, ctx["surface"][:3])
        mo = self._most_overlapping(stats, nearest)
        cr_mo = ratios["cr_mo"] = self._cr(stats, mo)
        same = active == mo
        cr_active = ratios["cr_active"] = self._cr(stats, active)
        if force or cr_active >= self.thr:                                   # case 1
            if not same and cr_mo >= self.thr_mo:
                switch = self._double_binding(ctx, active, mo, cr_mo)
                flag = self._msg1(ctx, active, mo, switch)
                return flag, "double binding, active submap switch" if switch else "double binding, unchanged"
            flag = self._msg2(ctx, active)
            self.double_binding_counter = 0
            return flag, "unchanged"
        cr_new = ratios["cr_active_new"] = _ratio(stats.a_expanded[active], stats.a_valid)
        if cr_new >= self.thr:                                               # case 2
            if not same and cr_mo >= self.thr_mo:
                switch = self._double_binding(ctx, active, mo, cr_mo)
                flag = self._msg1(ctx, active, mo, switch)
                return flag, "double binding, active submap switch" if switch else "double binding, expanded"
            flag = self._msg2(ctx, active)
            self.double_binding_counter = 0
            return flag, "expanded"
        self.double_binding_counter = 0
        if same or cr_mo < self.thr_back:                                    # cases 3 and 4
            flag, _ = self._msg3(ctx, active)
            self.wait_loop = False
            return flag, "new localMLP"
        switch = self._find_overlapping_region(ctx, active, mo)              # case 5
        if switch:
            flag = self._msg1(ctx, active, mo, True)
            self.wait_loop = False
            return flag, "switch to prev"
        flag, new = self._msg3(ctx, active)
        self.wait_loop, self.id_wait, self.id_actual = True, mo, new
        return flag, "wait loop, new localMLP"

    def _wait_loop(self, ctx, active, force):
        """process_keyframe_wait_loop"""
        cr_wt = ctx["ratios"]["cr_wait"] = self._cr(ctx["stats"], self.id_wait)
        if force or cr_wt < self.thr_back:
            return self._normal(ctx, active, force)
        if not self._loop_flag(ctx, self.id_wait, active, cr_wt):
            return self._normal(ctx, active, force)
        return self._msg1(ctx, active, self.id_wait, True), "switch to prev"

    def _loop_flag(self, ctx, mo, active, cr_mo, force_detect=False):
        """get_loop_flag"""
        if force_detect or (self.wait_loop and self.id_wait == mo and self.id_actual == active):
            if cr_mo >= self.thr_back and self._find_overlapping_region(ctx, active, mo):
                self.wait_loop = False
                return True
        return False

    def _double_binding(self, ctx, active, mo, cr_mo):
        """process_double_binding"""
        switch = False
        if self.double_binding_counter == 0:
            self.double_binding_counter += 1
            self.db_active, self.db_mo = active, mo
        elif active == self.db_active and mo == self.db_mo:
            if self.double_binding_counter >= self.thres_db_time:
                switch = self._loop_flag(ctx, mo, active, cr_mo, force_detect=True)
                self.double_binding_counter = 0
            else:
                self.double_binding_counter += 1
        else:
            self.double_binding_counter = 0
            self.db_active, self.db_mo = active, mo
        return switch

    def _find_overlapping_region(self, ctx, active, target):
        """find_overlapping_region: the related keyframes of ``target`` that are not bound to ``active``, the nearest ten of
        them, the frame's lattice-C points they see inside the target's box, and -- with enough of those -- the rectification"""
        kfs = self.keyframe_submaps[:self.n_keyframes]
        related = np.nonzero((kfs == target).any(1) & ~(kfs == active).any(1))[0]
        top, res = self._overlap(ctx["rows"], ctx["pose_world"], target, related, self.keyframe_world_poses(related))
        ctx["overlap"] = {"target_d": res["target_d"], "rays_d_cam": res["rays_d_cam"], "mask_final": res["mask_final"],
                          "kf_ids": np.asarray(top, np.int64), "top_kf_masks": res["top_kf_masks"], "count": res["count"]}
        if res["count"] < self.min_pts:
            return False
        # current_pose_switch_submap
        world = _matmul(self.kf_world[self.first_kf[active]], ctx["pose_local"])
        pose_ini = _matmul(_inverse(self.kf_world[self.first_kf[target]]), world)
        flag, _, pose = self.rectify(ctx["rows"], pose_ini, ctx["pose_local"].copy(), target, active, np.asarray(top, np.int64),
                                     res["top_kf_masks"])
        if flag:
            ctx["rectified"] = np.ascontiguousarray(pose.cpu().numpy() if torch.is_tensor(pose) else pose, F32).reshape(4, 4)
        return bool(flag)

    def _expanded(self, ctx, i, stale=False):
        """localMLP_expand_rule(box_i, surface box, max_len_i): the record's, or the host build of the same header when max_len_i
        changed after the record was made"""
        if stale:
            return sc.expand_rule(self.boxes[i], ctx["surface"], self.max_len[i])[0]
        return ctx["stats"].expanded[i]

    def _msg1(self, ctx, id1, id2, switch):
        """send_msg1: the keyframe is bound to two sub-maps"""
        kf = ctx["kf"]
        if switch:
            self.max_len[id2] = self.max_len_back
        new1 = self._expanded(ctx, id1)
        new2 = self._expanded(ctx, id2, stale=True) if switch else self.boxes[id2].copy()
        self.keyframe_submaps[kf] = (id2, id1) if switch else (id1, id2)
        self.boxes[id1], self.boxes[id2] = new1, new2
        self._adjacent(id1, id2)
        self.keyframe_ref[kf] = -2
        if switch:
            self.prev_active, self.active = self.active, id2
            return 1
        return 2

    def _msg2(self, ctx, i):
        """send_msg2: the keyframe is bound to the active sub-map alone"""
        row = self.keyframe_submaps[ctx["kf"]]
        row[0 if row[0] == -1 else 1] = i
        self.boxes[i] = self._expanded(ctx, i)
        return 2

    def _msg3(self, ctx, active):
        """send_msg3: a new sub-map whose box is the frame's surface box (localMLP_create_rule)"""
        kf = ctx["kf"]
        new = self._new_submap(ctx["surface"], kf)
        self.keyframe_submaps[kf] = (new, active)
        self._adjacent(active, new)
        self.prev_active, self.active = self.active, new
        self.keyframe_ref[kf] = -1
        self.kf_world[kf], self.kf_local[kf] = ctx["pose_world"], np.eye(4, dtype=F32)
        return 3, new


def derive_schedule(frames, poses_world, cfg, intrinsics, device="cuda", rectify=None, backend="hip", switch_interval=None,
                    image_hw=None, return_manager=False, **manager_kw):
    """Walk the keyframes of a sequence with the given world poses -> (schedule, trace): the ``{frame: ("new",) | ("back", s)}``
    dictionary ``GraphedSequence(schedule=...)`` takes, and the list of Decisions.  frames: the dictionaries ``synth`` renders
    (``direction`` [H,W,3], ``rgb`` [H,W,3], ``depth`` [H,W]) or ray rows [H*W,7]; ``force`` as mipsfusion.py:691 sets it:
    frame - last_switch_frame <= tracking.switch_interval.  image_hw: (H, W) when the frames are rows.  return_manager: also
    return the SubmapManager (its ``bindings()`` feed ``pose_graph.adjacent_pairs``)."""
    every = int(cfg["mapping"]["keyframe_every"])
    if switch_interval is None:
        switch_interval = cfg.get("tracking", {}).get("switch_interval", 0)

    def rows_of(f):
        if isinstance(f, dict):
            f = torch.cat([f["direction"], f["rgb"], f["depth"][..., None]], -1).reshape(-1, 7)
        f = torch.as_tensor(f, dtype=torch.float32)
        return f.to(device) if backend == "hip" else f
    first = frames[0]
    if not isinstance(first, dict) and image_hw is None:
        raise ValueError("derive_schedule: image_hw=(H, W) when the frames are ray rows")
    H, W = first["depth"].shape if isinstance(first, dict) else image_hw
    mgr = SubmapManager(cfg, H, W, intrinsics, device=device, rectify=rectify, backend=backend, **manager_kw)
    world = [np.ascontiguousarray(torch.as_tensor(p).detach().cpu().numpy(), F32) for p in poses_world]
    mgr.first_keyframe(rows_of(frames[0]), world[0])
    schedule, trace, last_switch = {}, [], 0
    for k in range(every, len(frames), every):
        local = _matmul(_inverse(mgr.kf_world[mgr.first_kf[mgr.active]]), world[k])
        d = mgr.process_keyframe(rows_of(frames[k]), local, k, force=(k - last_switch) <= switch_interval, pose_world=world[k])
        trace.append(d)
        if d.flag == 3:
            schedule[k], last_switch = ("new",), k
        elif d.flag == 1:
            schedule[k], last_switch = ("back", d.active), k
    return (schedule, trace, mgr) if return_manager else (schedule, trace)
