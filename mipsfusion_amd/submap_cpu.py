"""numpy float32 restatement of csrc/submap.hip (C ABI: include/mipsf_submap.h), with the operation order spelled
out.  ``SubmapManager(backend="cpu")`` computes its records with it, and tests/submap_cpu.py is this module: the device kernels
are held to it word for word, and it is held to the reference's own ``Manager`` functions on the CPU (tests/test_submap_cpu.py).

The expand rule is NOT restated here: ``expand_rule`` calls the host build of csrc/submap_dev.h, the header the device compiles.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

F32 = np.float32
HALF = np.float32(0.5)
HEADER_WORDS, BOX_WORDS, MAX_BOXES, MAX_TOP_KF = 16, 12, 64, 10
TPB, WAVE = 256, 64                      # the workgroup whose summation order lattice_sum restates
CASE_NAMES = ("contained", "full", "free", "positive", "negative", "both")

_HOST = None


def _host():
    global _HOST
    if _HOST is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmipsf_hostrng.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C mipsfusion_amd/csrc`")
        lib = C.CDLL(path)
        lib.mipsf_submap_expand_host.restype = C.c_uint32
        lib.mipsf_submap_expand_host.argtypes = [C.c_void_p] * 4
        _HOST = lib
    return _HOST


class FrameStats(NamedTuple):
    n_valid: int                # pixels with near < depth < far
    smin: np.ndarray            # float32 [3] (+inf without a valid pixel)
    smax: np.ndarray            # float32 [3] (-inf)
    a_valid: int                # lattice A points with depth > 0
    c_sum: np.ndarray           # float64 [3] sum of the lattice C points
    expanded: np.ndarray        # float32 [n,6] localMLP_expand_rule(box_i, surface box, max_len_i)
    a_clamped: np.ndarray       # int64 [n] lattice A, depth > 0, inside box_i with lengths clamped below by min_cr_len
    a_expanded: np.ndarray      # int64 [n] lattice A, depth > 0, inside the expanded box
    b_raw: np.ndarray           # int64 [n] lattice B, no depth mask, inside box_i
    cases: np.ndarray           # uint32 [n] the expand rule's case per axis, axis a in bits 8a..8a+7

    @property
    def surface(self):
        """get_frame_surface_bbox: (centre, length) float32 [3] each"""
        length = self.smax - self.smin
        return self.smin + HALF * length, length


def stats_to_words(s: FrameStats) -> np.ndarray:
    """the record of include/mipsf_submap.h, uint32 [16 + 12 n]"""
    n = len(s.cases)
    w = np.zeros(HEADER_WORDS + BOX_WORDS * n, np.uint32)
    w[0] = s.n_valid
    w[1:4] = np.asarray(s.smin, F32).view(np.uint32)
    w[4:7] = np.asarray(s.smax, F32).view(np.uint32)
    w[7] = s.a_valid
    w[8:14] = np.asarray(s.c_sum, np.float64).view(np.uint32)
    w[14] = n
    b = w[HEADER_WORDS:].reshape(n, BOX_WORDS)
    b[:, 0:6] = np.ascontiguousarray(s.expanded, F32).view(np.uint32)
    b[:, 6], b[:, 7], b[:, 8], b[:, 9] = s.a_clamped, s.a_expanded, s.b_raw, s.cases
    return w


def stats_from_words(w: np.ndarray) -> FrameStats:
    w = np.ascontiguousarray(w, np.uint32)
    n = int(w[14])
    b = w[HEADER_WORDS:HEADER_WORDS + BOX_WORDS * n].reshape(n, BOX_WORDS)
    return FrameStats(int(w[0]), w[1:4].copy().view(F32), w[4:7].copy().view(F32), int(w[7]), w[8:14].copy().view(np.float64),
                      np.ascontiguousarray(b[:, 0:6]).view(F32), b[:, 6].astype(np.int64), b[:, 7].astype(np.int64),
                      b[:, 8].astype(np.int64), b[:, 9].copy())


# ------------------------------------------------------------------------------------------------------------- the pieces
def lattice(H: int, W: int, num_h: int, num_w: int):
    """sample_pixels_uniformly as index arithmetic -> (rows int64 [num_h*num_w], cols)"""
    if not (1 <= num_h <= H and 1 <= num_w <= W):
        raise ValueError(f"lattice {num_h} x {num_w} is larger than the image {H} x {W}")
    ih, oh = (H - num_h) // (num_h + 1), (H - num_h) % (num_h + 1)
    iw, ow = (W - num_w) // (num_w + 1), (W - num_w) % (num_w + 1)
    r = np.arange(num_h, dtype=np.int64) * (ih + 1) + (ih + oh // 2)
    c = np.arange(num_w, dtype=np.int64) * (iw + 1) + (iw + ow // 2)
    return np.repeat(r, num_w), np.tile(c, num_h)


def lattice_pixels(H, W, num_h, num_w):
    r, c = lattice(H, W, num_h, num_w)
    return r * W + c


def world_points(rows: np.ndarray, pose: np.ndarray) -> np.ndarray:
    """p[i] = t[i] + ((x*R[i,0] + y*R[i,1]) + z*R[i,2]) * depth, float32 -> [n,3]"""
    rows, pose = np.asarray(rows, F32), np.asarray(pose, F32)
    x, y, z, d = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 6]
    out = np.empty((len(rows), 3), F32)
    for i in range(3):
        dw = (x * pose[i, 0] + y * pose[i, 1]) + z * pose[i, 2]
        out[:, i] = pose[i, 3] + dw * d
    return out


def inside(p: np.ndarray, centre: np.ndarray, length: np.ndarray) -> np.ndarray:
    """strictly inside centre -+ 0.5 length, the faces formed in float32 (pts_in_bbox)"""
    centre, length = np.asarray(centre, F32), np.asarray(length, F32)
    lo, hi = centre - HALF * length, centre + HALF * length
    return ((p > lo) & (p < hi)).all(-1)


def expand_rule(box, surface, max_len):
    """Manager.localMLP_expand_rule through the host build of csrc/submap_dev.h -> (float32 [6] centre + length, cases uint32)"""
    box, surface, max_len = (np.ascontiguousarray(v, F32).reshape(-1) for v in (box, surface, max_len))
    out = np.zeros(6, F32)
    cases = _host().mipsf_submap_expand_host(box.ctypes.data, surface.ctypes.data, max_len.ctypes.data, out.ctypes.data)
    return out, np.uint32(cases)


def case_of(cases, axis: int) -> int:
    return (int(cases) >> (8 * axis)) & 0xFF


def tree_sum(values: np.ndarray) -> np.ndarray:
    """float64 [n,c] -> [c] in the order of the kernels: thread t of 256 adds values t, t + 256, .. in that order; the 64 lanes of
    a wave combine by the butterfly 32, 16, .. 1; the four waves add up in ascending order."""
    values = np.asarray(values, np.float64)
    acc = np.zeros((TPB, values.shape[1]), np.float64)
    for r in range(0, len(values), TPB):
        chunk = values[r:r + TPB]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    v = acc.reshape(TPB // WAVE, WAVE, -1)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    total = v[0, 0]
    for w in range(1, TPB // WAVE):
        total = total + v[w, 0]
    return total


def lattice_sum(rows, pose, H, W, lat) -> np.ndarray:
    return tree_sum(world_points(np.asarray(rows, F32)[lattice_pixels(H, W, *lat)], pose).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------- the two calls
def frame_stats(rows, pose, boxes, max_len, H, W, lat_a, lat_b, lat_c, near, far, min_cr_len) -> FrameStats:
    """mipsf_submap_frame_stats.  rows [H*W,7], pose [4,4], boxes [n,6] (centre, length), max_len [n,3]."""
    rows = np.ascontiguousarray(rows, F32).reshape(H * W, 7)
    pose = np.asarray(pose, F32)
    boxes, max_len = np.asarray(boxes, F32).reshape(-1, 6), np.asarray(max_len, F32).reshape(-1, 3)
    n = len(boxes)
    if not 1 <= n <= MAX_BOXES or len(max_len) != n:
        raise ValueError(f"{n} sub-maps, accepted are 1 .. {MAX_BOXES}")
    min_cr_len = np.asarray(min_cr_len, F32)
    d = rows[:, 6]
    valid = (d > F32(near)) & (d < F32(far))
    pts = world_points(rows[valid], pose)
    if len(pts):
        smin, smax = pts.min(0), pts.max(0)
    else:
        smin, smax = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    with np.errstate(invalid="ignore"):
        s_len = smax - smin
        surface = np.concatenate([smin + HALF * s_len, s_len])
    rows_a = rows[lattice_pixels(H, W, *lat_a)]
    keep = rows_a[:, 6] > F32(0)
    pts_a = world_points(rows_a[keep], pose)
    pts_b = world_points(rows[lattice_pixels(H, W, *lat_b)], pose)
    expanded, cases = np.zeros((n, 6), F32), np.zeros(n, np.uint32)
    a_clamped, a_expanded, b_raw = (np.zeros(n, np.int64) for _ in range(3))
    for i in range(n):
        centre, length = boxes[i, :3], boxes[i, 3:]
        expanded[i], cases[i] = expand_rule(boxes[i], surface, max_len[i])
        a_clamped[i] = np.count_nonzero(inside(pts_a, centre, np.where(length < min_cr_len, min_cr_len, length)))
        a_expanded[i] = np.count_nonzero(inside(pts_a, expanded[i, :3], expanded[i, 3:]))
        b_raw[i] = np.count_nonzero(inside(pts_b, centre, length))
    return FrameStats(int(np.count_nonzero(valid)), smin, smax, int(np.count_nonzero(keep)), lattice_sum(rows, pose, H, W, lat_c),
                      expanded, a_clamped, a_expanded, b_raw, cases)


def overlap_distances(rows, pose, H, W, lat, table, slots, poses) -> np.ndarray:
    """phase (a) of mipsf_submap_overlap -> float64 [n]"""
    table = np.asarray(table, F32)
    centre = lattice_sum(rows, pose, H, W, lat) / np.float64(lat[0] * lat[1])
    out = np.empty(len(slots), np.float64)
    for j, (slot, M) in enumerate(zip(slots, np.asarray(poses, F32).astype(np.float64))):
        if not 0 <= int(slot) < len(table):
            out[j] = np.nan
            continue
        kf = table[int(slot)]
        m = tree_sum((kf[:, :3] * kf[:, 6:7]).astype(np.float64)) / np.float64(len(kf))
        q = np.float64(0.0)
        for i in range(3):
            w = ((m[0] * M[i, 0] + m[1] * M[i, 1]) + m[2] * M[i, 2]) + M[i, 3]
            e = w - centre[i]
            q = q + e * e
        out[j] = np.sqrt(q)
    return out


def overlap_camera_points(points, poses):
    """the lattice points in each chosen camera, float64 [k,P,3]: rigid inverse R^T, -(R^T t) in the kernel's order"""
    p = np.asarray(points, F32).astype(np.float64)
    out = np.empty((len(poses), len(p), 3), np.float64)
    for kk, M in enumerate(np.asarray(poses, F32).astype(np.float64)):
        for i in range(3):
            t_inv = -((M[0, i] * M[0, 3] + M[1, i] * M[1, 3]) + M[2, i] * M[2, 3])
            out[kk, :, i] = ((M[0, i] * p[:, 0] + M[1, i] * p[:, 1]) + M[2, i] * p[:, 2]) + t_inv
    return out


def overlap_project(cam, fx, fy, cx, cy):
    """project_to_pixel (x negated, z + 1e-5) in float64 -> u, v"""
    zz = cam[..., 2] + 1e-5
    return (fx * (-cam[..., 0]) + cx * cam[..., 2]) / zz, (fy * cam[..., 1] + cy * cam[..., 2]) / zz


def overlap_masks(rows, pose, H, W, lat, top_poses, target_box, fx, fy, cx, cy, cam_W, cam_H, edge=20.0):
    """phase (b) -> dict(top_kf_masks bool [k,P], mask_final bool [P], count, target_d float32 [P], rays_d_cam float32 [P,3])"""
    top_poses = np.asarray(top_poses, F32).reshape(-1, 4, 4)
    if len(top_poses) > MAX_TOP_KF:
        raise ValueError(f"{len(top_poses)} chosen keyframes, accepted are at most {MAX_TOP_KF}")
    sel = np.ascontiguousarray(rows, F32).reshape(H * W, 7)[lattice_pixels(H, W, *lat)]
    pts = world_points(sel, pose)
    cam = overlap_camera_points(pts, top_poses)
    u, v = overlap_project(cam, float(fx), float(fy), float(cx), float(cy))
    seen = (u < cam_W - edge) & (u > edge) & (v < cam_H - edge) & (v > edge) & (cam[..., 2] < 0.0)
    box = np.asarray(target_box, F32)
    final = seen.any(0) & inside(pts, box[:3], box[3:])
    return {"top_kf_masks": seen, "mask_final": final, "count": int(np.count_nonzero(final)), "target_d": sel[:, 6].copy(),
            "rays_d_cam": sel[:, :3].copy()}
