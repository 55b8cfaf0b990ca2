"""Times the brick-sparse TSDF volume (mipsfusion_amd/sparse_tsdf.py) beside the dense one on one GPU: the marched
128^3 box room seen from 64 views of 460 x 620 pixels (tools/tsdf_time.py's scene), first at 256^3 voxels, which both volumes
take, then at a resolution whose grid the dense volume refuses.

    python tools/sparse_time.py [--reps 7] [--res 256] [--big 1536] [--views 64] [--out file.json]

Milliseconds between two events on the stream after one warm-up call, median of --reps; the state is zeroed, untimed, before every
repeat of a call that changes it:
  allocate             mipsf_sparse_allocate of all views (marks, the prefix sum over the brick table, the slots)
  integrate            mipsf_sparse_integrate after it, beside mipsf_tsdf_integrate
  raycast_1, _64       one view and all views, beside mipsf_track_raycast
  dense_march          to_dense() over the tight window and marching cubes on it, beside volume() and marching cubes; host wall time
                       with a synchronise (marching reads counts back)
  odometry_frame       one frame of the odometry on the fused volume: ray cast, registration (30 iterations enqueued), allocation,
                       fusion
and the bricks in use against the bricks of the grid, the pool's bytes against the dense state's.  The shader clock and package
power sampled across the timed regions are printed beside the times (bench.BoardSampler), the date too."""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import _lib, mesh as mesh_mod, mesh_render as mr, sparse_tsdf, synth, tsdf   # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402
from tools.tsdf_time import wall                                              # noqa: E402


def time_sparse(origin, voxel, dims, capacity, depth, poses, K, H, W, reps, dev, march_window=None):
    vol = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, 4 * voxel, capacity, device=dev)
    n = depth.shape[0]
    run = {"capacity_bricks": capacity, "bricks_of_the_grid": int(np.prod(vol.bricks)), "table_and_mark_bytes": 8 * int(np.prod(vol.bricks))}
    alloc = torch.empty(4, dtype=torch.int64, device=dev)
    rec = torch.empty(2, dtype=torch.int64, device=dev)
    run["allocate_ms"] = timed(lambda: vol.allocate_enqueue(depth, poses, K, record=alloc), reps, setup=vol.reset)
    run["allocate_one_view_ms"] = timed(lambda: vol.allocate_enqueue(depth[:1], poses[:1], K), reps, setup=vol.reset)
    marked, new, dropped, in_use = (int(x) for x in alloc.tolist())
    run.update(bricks_in_use=in_use, bricks_dropped=dropped, pool_bytes_in_use=in_use * 8192, pool_bytes_allocated=capacity * 8192)

    def fresh():
        vol.reset()
        vol.allocate_enqueue(depth, poses, K)
    run["integrate_ms"] = timed(lambda: vol.fuse_enqueue(depth, poses, K, record=rec), reps, setup=fresh)
    run["integrate_updates"], run["observed_voxels"] = (int(x) for x in rec.tolist())
    run["allocate_and_integrate_one_view_ms"] = timed(lambda: vol.integrate_enqueue(depth[:1], poses[:1], K), reps, setup=vol.reset)
    fresh()
    vol.fuse_enqueue(depth, poses, K)
    run["raycast_1_ms"] = timed(lambda: vol.raycast_enqueue(poses[:1], K, H, W), reps)
    run["raycast_64_ms"] = timed(lambda: vol.raycast_enqueue(poses, K, H, W), reps)
    run["raycast_1_hits"] = int(vol.raycast_enqueue(poses[:1], K, H, W).hits[0])
    window = vol.tight_window() if march_window is None else march_window
    run["march_window"] = [list(window[0]), list(window[1])]
    run["to_dense_ms"] = timed(lambda: vol.to_dense(*window), reps)
    run["dense_march_ms"] = wall(lambda: mesh_mod.marching_cubes(vol.to_dense(*window).volume(), 0.0, truncation=1.0, return_device=True), 3)
    run["faces"] = int(len(vol.extract_mesh(window=window).faces))

    def frame():
        _, pose = vol.track_enqueue(depth[1], K, poses[0])
        vol.integrate_enqueue(depth[1:2], pose[None], K)
    run["odometry_frame_ms"] = timed(frame, reps)
    return run


def time_dense(origin, voxel, dims, depth, poses, K, H, W, reps, dev):
    vol = tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, device=dev)
    rec = torch.empty(2, dtype=torch.int64, device=dev)
    run = {"state_bytes": 8 * int(np.prod(dims)), "bricks_of_the_grid": int(np.prod([-(-d // b) for d, b in zip(dims, _lib.TSDF_BRICK)]))}
    run["integrate_ms"] = timed(lambda: vol.integrate_enqueue(depth, poses, K, record=rec), reps, setup=vol.reset)
    run["integrate_updates"], run["observed_voxels"] = (int(x) for x in rec.tolist())
    run["integrate_one_view_ms"] = timed(lambda: vol.integrate_enqueue(depth[:1], poses[:1], K), reps, setup=vol.reset)
    vol.reset()
    vol.integrate_enqueue(depth, poses, K)
    run["raycast_1_ms"] = timed(lambda: vol.raycast_enqueue(poses[:1], K, H, W), reps)
    run["raycast_64_ms"] = timed(lambda: vol.raycast_enqueue(poses, K, H, W), reps)
    run["raycast_1_hits"] = int(vol.raycast_enqueue(poses[:1], K, H, W).hits[0])
    run["dense_march_ms"] = wall(lambda: mesh_mod.marching_cubes(vol.volume(), 0.0, truncation=1.0, return_device=True), 3)
    run["faces"] = int(len(vol.extract_mesh().faces))

    def frame():
        _, pose = vol.track_enqueue(depth[1], K, poses[0])
        vol.integrate_enqueue(depth[1:2], pose[None], K)
    run["odometry_frame_ms"] = timed(frame, reps)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--big", type=int, default=1536)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth, _ = mr.render_mesh_depth(marched, poses, K, H, W)
    res = {"date": datetime.date.today().isoformat(), "image": [H, W], "views": args.views, "trunc_voxels": 4, "band": "trunc", "reps": args.reps, "runs": {}}
    with BoardSampler(dev.index or 0) as board:
        for name, side in (("both", args.res), ("sparse_only", args.big)):
            voxel = float((hi - lo + 0.5).max() / (side - 1))
            origin = centre - 0.5 * voxel * (side - 1)
            dims = (side,) * 3
            run = {"dims": list(dims), "voxel_m": round(voxel, 5), "voxels": side ** 3}
            if side ** 3 <= _lib.TSDF_MAX_VOXELS:
                run["dense"] = time_dense(origin, voxel, dims, depth, poses, K, H, W, args.reps, dev)
                run["sparse"] = time_sparse(origin, voxel, dims, 16384, depth, poses, K, H, W, args.reps, dev)
            else:
                try:
                    tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, device=dev)
                    run["dense"] = "accepted"
                except ValueError as e:
                    run["dense"] = f"refused: {e}"
                corner = tuple(int(x) for x in np.minimum(np.asarray(dims), 512))
                run["sparse"] = time_sparse(origin, voxel, dims, _lib.SPARSE_MAX_CAPACITY, depth, poses, K, H, W, args.reps, dev, ((0, 0, 0), corner))
            res["runs"][name] = run
            torch.cuda.empty_cache()
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
