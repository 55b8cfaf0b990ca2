"""Times the removal of fused views from the brick-sparse volume (mipsfusion_amd/sparse_tsdf.py history, deintegrate and reintegrate,
DESIGN.md 4.27) on one GPU beside the sparse fusion it undoes, on the scenes of tools/sparse_time.py: the marched 128^3 box room
seen from 256 views of 460 x 620 pixels, in a virtual grid of 256^3 voxels and in one of 1536^3, which no dense volume holds.  Every
fourth view is the one that moves (64 views).

    python tools/sparse_remove_time.py [--reps 5] [--res 256] [--big 1536] [--views 256] [--every 4] [--out file.json]

Milliseconds between two events on the stream after one warm-up call, median of --reps; the state every timed call starts from
(table, slots, history and pool) is put back, untimed, before every repeat:
  deintegrate          mipsf_sparse_deintegrate of the 64 views, out of the volume that holds all 256
  fuse                 mipsf_sparse_integrate of the same 64, into the volume that holds the other 192 (allocated and stamped, untimed)
  integrate            integrate_enqueue of the same 64 into the same volume: allocation, stamp and fusion
  reintegrate          reintegrate_enqueue of the 64: removed at poses 0.03 rad and (6, -4, 5) cm off, allocated for and fused where
                       they belong
  reset_and_fuse_all   reset() and integrate_enqueue of all 256, what the volume had to pay before
  stamp                mipsf_sparse_stamp alone (its two launches), and integrate_enqueue of one view with history beside the same
                       call on a volume made without
The shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler), the date too."""
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
from mipsfusion_amd import mesh_render as mr, sparse_tsdf, synth              # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402
from tools.tsdf_remove_time import drifted                                    # noqa: E402


def time_scene(origin, voxel, dims, capacity, depth, poses, wrong, moved, kept, K, reps, dev):
    vol = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, 4 * voxel, capacity, device=dev, history=True)
    plain = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, 4 * voxel, capacity, device=dev)
    n = depth.shape[0]
    d_m, p_m, w_m = depth[moved].contiguous(), poses[moved].contiguous(), wrong[moved].contiguous()
    ids_m = moved.to(torch.int32).contiguous()                 # fused in one call: the id of a view is its position
    words = [vol.table, vol.slot_brick, vol.count, vol.born, vol.serial, vol.tsdf, vol.weight]

    def fused(p_all, idx=None):
        """the state after fusing the views idx (all by default) at p_all, as copies, with the host's count of views"""
        vol.reset()
        if idx is None:
            rec, alloc = vol.integrate_enqueue(depth, p_all, K)
        else:
            rec, alloc = vol.integrate_enqueue(depth[idx].contiguous(), p_all[idx].contiguous(), K)
        return [t.clone() for t in words], vol.views_fused, rec.tolist(), alloc.tolist()

    def put(state):
        for t, s in zip(words, state[0]):
            t.copy_(s)
        vol.views_fused = state[1]
    full, rest, stale = fused(poses), fused(poses, kept), fused(wrong)
    run = {"capacity_bricks": capacity, "bricks_of_the_grid": int(np.prod(vol.bricks)), "bricks_in_use": full[3][3], "bricks_dropped": full[3][2],
           "fuse_all_counts": full[2]}
    gone = torch.empty(5, dtype=torch.int64, device=dev)
    back = torch.empty(2, dtype=torch.int64, device=dev)
    run["deintegrate_ms"] = timed(lambda: vol.deintegrate_enqueue(d_m, p_m, K, ids_m, record=gone), reps, setup=lambda: put(full))
    run["deintegrate_counts"] = gone.tolist()

    def ready():
        put(rest)
        vol.allocate_enqueue(d_m, p_m, K)
        vol.stamp_enqueue(d_m.shape[0])
    run["fuse_ms"] = timed(lambda: vol.fuse_enqueue(d_m, p_m, K, record=back), reps, setup=ready)
    run["fuse_counts"] = back.tolist()
    run["deintegrate_over_fuse"] = round(run["deintegrate_ms"] / run["fuse_ms"], 3)
    run["integrate_ms"] = timed(lambda: vol.integrate_enqueue(d_m, p_m, K), reps, setup=lambda: put(rest))
    out = []

    def both():
        out[:] = vol.reintegrate_enqueue(d_m, w_m, p_m, K, ids_m)
    run["reintegrate_ms"] = timed(both, reps, setup=lambda: put(stale))
    run["reintegrate_counts"] = [r.tolist() for r in out]
    run["observed_after_reintegrate_and_fresh"] = [int((vol.weight > 0).sum()), int((full[0][6] > 0).sum())]

    def again():
        vol.reset()
        vol.integrate_enqueue(depth, poses, K)
    run["reset_and_fuse_all_ms"] = timed(again, reps)
    run["fuse_all_over_reintegrate"] = round(run["reset_and_fuse_all_ms"] / run["reintegrate_ms"], 2)
    # the stamp: alone, and as the difference it makes to one frame
    put(full)
    run["stamp_ms"] = timed(lambda: vol.stamp_enqueue(1), reps, setup=lambda: put(full))
    plain.integrate_enqueue(depth, poses, K)
    frame_d, frame_p = depth[n - 1:].contiguous(), poses[n - 1:].contiguous()
    run["integrate_one_view_with_history_ms"] = timed(lambda: vol.integrate_enqueue(frame_d, frame_p, K), reps, setup=lambda: put(full))
    run["integrate_one_view_without_ms"] = timed(lambda: plain.integrate_enqueue(frame_d, frame_p, K), reps)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--big", type=int, default=1536)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_remove_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth = torch.cat([mr.render_mesh_depth(marched, poses[k:k + 64], K, H, W)[0] for k in range(0, args.views, 64)])
    moved = torch.arange(1, args.views, args.every, device=dev)
    stays = torch.ones(args.views, dtype=torch.bool, device=dev)
    stays[moved] = False
    kept = torch.nonzero(stays)[:, 0]
    wrong = drifted(poses, moved)
    res = {"date": datetime.date.today().isoformat(), "image": [H, W], "views": args.views, "moved": int(moved.numel()), "trunc_voxels": 4, "band": "trunc",
           "reps": args.reps, "drift": {"angle_rad": 0.03, "shift_m": [0.06, -0.04, 0.05]}, "runs": {}}
    with BoardSampler(dev.index or 0) as board:
        for name, side, capacity in (("256", args.res, 16384), ("1536", args.big, 262144)):
            voxel = float((hi - lo + 0.5).max() / (side - 1))
            origin = centre - 0.5 * voxel * (side - 1)
            run = {"dims": [side] * 3, "voxel_m": round(voxel, 5), "voxels": side ** 3}
            run.update(time_scene(origin, voxel, (side,) * 3, capacity, depth, poses, wrong, moved, kept, K, args.reps, dev))
            res["runs"][name] = run
            torch.cuda.empty_cache()
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
