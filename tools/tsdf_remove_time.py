"""Times the removal of fused views (mipsfusion_amd/tsdf.py deintegrate and reintegrate) on one GPU beside the fusion
it undoes: a 256^3 volume over the marched 128^3 box room, 256 views of 460 x 620 pixels rendered by render_mesh_depth, of which
every fourth is the one that moves (64 views).

    python tools/tsdf_remove_time.py [--reps 5] [--res 256] [--views 256] [--every 4] [--out file.json]

Milliseconds between two events on the stream after one warm-up call, median of --reps; the state every timed call starts from is
put back, untimed, before every repeat.  Without and with colour:
  deintegrate          mipsf_deintegrate_views of the 64 views, out of the volume that holds all 256
  integrate            mipsf_tsdf_integrate of the same 64, into the volume that holds the other 192
  reintegrate          reintegrate_enqueue of the 64: removed at poses 0.03 rad and (6, -4, 5) cm off, fused where they belong
  reset_and_fuse_all   reset() and mipsf_tsdf_integrate of all 256, what the volume had to pay before
  reintegrate_wall     TSDFVolume.reintegrate given all 256 views: the selection on the host, the gather of the moved views, the two
                       launches and the read-back; host wall time with a synchronise
The shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import mesh_render as mr, synth, tsdf                     # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402


def drifted(poses, which, angle=0.03, shift=(0.06, -0.04, 0.05)):
    """the views `which` turned in place by `angle` about the world's z axis and moved by `shift`"""
    c, s = math.cos(angle), math.sin(angle)
    turn = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=poses.device)
    out = poses.double().clone()
    out[which, :3, :3] = turn @ out[which, :3, :3]
    out[which, :3, 3] += torch.tensor(shift, dtype=torch.float64, device=poses.device)
    return out.to(torch.float32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_remove_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth = torch.cat([mr.render_mesh_depth(marched, poses[k:k + 64], K, H, W)[0] for k in range(0, args.views, 64)])
    rays = synth.camera_rays(H, W, fx, fy, cx, cy).to(dev)
    voxel = float((hi - lo + 0.5).max() / (args.res - 1))
    origin = centre - 0.5 * voxel * (args.res - 1)
    dims = (args.res,) * 3
    moved = torch.arange(1, args.views, args.every, device=dev)
    stays = torch.ones(args.views, dtype=torch.bool, device=dev)
    stays[moved] = False
    kept = torch.nonzero(stays)[:, 0]
    wrong = drifted(poses, moved)
    res = {"image": [H, W], "views": args.views, "moved": int(moved.numel()), "dims": list(dims), "voxel_m": round(voxel, 5), "trunc_voxels": 4,
           "drift": {"angle_rad": 0.03, "shift_m": [0.06, -0.04, 0.05]}, "runs": {}}
    with BoardSampler(dev.index or 0) as board:
        for color in (False, True):
            vol = tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, color=color, device=dev)
            c3 = (0.5 + 0.5 * torch.sin(4.0 * rays[None] * depth[..., None])).contiguous() if color else None   # any smooth colour
            pick = lambda t, idx: None if t is None else t[idx].contiguous()                                    # noqa: E731
            d_m, p_m, w_m, c_m = depth[moved].contiguous(), poses[moved].contiguous(), wrong[moved].contiguous(), pick(c3, moved)
            words = [t for t in (vol.tsdf, vol.weight, vol.color) if t is not None]

            def fused(p_all, idx=None):
                """the state after fusing the views idx (all by default) at p_all, as copies"""
                vol.reset()
                if idx is None:
                    vol.integrate_enqueue(depth, p_all, K, c3)
                else:
                    vol.integrate_enqueue(depth[idx].contiguous(), p_all[idx].contiguous(), K, pick(c3, idx))
                return [t.clone() for t in words]

            def put(state):
                for t, s in zip(words, state):
                    t.copy_(s)
            full, rest, stale = fused(poses), fused(poses, kept), fused(wrong)
            gone, back = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
            run = {}
            run["deintegrate_ms"] = timed(lambda: vol.deintegrate_enqueue(d_m, p_m, K, c_m, record=gone), args.reps, setup=lambda: put(full))
            run["deintegrate_counts"] = gone.tolist()
            run["weights_equal_the_fusion_of_the_rest"] = bool(torch.equal(vol.weight, rest[1]))
            run["tsdf_within"] = float((vol.tsdf.double() - rest[0].double()).abs().max())
            run["integrate_ms"] = timed(lambda: vol.integrate_enqueue(d_m, p_m, K, c_m, record=back), args.reps, setup=lambda: put(rest))
            run["integrate_counts"] = back.tolist()
            run["deintegrate_over_integrate"] = round(run["deintegrate_ms"] / run["integrate_ms"], 3)
            run["reintegrate_ms"] = timed(lambda: vol.reintegrate_enqueue(d_m, w_m, p_m, K, c_m, records=(gone, back)), args.reps, setup=lambda: put(stale))
            run["reintegrate_counts"] = gone.tolist() + back.tolist()
            run["weights_equal_the_fresh_fusion"] = bool(torch.equal(vol.weight, full[1]))
            run["tsdf_within_of_fresh"] = float((vol.tsdf.double() - full[0].double()).abs().max())

            def again():
                vol.reset()
                vol.integrate_enqueue(depth, poses, K, c3, record=back)
            run["reset_and_fuse_all_ms"] = timed(again, args.reps)
            run["fuse_all_over_reintegrate"] = round(run["reset_and_fuse_all_ms"] / run["reintegrate_ms"], 2)
            took = []
            for _ in range(3):                                                 # the first one is the warm-up
                put(stale)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                counts = vol.reintegrate(depth, wrong, poses, K, c3)
                torch.cuda.synchronize()
                took.append((time.perf_counter() - t0) * 1e3)
            run["reintegrate_wall_ms"] = round(float(np.median(took[1:])), 3)
            run["reintegrate_wall_views_moved"] = counts.views_moved
            res["runs"]["colour" if color else "plain"] = run
            del vol, words, full, rest, stale, c3, c_m
            torch.cuda.empty_cache()
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
