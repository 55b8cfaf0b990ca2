"""Times the TSDF tracker's model side (mipsfusion_amd/tsdf.py) on one GPU: a 256^3 volume of the box room fused from
64 views of 460 x 620 pixels (the set-up of tools/tsdf_time.py), then

    python tools/track_time.py [--reps 7] [--res 256] [--views 64] [--out file.json]

Milliseconds between two events on the stream after one warm-up call, median of --reps (min and max beside it):
  raycast_1, raycast_64       mipsf_track_raycast of one view and of all views, depth and normals, with the brick skipping and with
                              every sample evaluated (MIPSF_TRACK_NO_SKIP); rays per second are pixels over the time of the call
  register_10                 mipsf_track_register against one ray-cast view from a pose 2 degrees and 5 cm away, max_iteration 10,
                              relative_fitness = relative_rmse = 0 so that all 11 evaluations run
  register_color_10           mipsf_track_register_color on the same frame and pose against one view, cast with its
                              colour, of a second volume that fused the same views with the box room's texture 0.5 + 0.5 sin(4 x);
                              max_iteration 10 and relative_color_rmse = 0 as well, so that all 11 evaluations run; in the same run as
                              register_10, to be read beside it
  odometry_frame              what tsdf_odometry enqueues per frame: ray cast, registration (30 iterations at most, the default
                              stop), the selection of the pose and the fusion of the frame
  volume_march_render         the route to the same depth image without the ray caster: volume(), marching_cubes, render_mesh_depth
                              of one view; host wall time with a synchronise (marching reads counts back)
The shader clock and package power sampled across the timed regions (bench.BoardSampler) and the date are printed beside the times."""
import argparse
import datetime
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import _lib, mesh as mesh_mod, mesh_render as mr, synth, tsdf   # noqa: E402
from tools.raster_time import marched_room, view_poses                       # noqa: E402
from tools.tsdf_time import wall                                              # noqa: E402


def timed3(fn, reps, setup=None):
    """-> [median, min, max] ms between two events, after one warm-up call"""
    out = []
    for k in range(reps + 1):
        if setup is not None:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return [round(float(np.median(out)), 4), round(float(min(out)), 4), round(float(max(out)), 4)]


def texture(depth, poses, K):
    """the box room's texture at the points a depth image sees: depth [n,H,W], poses [n,4,4] on the device -> rgb fp32 [n,H,W,3]"""
    n, H, W = depth.shape
    fx, fy, cx, cy = K
    row, col = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32), torch.arange(W, device=depth.device, dtype=torch.float32),
                              indexing="ij")
    d_cam = torch.stack([(col - cx) / fx, -(row - cy) / fy, -torch.ones_like(col)], -1)
    d_world = torch.einsum("nrc,hwc->nhwr", poses[:, :3, :3], d_cam)
    hit = poses[:, None, None, :3, 3] + d_world * depth[..., None]
    return (0.5 + 0.5 * torch.sin(4.0 * hit)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth, _ = mr.render_mesh_depth(marched, poses, K, H, W)
    voxel = float((hi - lo + 0.5).max() / (args.res - 1))
    origin = centre - 0.5 * voxel * (args.res - 1)
    dims = (args.res,) * 3
    vol = tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, device=dev)
    vol.integrate_enqueue(depth, poses, K)
    res = {"date": datetime.date.today().isoformat(), "image": [H, W], "views": args.views, "dims": list(dims), "voxel_m": round(voxel, 5),
           "trunc_voxels": 4, "step_voxels": 2, "reps": args.reps, "ms": "median, min, max", "runs": {}}
    run = res["runs"]
    with BoardSampler(dev.index or 0) as board:
        for name, n in (("raycast_1", 1), (f"raycast_{args.views}", args.views)):
            for tag, flags in (("", 0), ("_no_skip", _lib.TRACK_NO_SKIP)):
                ms = timed3(lambda: vol.raycast_enqueue(poses[:n], K, H, W, flags=flags), args.reps)
                run[name + tag + "_ms"] = ms
                run[name + tag + "_rays_per_s"] = float(f"{n * H * W / (ms[0] * 1e-3):.4g}")
        cast = vol.raycast_enqueue(poses[:args.views], K, H, W)
        hits, marked = (int(x) for x in cast.hits.cpu())
        bricks = int(np.prod([-(-d // b) for d, b in zip(dims, _lib.TSDF_BRICK)]))
        run["hit_rate"], run["bricks_marked"], run["bricks"] = round(hits / (args.views * H * W), 4), marked, bricks
        # a live frame 2 degrees and 5 cm from the model's pose
        away = poses[1].clone()
        ca, sa = math.cos(math.radians(2.0)), math.sin(math.radians(2.0))
        away[:3, :3] = poses[1][:3, :3] @ torch.tensor([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]], device=dev)
        away[:3, 3] += torch.tensor([0.03, -0.02, 0.035], device=dev)
        live, _ = mr.render_mesh_depth(marched, away[None], K, H, W)
        model = vol.raycast_enqueue(poses[1:2], K, H, W)
        run["register_10_ms"] = timed3(lambda: vol.track_enqueue(live[0], K, poses[1], poses[1], model, max_iteration=10, relative_fitness=0.0,
                                                                 relative_rmse=0.0), args.reps)
        result, pose = vol.track_enqueue(live[0], K, poses[1], poses[1], model, max_iteration=10, relative_fitness=0.0, relative_rmse=0.0)
        r = result.cpu().numpy()
        run["register_10"] = {"iterations": int(r[19]), "pairs": int(r[16]), "fitness": round(float(r[17]), 4), "rmse_m": round(float(r[18]), 5),
                              "translation_error_cm": round(100 * float((pose[:3, 3] - away[:3, 3]).norm()), 3)}
        # the same registration with the colour term, against a volume that fused the texture too
        cvol = tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, color=True, device=dev)
        for k in range(0, args.views, 16):                       # the colour images of 16 views at a time
            cvol.integrate_enqueue(depth[k:k + 16], poses[k:k + 16], K, texture(depth[k:k + 16], poses[k:k + 16], K))
        cmodel = cvol.raycast_enqueue(poses[1:2], K, H, W, color=True)
        rgb = texture(live, away[None], K)[0]
        ckw = dict(max_iteration=10, relative_fitness=0.0, relative_rmse=0.0, relative_color_rmse=0.0, rgb=rgb)
        run["register_color_10_ms"] = timed3(lambda: cvol.track_enqueue(live[0], K, poses[1], poses[1], cmodel, **ckw), args.reps)
        run["register_10_again_ms"] = timed3(lambda: vol.track_enqueue(live[0], K, poses[1], poses[1], model, max_iteration=10, relative_fitness=0.0,
                                                                       relative_rmse=0.0), args.reps)
        result, pose = cvol.track_enqueue(live[0], K, poses[1], poses[1], cmodel, **ckw)
        r = result.cpu().numpy()
        run["register_color_10"] = {"iterations": int(r[19]), "pairs": int(r[16]), "fitness": round(float(r[17]), 4), "rmse_m": round(float(r[18]), 5),
                                    "rows": int(r[20]), "color_rmse": round(float(r[21]), 5), "color_weight": tsdf.DEFAULT_COLOR_WEIGHT,
                                    "translation_error_cm": round(100 * float((pose[:3, 3] - away[:3, 3]).norm()), 3)}
        del cvol, cmodel
        nan_pose = torch.full((4, 4), float("nan"), device=dev)

        def frame():
            result, pose = vol.track_enqueue(live[0], K, poses[1])
            bad = result[16] < 1000.0
            vol.integrate_enqueue(live, torch.where(bad, nan_pose, pose)[None], K)
        run["odometry_frame_ms"] = timed3(frame, args.reps)

        def route():
            v, f = mesh_mod.marching_cubes(vol.volume(), 0.0, truncation=1.0, return_device=True)
            world = torch.from_numpy(origin).to(dev) + v * voxel
            return mr.render_mesh_depth((world, f), poses[:1], K, H, W)
        run["volume_march_render_ms"] = wall(route, 3)
    res["board"] = board.summary()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
