"""Times the TSDF fusion (mipsfusion_amd/tsdf.py) on one GPU: a 256^3 volume over the marched 128^3 box room, 64 views
of 460 x 620 pixels rendered by render_mesh_depth.

    python tools/tsdf_time.py [--reps 5] [--res 256] [--views 64] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps; the state is zeroed, untimed, before every
repeat (a fused volume saturates nothing, but the words then are the first call's):
  integrate            mipsf_tsdf_integrate of all views, without and with colour, with the brick culling and with every brick
                       taking every view (MIPSF_TSDF_NO_CULL)
  one_view             the same call with one view
  state_copy           a device copy of the state's bytes (tsdf + weight, + colour), the floor of a call that did no arithmetic
  volume_march         volume() and marching_cubes on it, host wall time with a synchronise (marching reads counts back)
  mesh_from_frames     the whole tsdf_mesh_from_frames, bounds from the frames, host wall time
and, for scale, THIS PROJECT's float64 restatement (tests/tsdf_cpu.py: numpy, every voxel against every view) at 128^3 voxels and
16 views.  Pairs per second are voxels x views over the time of the call.  The shader clock and package power sampled across the
timed regions are printed beside the times (bench.BoardSampler)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                # noqa: E402
from mipsfusion_amd import _lib, mesh as mesh_mod, mesh_render as mr, synth, tsdf   # noqa: E402
from tools.raster_time import marched_room, timed, view_poses                # noqa: E402


def wall(fn, reps):
    out = []
    for k in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, 128)
    lo, hi = room[0].min(0), room[0].max(0)
    centre = 0.5 * (lo + hi)
    poses = view_poses(args.views, centre).to(dev).contiguous()
    depth, _ = mr.render_mesh_depth(marched, poses, K, H, W)
    hit = synth.camera_rays(H, W, fx, fy, cx, cy).to(dev)[None] * depth[..., None]
    rgb = (0.5 + 0.5 * torch.sin(4.0 * hit)).contiguous()                      # any smooth colour: the time does not depend on it
    voxel = float((hi - lo + 0.5).max() / (args.res - 1))
    origin = centre - 0.5 * voxel * (args.res - 1)
    dims = (args.res,) * 3
    voxels, pairs = args.res ** 3, args.res ** 3 * args.views
    res = {"image": [H, W], "views": args.views, "dims": list(dims), "voxel_m": round(voxel, 5), "trunc_voxels": 4, "pairs": pairs, "runs": {}}
    with BoardSampler(dev.index or 0) as board:
        for color in (False, True):
            vol = tsdf.TSDFVolume(origin, voxel, dims, 4 * voxel, color=color, device=dev)
            c3 = rgb if color else None
            rec = torch.empty(2, dtype=torch.int64, device=dev)
            run = {}
            for name, flags, n in (("integrate", 0, args.views), ("integrate_no_cull", _lib.TSDF_NO_CULL, args.views), ("one_view", 0, 1)):
                ms = timed(lambda: vol.integrate_enqueue(depth[:n], poses[:n], K, None if c3 is None else c3[:n], record=rec, flags=flags),
                           args.reps, setup=vol.reset)
                run[name + "_ms"] = ms
                run[name + "_pairs_per_s"] = float(f"{voxels * n / (ms * 1e-3):.4g}")
                run[name + "_updates"] = int(rec[0])
            state = [t for t in (vol.tsdf, vol.weight, vol.color) if t is not None]
            copies = [torch.empty_like(t) for t in state]
            run["state_bytes"] = 2 * sum(t.numel() * 4 for t in state)         # read and written once
            run["state_copy_ms"] = timed(lambda: [c.copy_(t) for c, t in zip(copies, state)], args.reps)
            run["state_copy_TB_per_s"] = round(run["state_bytes"] / (run["state_copy_ms"] * 1e-3) / 1e12, 3)
            del copies
            vol.reset()
            vol.integrate_enqueue(depth, poses, K, c3)
            run["volume_march_ms"] = wall(lambda: mesh_mod.marching_cubes(vol.volume(), 0.0, truncation=1.0, return_device=True), args.reps)
            run["extract_mesh_ms"] = wall(vol.extract_mesh, 1)
            run["faces"] = int(len(vol.extract_mesh().faces))
            res["runs"]["colour" if color else "plain"] = run
            del vol
        res["mesh_from_frames_ms"] = wall(lambda: tsdf.tsdf_mesh_from_frames(depth, poses, K, voxel), 2)
    res["board"] = board.summary()
    res["yardsticks"] = {"fuse_visibility_tests_per_s": 7.1e11, "note": "mipsf_fuse_visibility is fp32: an upper mark, not a target"}
    if not args.no_cpu:
        from tests import tsdf_cpu as T
        n, small = 16, 128
        v = float((hi - lo + 0.5).max() / (small - 1))
        ticks = T.make_ticks(centre - 0.5 * v * (small - 1), v, (small,) * 3)
        d_host, p_host = depth[:n].cpu().numpy(), poses[:n].cpu()
        t0 = time.perf_counter()
        T.integrate(T.new_state((small,) * 3), ticks, d_host, p_host, K, 4 * v)
        dt = time.perf_counter() - t0
        res["cpu_restatement"] = {"what": "tests/tsdf_cpu.py (numpy float64, every voxel against every view)", "dims": [small] * 3, "views": n,
                                  "ms": round(dt * 1e3, 1), "pairs_per_s": float(f"{small ** 3 * n / dt:.4g}")}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
