"""Times the mesh renderer (mipsfusion_amd/mesh_render.py) on one GPU at the size of a cropped dataset frame,
460 x 620 pixels: the box room's 12 triangles and a marched 128^3 SDF of the same room, from 1 view and from 64 views in one launch.

    python tools/raster_time.py [--reps 7] [--res 128] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps.  The stages of mipsf_raster_depth are
run one at a time through its `stages` mask; what a stage needs from the one before is put back, untimed, before every repeat:
  count      keys cleared, tiles of every (view, face) counted
  scan       64-bit prefix sum of the counts                           (after a count)
  raster     one wavefront per tile, atomicMin of the keys             (after count + scan: the keys are empty again)
  resolve    keys -> depth and face
  depth      the whole call
  l1         mipsf_raster_l1 of the marched room's depth against the 12 triangles'
  visible    mipsf_raster_visible of the marched mesh's vertices against the views' depth
and, for scale, THIS PROJECT's float64 restatement (tests/raster_cpu.py: numpy, every pixel against every face) of one view of
the 12 triangles and of a marched 24^3 room at the same image size, 16 views at a time on 16 threads.  The shader clock and package
power sampled across the timed regions are printed beside the times (bench.BoardSampler)."""
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

from bench import BoardSampler                                                            # noqa: E402
from mipsfusion_amd import _lib, evaluate as ev, mesh as mesh_mod, mesh_render as mr, synth  # noqa: E402
from mipsfusion_amd import pose_corrector as pc                                           # noqa: E402


def timed(fn, reps, setup=None):
    out = []
    for k in range(reps + 1):
        if setup is not None:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:                                                                             # the first one is the warm-up
            out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


def marched_room(dev, res, pad=0.25):
    v, f = synth.box_room_mesh(synth.config_reference_defaults()["mapping"]["bound"])
    lo, hi = v.min(0), v.max(0)
    ticks = [torch.linspace(float(lo[d] - pad), float(hi[d] + pad), res, dtype=torch.float64, device=dev) for d in range(3)]
    p = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1)
    sdf = torch.minimum(p - torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev) - p).amin(-1).to(torch.float32).contiguous()
    mv, mf = mesh_mod.marching_cubes(sdf, 0.0, truncation=3.0)
    step = np.array([(float(t[-1]) - float(t[0])) / (res - 1) for t in ticks])
    return (np.array([float(t[0]) for t in ticks]) + mv * step, mf), (v, f)


def view_poses(n, centre):
    """n poses around the room's centre: the yaw goes round once, the pitch and the position sway"""
    poses = []
    for k in range(n):
        u = k / max(n, 1)
        c2w = torch.eye(4)
        c2w[:3, :3] = synth.look_rotation(0.3 + 2.0 * math.pi * u, -0.1 + 0.4 * math.sin(5.0 * u))
        c2w[:3, 3] = torch.tensor(centre + np.array([0.5 * math.sin(7.0 * u), 0.3 * math.cos(3.0 * u), 0.4 * math.sin(4.0 * u)]), dtype=torch.float32)
        poses.append(c2w)
    return torch.stack(poses)


def time_mesh(mesh, poses, K, H, W, reps, dev):
    v, f = ev._mesh_tensors(*mesh)
    P = poses.to(dev).contiguous()
    n = P.shape[0]
    ws = pc._bytes(mr._ws_bytes(_lib.RASTER_WS_DEPTH, n, f.shape[0], H, W), dev)
    depth = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(n, H, W, dtype=torch.int32, device=dev)

    def run(stages):
        return lambda: mr.render_enqueue(v, f, P, K, H, W, depth=depth, face=face, workspace=ws, stages=stages)
    C, S, R, Z = _lib.RASTER_STAGE_COUNT, _lib.RASTER_STAGE_SCAN, _lib.RASTER_STAGE_RASTER, _lib.RASTER_STAGE_RESOLVE
    run(0)()
    out = {"views": n, "faces": int(f.shape[0]), "count_ms": timed(run(C), reps), "scan_ms": timed(run(S), reps, setup=run(C)),
           "raster_ms": timed(run(R), reps, setup=run(C | S)), "resolve_ms": timed(run(Z), reps), "depth_ms": timed(run(0), reps)}
    run(C)()
    torch.cuda.synchronize()
    items = n * f.shape[0]
    counts = ws.view(torch.int64)[(n * H * W * 8 + 15) // 16 * 2:][:items]                # the counts, before a scan
    out["tiles"] = int(counts.sum())
    out["pairs_with_the_whole_image"] = int((counts == ((H + 7) // 8) * ((W + 7) // 8)).sum())
    run(0)()
    return out, depth, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, args.res)
    centre = 0.5 * (room[0].min(0) + room[0].max(0))
    res = {"image": [H, W], "marched_res": args.res, "runs": []}
    with BoardSampler(dev.index or 0) as board:
        for n in (1, 64):
            poses = view_poses(n, centre)
            r_room, d_room, _ = time_mesh(room, poses, K, H, W, args.reps, dev)
            r_marched, d_marched, verts = time_mesh(marched, poses, K, H, W, args.reps, dev)
            P = poses.to(dev).contiguous()
            md = torch.full((n,), 10.0, device=dev)
            extra = {"l1_ms": timed(lambda: mr.l1_enqueue(d_marched, d_room), args.reps),
                     "visible_ms": timed(lambda: mr.visible_enqueue(verts, d_marched, P, md, K, 20.0, 0.02), args.reps),
                     "visible_points": int(verts.shape[0])}
            m = mr.metrics_from_records(mr.read_l1_records(mr.l1_enqueue(d_marched, d_room)), H, W)
            extra["l1_mm"], extra["both"] = round(m.l1 * 1e3, 4), m.both
            res["runs"].append({"room_12": r_room, "marched": r_marched, "both": extra})
    res["board"] = board.summary()
    if not args.no_cpu:
        from concurrent.futures import ThreadPoolExecutor
        from tests import raster_cpu as R
        cpu = {"what": "tests/raster_cpu.py (numpy, every pixel against every face), 16 views at a time on 16 threads", "threads": 16}
        poses16 = view_poses(16, centre)
        for name, (v, f) in (("room_12", room), ("marched_24", R.marched_room())):
            v32 = np.asarray(v, np.float32)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(lambda p: R.render_depth(v32, f, p[None], K, H, W, chunk=8), poses16))
            cpu[name] = {"faces": int(len(f)), "ms_per_view": round((time.perf_counter() - t0) * 1e3 / 16, 1)}
        res["cpu_restatement"] = cpu
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
