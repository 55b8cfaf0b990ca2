"""Times the mesh shader (mipsfusion_amd/mesh_render.py) on one GPU at the size of a cropped dataset frame,
460 x 620 pixels: the box room's 12 triangles and a marched 128^3 SDF of the same room, from 1 view and from 64 views in one launch.

    python tools/shade_time.py [--reps 7] [--res 128] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps, with the smallest and the largest:
  vertex_normals   mipsf_shade_vertex_normals of the mesh (all its launches)
  color            mipsf_shade_pixels over the face image of mipsf_raster_depth, the colour alone
  normals_flat     the normals alone, from the faces
  normals_smooth   the normals alone, from the vertex normals
  shaded           the head-lit image alone (smooth)
  all              colour, smooth normals and the head-lit image in one launch
  depth            mipsf_raster_depth for the same views, for scale
and THIS PROJECT's float64 restatement (tests/shade_cpu.py, numpy on one thread) of the same calls for one view: the vertex normals
of the marched mesh and the pass with all three outputs.  The shader clock and package power sampled across the timed regions are
printed beside the times (bench.BoardSampler)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import BoardSampler                                                            # noqa: E402
from mipsfusion_amd import _lib, evaluate as ev, mesh_render as mr, synth                 # noqa: E402
from mipsfusion_amd import pose_corrector as pc                                           # noqa: E402
from raster_time import marched_room, view_poses                                          # noqa: E402


def timed(fn, reps):
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:                                                                             # the first one is the warm-up
            out.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def time_mesh(mesh, poses, K, H, W, reps, dev):
    v, f = ev._mesh_tensors(*mesh)
    P = poses.to(dev).contiguous()
    n = P.shape[0]
    cols = torch.rand(v.shape, generator=torch.Generator().manual_seed(22)).to(dev)
    ws = pc._bytes(int(_lib.lib().mipsf_shade_workspace_bytes(_lib.SHADE_WS_VERTEX_NORMALS, v.shape[0], f.shape[0])), dev)
    vn = torch.empty_like(v)
    depth_ws = pc._bytes(mr._ws_bytes(_lib.RASTER_WS_DEPTH, n, f.shape[0], H, W), dev)
    depth = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    color, normals = torch.empty(n, H, W, 3, device=dev), torch.empty(n, H, W, 3, device=dev)
    shaded = torch.empty(n, H, W, device=dev)
    record = torch.empty(2, dtype=torch.int64, device=dev)
    raster = lambda: mr.render_enqueue(v, f, P, K, H, W, depth=depth, face=face, workspace=depth_ws)      # noqa: E731
    raster()
    mr.vertex_normals_enqueue(v, f, vn, ws)

    def shade(mode, **out):
        return lambda: mr.shade_enqueue(v, f, P, K, face, cols, vn, mode, (0.0, 0.0, 0.0), record=record, **out)
    out = {"views": n, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
           "vertex_normals": timed(lambda: mr.vertex_normals_enqueue(v, f, vn, ws), reps),
           "color": timed(shade(_lib.SHADE_FLAT, color=color), reps),
           "normals_flat": timed(shade(_lib.SHADE_FLAT, normals=normals), reps),
           "normals_smooth": timed(shade(_lib.SHADE_SMOOTH, normals=normals), reps),
           "shaded": timed(shade(_lib.SHADE_SMOOTH, shaded=shaded), reps),
           "all": timed(shade(_lib.SHADE_SMOOTH, color=color, normals=normals, shaded=shaded), reps),
           "depth": timed(raster, reps)}
    torch.cuda.synchronize()
    out["hits"], out["with_a_normal"] = (int(x) for x in record.cpu())
    out["longest_segment"] = int(torch.bincount(f.reshape(-1).long(), minlength=1).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shade_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, fx, fy, cx, cy = synth.intrinsics_after_crop(synth.config_reference_defaults())
    K = (fx, fy, cx, cy)
    marched, room = marched_room(dev, args.res)
    centre = 0.5 * (room[0].min(0) + room[0].max(0))
    res = {"image": [H, W], "marched_res": args.res, "reps": args.reps, "runs": []}
    with BoardSampler(dev.index or 0) as board:
        for n in (1, 64):
            poses = view_poses(n, centre)
            res["runs"].append({"room_12": time_mesh(room, poses, K, H, W, args.reps, dev), "marched": time_mesh(marched, poses, K, H, W, args.reps, dev)})
    res["board"] = board.summary()
    if not args.no_cpu:
        from tests import raster_cpu as R
        from tests import shade_cpu as S
        cpu = {"what": "tests/shade_cpu.py (numpy, one thread), one view at the same image size; the face image comes from the device"}
        pose = view_poses(1, centre)
        for name, (v, f) in (("room_12", room), ("marched", marched)):
            v32 = np.asarray(v, np.float32)
            face = mr.render_mesh_depth((v32, f), pose, K, H, W)[1].cpu().numpy()
            t0 = time.perf_counter()
            vn = S.vertex_normals(v32, f)
            t1 = time.perf_counter()
            S.shade(v32, f, pose, K, face, S.uniform_colors(len(v32)), vn, S.SMOOTH)
            t2 = time.perf_counter()
            cpu[name] = {"faces": int(len(f)), "vertex_normals_ms": round((t1 - t0) * 1e3, 1), "all_ms_per_view": round((t2 - t1) * 1e3, 1)}
        res["cpu_restatement"] = cpu
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
