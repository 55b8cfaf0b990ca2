"""Times the mesh evaluation (mipsfusion_amd/evaluate.py) on one GPU at the published protocol's size: 200 000
samples on each of two meshes of the box room (the room's 12 triangles, and a marched 128^3 SDF of the room shifted by 2 cm).

    python tools/eval_time.py [--n 200000] [--reps 7] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps:
  sample     mipsf_eval_sample of the marched mesh (units, 64-bit scan, draw)
  bin        mipsf_icp_bin of one sample cloud (box, count, scan, scatter)
  nearest    mipsf_eval_nearest, reconstruction -> ground truth, on a grid already made
  stats      mipsf_eval_stats of the 200 000 squared distances
  metrics    reconstruction_metrics as a user calls it, host clock around the call (uploads, 4 read-backs)
and, for scale, THIS PROJECT's float64 restatement (tests/eval_cpu.py: numpy + scipy's cKDTree) of the whole call on the host's
threads.  The shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                           # noqa: E402
from mipsfusion_amd import _lib, evaluate as ev, mesh as mesh_mod, synth  # noqa: E402
from mipsfusion_amd import pose_corrector as pc                          # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


def marched_room(dev, shift, res=128, pad=0.25):
    v, f = synth.box_room_mesh(synth.config_reference_defaults()["mapping"]["bound"])
    lo, hi = v.min(0) + shift, v.max(0) + shift
    ticks = [torch.linspace(float(lo[d] - pad), float(hi[d] + pad), res, dtype=torch.float64, device=dev) for d in range(3)]
    p = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1)
    sdf = torch.minimum(p - torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev) - p).amin(-1).to(torch.float32).contiguous()
    mv, mf = mesh_mod.marching_cubes(sdf, 0.0, truncation=3.0)
    step = np.array([(float(t[-1]) - float(t[0])) / (res - 1) for t in ticks])
    return mesh_mod.Mesh(np.array([float(t[0]) for t in ticks]) + mv * step, mf, None), mesh_mod.Mesh(v, f, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_time.py needs a GPU")
    dev = torch.device("cuda:0")
    n = args.n
    rec, gt = marched_room(dev, np.array([0.02, 0.0, 0.0]))
    rv, rf = ev._mesh_tensors(rec.vertices, rec.faces)
    p_rec, _, _ = ev.sample_surface(rec, n=n, seed=0)
    p_gt, _, _ = ev.sample_surface(gt, n=n, seed=1)
    grid, cells = pc.bin_enqueue(p_gt)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)

    def nearest():
        a = _lib.EvalNearestArgs.new(n_source=n, n_target=n, max_cells=cells, source=p_rec.data_ptr(), grid=grid.data_ptr(),
                                     index=index.data_ptr(), d2=d2.data_ptr())
        _lib.check(_lib.lib().mipsf_eval_nearest(C.byref(a), _lib.stream_ptr()), "eval_nearest")
    res = {"sizes": {"samples_per_mesh": n, "faces_rec": int(len(rec.faces)), "faces_gt": int(len(gt.faces))}}
    with BoardSampler(dev.index or 0) as board:
        gpu = {"sample_ms": timed(lambda: ev.sample_enqueue(rv, rf, n, 0), args.reps),
               "bin_ms": timed(lambda: pc.bin_enqueue(p_gt), args.reps),
               "nearest_ms": timed(nearest, args.reps),
               "stats_ms": timed(lambda: ev.stats_enqueue(d2, 0.05), args.reps)}
        host = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = ev.reconstruction_metrics(rec, gt, n, 0.05)
            host.append((time.perf_counter() - t0) * 1e3)
        gpu["metrics_ms_host_clock"] = round(float(np.median(host[1:])), 3)
    res["gpu"] = gpu
    res["metrics"] = m._asdict()
    res["board"] = board.summary()
    if not args.no_cpu:
        from tests import eval_cpu as E
        t0 = time.perf_counter()
        want = E.reconstruction_metrics((rec.vertices, rec.faces), (gt.vertices, gt.faces), n, 0.05)
        res["cpu_restatement"] = {"what": "tests/eval_cpu.py (numpy + scipy cKDTree), this project's restatement",
                                  "tree_query_threads": __import__("tests.icp_cpu", fromlist=["WORKERS"]).WORKERS,
                                  "metrics_ms": round((time.perf_counter() - t0) * 1e3, 1),
                                  "equal_counts": bool(want["completion_ratio"] == m.completion_ratio and want["accuracy_ratio"] == m.accuracy_ratio),
                                  "accuracy": want["accuracy"], "completion": want["completion"]}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
