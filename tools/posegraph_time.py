"""Times the sub-map pose graph (mipsfusion_amd/pose_graph.py) on one GPU: the one launch of
``pose_graph_enqueue`` on the 8-node loop, a 64-node loop with 64 edges and the 64-node graph with 1024 edges of
tests/posegraph_cpu.py's fixtures, at the reference's settings (10 steps at most, patience 3, radius 1e4).

    python tools/posegraph_time.py [--reps 21] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps (inputs already on the device, outputs
and workspace reused), the host clock around ``pose_graph_optimize`` (edges built on the host, upload, launch, one read-back),
and, for scale, THIS PROJECT's numpy restatement (tests/posegraph_cpu.py, not pypose, which is not installed) on the host.  The
shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                           # noqa: E402
from mipsfusion_amd import pose_graph as pg                              # noqa: E402
from tests import posegraph_cpu as R                                     # noqa: E402

GRAPHS = {"n8_e8": R.GPU_FIXTURES["chain8_loop0"], "n64_e64": lambda: R.chain_graph(64, drift=0.3, seed=7, weight=1.0),
          "n64_e1024": R.GPU_FIXTURES["n64_e1024"]}


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
    return round(float(np.median(out)), 4), round(float(np.min(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posegraph_time.py needs a GPU")
    dev = torch.device("cuda:0")
    res = {}
    with BoardSampler(dev.index or 0) as board:
        for name, make in GRAPHS.items():
            X, e, o, w = make()
            bufs = (torch.from_numpy(X).to(dev), torch.from_numpy(e).to(dev), torch.from_numpy(o).to(dev), torch.from_numpy(w).to(dev))
            out = pg.pose_graph_enqueue(*bufs)
            med, best = timed(lambda: pg.pose_graph_enqueue(*bufs, out=out), args.reps)
            r = out[2].cpu()
            row = {"nodes": len(X), "edges": len(e), "launch_ms_median": med, "launch_ms_min": best, "steps": int(r[2]), "solves": int(r[3]),
                   "rejections": int(r[4]), "first_loss": float(r[0]), "loss": float(r[1])}
            # the checked call as a user makes it: adjacency edges of the chain + the loop's key edge
            n = len(X)
            pairs = [[i, i + 1] for i in range(n - 1)]
            Xp = R.project(X)
            prev = np.eye(4)
            aft = R.rigid_inverse(Xp[0]) @ Xp[n - 1] @ R.random_pose(np.random.default_rng(0), 0.1, 0.1)
            host = []
            for _ in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pg.pose_graph_optimize(torch.from_numpy(X), pairs, torch.from_numpy(prev), torch.from_numpy(aft), n - 1, 0, device=dev)
                host.append((time.perf_counter() - t0) * 1e3)
            row["optimize_ms_host_clock_chain_edges"] = round(float(np.median(host[1:])), 3)
            if not args.no_cpu:
                cpu = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    want = R.optimize(X, e, o, w)
                    cpu.append((time.perf_counter() - t0) * 1e3)
                row["cpu_restatement_ms"] = round(float(np.median(cpu)), 2)
                row["cpu_restatement_steps"] = want["steps"]
            res[name] = row
    res["board"] = board.summary()
    res["cpu_restatement"] = "tests/posegraph_cpu.py (numpy, LAPACK Cholesky), this project's restatement, not pypose"
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
