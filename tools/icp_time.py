"""Times the switch-pose rectification (mipsfusion_amd/pose_corrector.py) on one GPU at the reference's sizes:
10 keyframes x 30 000 ray rows as the target, one frame's 30 000 rows as the source (synth frames of the box room, 2 % of the
pixels without depth, the frame's pose off by 1 degree and 2 cm).

    python tools/icp_time.py [--reps 7] [--out file.json] [--no-cpu] [--no-walk]

Milliseconds between two events on the stream after one warm-up call, median of --reps:
  cloud      mipsf_icp_cloud over the 300 000 target rows (flag, scan, emit)
  bin        mipsf_icp_bin of the target cloud with the registration's edge (box, count, scan, scatter)
  normals    estimate_normals of the target cloud: its own grid + the 30-neighbour search + covariance + eigenvector
  icp        registration_enqueue: the target's grid + 31 enqueued evaluations, of which those after the stop return at once
  rectify    switch_pose_rectifying as the runner calls it, host clock around the call (it ends in a read-back)
and, for scale, THIS PROJECT's float64 restatement (tests/icp_cpu.py: numpy + scipy's cKDTree, not open3d, which is not
installed) of the same steps on the host's threads.  --walk (default) also runs the two-room walk of tests/test_gpu_icp.py with
and without ``rectify_switch`` and prints the cost of its ("back", 0) switch frame (store, load, refinement replay; with the
flag: + the rectification at that walk's 8 000 rays per keyframe), so the share the rectification adds can be read off.
The shader clock and package power sampled across the timed regions are printed beside the times (bench.BoardSampler)."""
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
from mipsfusion_amd import pose_corrector as pc                          # noqa: E402
from mipsfusion_amd.keyframe_rays import DeviceRayDB                     # noqa: E402
from tests import icp_cpu as R                                           # noqa: E402


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


def walk(dev, rectify):
    from tests.test_gpu_icp import _walk
    seq, res, out, schedule = _walk(dev, rectify)
    back = [v for v in out["switch_frames"].values() if v["kind"] == "back"]
    return {"back_switch_ms": back[0]["ms"], "rectified": res["rectified"], "rays_per_keyframe": seq.R,
            "ate_rmse_m": out["ate_rmse_m"], "ate_max_m": out["ate_max_m"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-walk", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_time.py needs a GPU")
    dev = torch.device("cuda:0")
    s = R.synth_scene(n_kf=10, rays_per_kf=(100, 300))
    k, r = s["kf_rows"].shape[:2]
    rows, poses = s["kf_rows"].reshape(-1, 7).contiguous().to(dev), s["kf_poses"].to(dev).contiguous()
    frame_rows, drifted = s["frame_rows"].to(dev), s["frame_pose_drifted"]
    db = DeviceRayDB(k, r, dev)
    for i in range(k):
        db.store(i, s["kf_rows"][i].to(dev))
    target, nt = pc.cloud_from_rays(rows, r, poses)
    source, ns = pc.cloud_from_rays(frame_rows, r, drifted[None].to(dev).contiguous())
    target, source = target.contiguous(), source.contiguous()
    normals = pc.estimate_normals(target)
    md = pc.SWITCH_DEFAULTS["align_threshold"]
    res = {"sizes": {"target_rows": k * r, "target_points": nt, "source_rows": r, "source_points": ns, "max_dist": md}}
    with BoardSampler(dev.index or 0) as board:
        gpu = {"cloud_ms": timed(lambda: pc.cloud_enqueue(rows, r, poses), args.reps),
               "bin_ms": timed(lambda: pc.bin_enqueue(target, md * pc.EDGE_MARGIN), args.reps),
               "normals_ms": timed(lambda: pc.normals_enqueue(target), args.reps),
               "icp_ms": timed(lambda: pc.registration_enqueue(source, target, normals, md), args.reps)}
        cfg = {"tracking": {"switch": {}}}
        host = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flag, n, pose = pc.switch_pose_rectifying(db, list(range(k)), s["kf_poses"], frame_rows, drifted, cfg)
            host.append((time.perf_counter() - t0) * 1e3)
        gpu["rectify_ms_host_clock"] = round(float(np.median(host[1:])), 3)
    icp = pc.registration_icp(source, target, normals, md)
    gt = s["frame_pose_gt"]
    res["gpu"] = gpu
    res["result"] = {"flag": flag, "n_correspondences": n, "iterations": icp.iterations, "fitness": round(icp.fitness, 4),
                     "inlier_rmse_m": round(icp.inlier_rmse, 5),
                     "translation_error_m": [round(float((drifted[:3, 3] - gt[:3, 3]).norm()), 5), round(float((pose[:3, 3] - gt[:3, 3]).norm()), 5)]}
    res["board"] = board.summary()
    if not args.no_cpu:
        tp, sp = target.cpu().numpy(), source.cpu().numpy()
        t0 = time.perf_counter()
        cn = R.normals_cpu(tp)[0]
        t1 = time.perf_counter()
        want = R.icp_cpu(sp, tp, cn, md)
        t2 = time.perf_counter()
        res["cpu_restatement"] = {"what": "tests/icp_cpu.py (numpy + scipy cKDTree), this project's restatement, not open3d",
                                  "tree_query_threads": R.WORKERS,
                                  "normals_ms": round((t1 - t0) * 1e3, 1), "icp_ms": round((t2 - t1) * 1e3, 1),
                                  "iterations": want["iterations"], "n_correspondences": want["n"]}
    if not args.no_walk:
        res["two_room_walk"] = {"with_rectify_switch": walk(dev, True), "without": walk(dev, False)}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
