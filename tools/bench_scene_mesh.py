"""Times the scene mesher (mipsfusion_amd/scene_mesh.py) on one GPU: 4 sub-maps, a 256^3 grid, 64 keyframes each.

    python tools/bench_scene_mesh.py [--reps 5] [--out file.json] [--no-cpu]

The scene is analytic (a box room, one sub-map per quadrant, overlapping), so that marching and clean-up see a real surface.
Milliseconds, host clock around a device synchronise, after one warm-up pass, median of --reps:
  visibility      the kernel alone over the whole grid with 64 keyframes, (a) as it is, where a wave leaves the keyframe loop
                  once all its points are seen, and (b) with every max depth at 0, where nothing is seen and all n*k tests run:
                  (b) gives the rate in point-keyframe tests per second, computed from the shapes
  fusion          fuse_volume with the model queries replaced by slices of a precomputed table: points kernel + accumulate
                  (visibility of each sub-map's keyframes fused in) + finalize
  queries         query_sdf_entropy_prob of a randomly initialised JointEncoding (the reference's default configuration) over as
                  many points as the four sub-boxes hold, in the batches fuse_volume uses
  marching        mesh.marching_cubes on the fused volume
  clean-up        visibility of the vertices, components, bounding geometry, compaction
  colours         blend_colors on the final vertices (analytic colour)
and the CPU restatement (tests/scene_mesh_cpu.py) of fusion + marching + clean-up on a 96^3 grid on 16 threads, for scale.
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
from mipsfusion_amd import inference, mesh, scene_mesh as sm, synth     # noqa: E402
from mipsfusion_amd.model import JointEncoding                           # noqa: E402
from tests import scene_mesh_cpu as sc                                   # noqa: E402

K, W, H = sc.CAMERA["K"], sc.CAMERA["W"], sc.CAMERA["H"]
EXTENT = 7.59                                   # (EXTENT + 2 * 0.05) // 0.03 = 256 ticks, // 0.08 = 96 ticks
ROOM = np.array([[0.5, EXTENT - 0.5]] * 3)
CFG = {"grid": {"tcnn_encoding": True, "use_bound_normalize": True}, "cam": {"W": W, "H": H},
       "mapping": {"bound": [[-0.5, EXTENT + 0.5]] * 3, "localMLP_max_len": [9.0, 9.0, 9.0]}, "training": {"norm_factor": 1.0},
       "mesh": {"voxel_final": 0.03}}


def room_sdf(w):
    box = torch.tensor(ROOM, dtype=w.dtype, device=w.device)
    return torch.clamp(torch.minimum(w - box[:, 0], box[:, 1] - w).min(-1)[0] / 0.3, -1, 1)


def submaps(k=64):
    out = []
    half = EXTENT / 2
    for i in range(4):
        qx, qz = i % 2, i // 2
        aabb = np.array([[qx * half - 0.2 * qx, (qx + 1) * half + 0.2 * (1 - qx)], [0.0, EXTENT],
                         [qz * half - 0.2 * qz, (qz + 1) * half + 0.2 * (1 - qz)]])
        centre = aabb.mean(1)
        c2w, md = sc.ring_of_keyframes(centre, k, 40 + i, radius=0.8)
        model = sc.Analytic(CFG, np.eye(4), room_sdf, sc.wavy_entropy(0.1 + 0.02 * i, 0.05), rgb=lambda w, i=i: torch.sin(3.0 * w + i))
        out.append(sm.SubMap(model, np.eye(4, dtype=np.float32), c2w, md * 1.5, aabb, None, centre.astype(np.float32), None))
    return out


class Table:
    """stands in for a model: the answers were computed before, a query returns the next rows of the table"""

    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def query_sdf_entropy_prob(self, p):
        self.at += p.shape[0]
        return self.raw[self.at - p.shape[0]:self.at]


def timed(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    with BoardSampler(dev.index or 0) as board:
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
    s = board.summary()
    return out, {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                 "sclk_mhz_median": s["sclk_mhz_median"], "power_w_median": s["power_w_median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_mesh needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    subs = submaps()
    res = {"submaps": len(subs), "keyframes_each": 64, "device": torch.cuda.get_device_name(dev)}

    ticks = sm.get_grid_uniform(np.zeros(3), np.full(3, EXTENT), 0.05, 0.03)
    n = int(np.prod([len(t) for t in ticks]))
    res["grid"] = [len(t) for t in ticks]
    c2w, md = subs[0].kf_c2w, subs[0].kf_max_depth
    seen, res["visibility"] = timed(lambda: sm.grid_point_mask(ticks, c2w, md, K, W, H, device=dev), a.reps, dev)
    res["visibility"]["seen_share"] = round(float(seen.float().mean()), 4)
    _, res["visibility_all_tests"] = timed(lambda: sm.grid_point_mask(ticks, c2w, np.zeros_like(md), K, W, H, device=dev), a.reps, dev)
    res["visibility_all_tests"]["point_keyframe_tests"] = n * len(md)
    res["visibility_all_tests"]["tests_per_second"] = float(f"{n * len(md) / (res['visibility_all_tests']['ms_median'] * 1e-3):.4g}")

    # the answers of the analytic models, once, for the fusion without queries
    grid = sm._Grid(ticks, dev)
    tables, n_query = [], 0
    for s in subs:
        lo, size = grid.index_box(s.aabb)
        pts = sm._local_points(grid.points(lo, size), s.first_kf_c2w, CFG, dev)
        tables.append(inference.query_in_batches(s.model.query_sdf_entropy_prob, pts, sm.QUERY_BATCH).to(torch.float32).contiguous())
        n_query += pts.shape[0]
        del pts
    res["points_queried"] = n_query

    def fuse_from_tables():
        return sm.fuse_volume([s._replace(model=Table(t)) for s, t in zip(subs, tables)], CFG, K, device=dev)
    fused, res["fusion_without_queries"] = timed(fuse_from_tables, a.reps, dev)
    res["fusion_without_queries"]["finite_share"] = round(float(torch.isfinite(fused.volume).float().mean()), 4)
    del tables

    cfg = synth.config_reference_defaults()
    torch.manual_seed(0)
    net = JointEncoding(cfg, torch.from_numpy(np.array(cfg["mapping"]["bound"])), torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))).to(dev)
    pts = torch.rand((sm.CHUNK, 3), dtype=torch.float64, device=dev)

    def queries():
        for first in range(0, n_query, sm.CHUNK):
            inference.query_in_batches(net.query_sdf_entropy_prob, pts[:min(sm.CHUNK, n_query - first)], sm.QUERY_BATCH)
    _, res["queries"] = timed(queries, max(1, a.reps // 2), dev)
    del net, pts

    (v, f), res["marching"] = timed(lambda: mesh.marching_cubes(fused.volume, 0.0, 3.0, return_device=True), a.reps, dev)
    spacing = torch.tensor([t[2] - t[1] for t in ticks], dtype=torch.float64, device=dev)
    origin = torch.tensor([t[0] for t in ticks], dtype=torch.float64, device=dev)
    v = v * spacing + origin
    res["marching"].update(vertices=int(v.shape[0]), faces=int(f.shape[0]))
    (cv, cf), res["clean_up"] = timed(lambda: sm.clean_up(v, f, subs, CFG, K), a.reps, dev)
    res["clean_up"].update(vertices=int(cv.shape[0]), faces=int(cf.shape[0]))
    _, res["colours"] = timed(lambda: sm.blend_colors(cv, subs, CFG, K), a.reps, dev)

    if not a.no_cpu:
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        ref = sc.fuse_volume(subs, CFG, K, voxel_size=0.08)
        t1 = time.perf_counter()
        rv, rf, _ = sc.scene_mesh_from_volume(ref["volume"], ref["ticks"], subs, CFG, K, render_color=False)
        t2 = time.perf_counter()
        res["cpu_restatement_96"] = {"grid": list(ref["volume"].shape), "fusion_with_queries_ms": round((t1 - t0) * 1e3, 1),
                                     "marching_and_clean_up_ms": round((t2 - t1) * 1e3, 1), "faces": int(len(rf)), "threads": 16}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
