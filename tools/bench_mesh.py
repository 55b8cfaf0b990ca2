#!/usr/bin/env python3
"""Times the mesh extractor on one GPU: per stage (device event pairs) and the whole marching_cubes() call, for 96^3, 256^3
and 512x512x256 analytic volumes generated on the device, with the grid query that feeds it beside it.

    python tools/bench_mesh.py [--repeats 20] [--warmup 3] [--json out.json]

`count` is classify + per-block reduce + block scan (one C call); its traffic is one read of the volume (4 B/voxel), one byte
written and one byte re-read per cell.  The split of `count` into its three kernels comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py --repeats 5` (kernels mcubes_classify_kernel,
mcubes_reduce_kernel, scan_blocks_kernel).  HBM_BPS is the achievable copy bandwidth DESIGN.md uses."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mipsfusion_amd import _lib, inference, mesh, synth  # noqa: E402

HBM_BPS = 6.3e12


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def volume(shape, dev):
    x, y, z = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in shape], indexing="ij")
    c = [0.49 * n for n in shape]
    r = 0.32 * min(shape)
    return (torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
            + 2.0 * torch.sin(0.3 * x) * torch.sin(0.27 * y) * torch.sin(0.33 * z)).contiguous()


def bench_shape(shape, dev, warmup, repeats):
    vol = volume(shape, dev)
    n = vol.numel()
    out = {"shape": list(shape)}
    out["count"] = timed(lambda: mesh._count(vol, 0.0, 3.0), warmup, repeats)
    a, cases, offsets = mesh._count(vol, 0.0, 3.0)
    T = int(offsets[-1])
    soup = torch.empty((T, 3, 3), dtype=torch.float32, device=dev)
    cells = torch.empty((T,), dtype=torch.int32, device=dev)
    a.soup, a.cell_ids, a.capacity_tris = _lib.dptr(soup), _lib.dptr(cells, torch.int32), T
    out["emit"] = timed(lambda: _lib.check(_lib.lib().mipsf_mcubes_emit(C.byref(a), _lib.stream_ptr()), "emit"), warmup, repeats)
    out["weld"] = timed(lambda: mesh.weld(soup), warmup, repeats)              # includes the read-back of V
    v, f = mesh.weld(soup)
    out["filter"] = timed(lambda: mesh.filter_faces(f, cells), warmup, repeats)
    out["whole_call_device"] = timed(lambda: mesh.marching_cubes(vol, 0.0, 3.0, return_device=True), warmup, repeats)
    out["whole_call_numpy"] = timed(lambda: mesh.marching_cubes(vol, 0.0, 3.0), warmup, max(3, repeats // 4))
    vv, ff = mesh.marching_cubes(vol, 0.0, 3.0, return_device=True)
    out.update(triangles_soup=T, vertices=int(vv.shape[0]), faces=int(ff.shape[0]))
    bytes_count = 6 * n
    out["count_bytes"] = bytes_count
    out["count_share_of_hbm"] = bytes_count / HBM_BPS / (out["count"]["median_ms"] * 1e-3)
    out["volume_read_floor_ms"] = 4 * n / HBM_BPS * 1e3
    return out


def bench_query(shape, dev, warmup, repeats):
    cfg = synth.config_headline()
    bb = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float64)
    nf = torch.tensor(cfg["mapping"]["localMLP_max_len"], dtype=torch.float64)
    from mipsfusion_amd.model import JointEncoding
    torch.manual_seed(0)
    model = JointEncoding(cfg, bb, nf).to(dev).eval()
    ticks = [torch.linspace(0.0, 1.0, n, device=dev) for n in shape]
    pts = torch.stack(torch.meshgrid(*ticks, indexing="ij"), -1).reshape(-1, 3)
    with torch.no_grad():
        return timed(lambda: inference.query_in_batches(lambda p: model.query_sdf(p[:, None, :]), pts, 1024 * 64), 1, max(2, repeats // 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--no-query", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "hbm_bps_assumed": HBM_BPS, "shapes": []}
    for shape in ((96, 96, 96), (256, 256, 256), (512, 512, 256)):
        r = bench_shape(shape, dev, a.warmup, a.repeats)
        if not a.no_query and shape[0] <= 256:
            r["grid_query"] = bench_query(shape, dev, a.warmup, a.repeats)
        res["shapes"].append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
