"""Times the image metrics (mipsfusion_amd/image_metrics.py) on one GPU at the size of a cropped dataset frame,
460 x 620 x 3 fp32, for 1 view and for 64 views in one call.

    python tools/image_time.py [--reps 7] [--out file.json] [--no-cpu]

Milliseconds between two events on the stream after one warm-up call, median of --reps:
  error      mipsf_image_error
  ssim       mipsf_image_ssim of the full-size images
  ms_ssim    the five mipsf_image_ssim and the eight mipsf_image_pool2 of the pyramid
and, by a host clock around a call that ends in its read-back:
  image_metrics   the whole call from device tensors: all of the above, one read-back, the combination in Python
Beside them, for scale: the same maps as a float64 grouped conv2d with the 11 x 11 outer-product window in torch on the same GPU
(five levels, avg_pool2d between them; means by torch), and THIS PROJECT's float64 restatement (tests/image_cpu.py, numpy) of
one view a thread on 16 threads.  The shader clock and package power sampled across the timed regions are printed beside the
times (bench.BoardSampler)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import BoardSampler                                                            # noqa: E402
from mipsfusion_amd import image_metrics as M                                             # noqa: E402


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
    return round(float(np.median(out)), 4)


def wall(fn, reps):
    out = []
    for k in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4)


def pyramid(a, b, window, C1, C2):
    for i in range(5):
        M.ssim_enqueue(a, b, window, C1, C2)
        if i < 4:
            a, b = M.pool_enqueue(a), M.pool_enqueue(b)


def torch_ms_ssim(a, b, window, C1, C2):
    """the conv2d formulation in float64 on the device -> (ssim, ms_ssim) means per (view, channel)"""
    x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    C = x.shape[1]
    w = torch.outer(window, window)[None, None].repeat(C, 1, 1, 1)
    vals = []
    for i in range(5):
        f = lambda q: F.conv2d(q, w, groups=C)                                            # noqa: E731
        m1, m2 = f(x), f(y)
        s1, s2, s12 = f(x * x) - m1 * m1, f(y * y) - m2 * m2, f(x * y) - m1 * m2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim = ((2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1)) * cs
        vals.append((ssim.mean((2, 3)), cs.mean((2, 3))))
        if i < 4:
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    weights = torch.tensor(M.MS_WEIGHTS, dtype=torch.float64, device=a.device)
    levels = torch.stack([v[1] for v in vals[:4]] + [vals[4][0]], 0).clamp_min(0)
    return vals[0][0], torch.prod(levels ** weights[:, None, None], 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_time.py needs a GPU")
    dev = torch.device("cuda:0")
    H, W, C = 460, 620, 3
    window, (C1, C2) = M.gaussian_window(), M.ssim_constants(1.0)
    wt = torch.tensor(window, dtype=torch.float64, device=dev)
    res = {"image": [H, W, C], "dtype": "float32", "reps": args.reps, "runs": []}
    g = torch.Generator(device="cpu").manual_seed(0)
    with BoardSampler(dev.index or 0) as board:
        for n in (1, 64):
            a = torch.rand(n, H, W, C, generator=g)
            b = (a + 0.1 * torch.randn(n, H, W, C, generator=g)).clamp(0, 1)
            a, b = a.to(dev), b.to(dev)
            m = M.image_metrics(a, b)
            try:                                       # a float64 convolution is not every backend's: say so instead of stopping
                t_ssim, t_ms = torch_ms_ssim(a, b, wt, C1, C2)
                conv = {"torch_conv2d_f64_ms_ssim_ms": timed(lambda: torch_ms_ssim(a, b, wt, C1, C2), args.reps),
                        "ssim_minus_torch": abs(m.ssim - float(t_ssim.mean())), "ms_ssim_minus_torch": abs(m.ms_ssim - float(t_ms.mean()))}
            except RuntimeError as e:
                conv = {"torch_conv2d_f64_ms_ssim_ms": None, "torch_conv2d_f64_error": str(e).splitlines()[0][:200]}
            run = {"views": n,
                   "error_ms": timed(lambda: M.error_enqueue(a, b), args.reps),
                   "ssim_ms": timed(lambda: M.ssim_enqueue(a, b, window, C1, C2), args.reps),
                   "ms_ssim_ms": timed(lambda: pyramid(a, b, window, C1, C2), args.reps),
                   "image_metrics_wall_ms": wall(lambda: M.image_metrics(a, b), args.reps),
                   "psnr": m.psnr, "ssim": m.ssim, "ms_ssim": m.ms_ssim, **conv}
            res["runs"].append(run)
    res["board"] = board.summary()
    if not args.no_cpu:
        from concurrent.futures import ThreadPoolExecutor
        from tests import image_cpu as I
        a16, b16 = a[:16].cpu().numpy(), b[:16].cpu().numpy()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            got = list(ex.map(lambda k: I.metrics(a16[k:k + 1], b16[k:k + 1]), range(16)))
        res["cpu_restatement"] = {"what": "tests/image_cpu.py (numpy float64), one view a thread on 16 threads", "threads": 16,
                                  "ms_per_view": round((time.perf_counter() - t0) * 1e3 / 16, 1),
                                  "equals_the_device": [x["ms_ssim_per_view"][0] for x in got] == list(m.ms_ssim_per_view[:16])}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
