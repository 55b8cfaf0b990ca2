"""What the deterministic training mode costs, from one process:
  1. the hash grid's parameter-gradient scatter at the headline batch (config 2: 4096 x 64 samples, 2^19 table), fast vs
     deterministic (MIPSF_HG_DETERMINISTIC), event pairs, median of N calls;
  2. the graphed mapping step (forward + backward + FusedAdam) at config 2, default vs deterministic;
  3. ms per frame of the two-room walk (tests/test_gpu_sequence.py's sequence) in both modes;
and the fast scatter once more at the end (the board's clock drifts under load).

    python tools/det_cost.py [--reps 50] [--no-walk]"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mipsfusion_amd import ops, synth  # noqa: E402
from mipsfusion_amd.graph import GraphedSteps, work_stream  # noqa: E402
from mipsfusion_amd.model import JointEncoding  # noqa: E402
from mipsfusion_amd.optim import FusedAdam  # noqa: E402
from oracle import path_cpu  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def headline(dev):
    cfg = synth.config_headline()
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    torch.manual_seed(0)
    m = JointEncoding(cfg, bb, nf).to(dev).train()
    with torch.no_grad():
        m.embed_fn.params.copy_((torch.randn(m.embed_fn.params.shape) * 0.2).to(dev))
    frame = synth.make_frame(cfg, seed=0)
    H, W = frame["depth"].shape
    random.seed(0)
    idx = torch.tensor(random.sample(range(H * W), 4096))
    return cfg, m, [t.to(dev) for t in synth.ray_batch(frame, idx, frame["c2w"])]


def scatter_inputs(dev):
    cfg, m, (ro, rd, rgb, d) = headline(dev)
    keep = {}
    orig = ops.hashgrid_bwd

    def spy(x, params, dout, dparams, meta, layout=0, dx=None, **kw):
        keep.update(x=x.clone(), dout=dout.clone(), layout=layout)
        return orig(x, params, dout, dparams, meta, layout, dx, **kw)
    ops.hashgrid_bwd = spy
    try:
        ret = m.forward(ro, rd, rgb, d, noise=torch.rand(4096, 64, device=dev))
        path_cpu.total_loss(ret, cfg["training"]).backward()
    finally:
        ops.hashgrid_bwd = orig
    return m, keep


def scatter_ms(m, k, det, reps):
    params = m.embed_fn.params.detach()
    dp = torch.zeros_like(params)
    return timed(lambda: ops.hashgrid_bwd(k["x"], params, k["dout"], dp, m.embed_fn.meta, k["layout"], None,
                                          dparams_zero=True, deterministic=det), reps)


def mapping_step_ms(dev, det, reps):
    side = work_stream(dev)
    with torch.cuda.stream(side):
        cfg, m, (ro, rd, rgb, d) = headline(dev)
        m.deterministic = det
        m.accumulate_param_grads_in_place = True
        m.grid_grad_is_zero_at_backward = True
        opt = FusedAdam([{"params": m.decoder.parameters(), "weight_decay": 1e-6, "lr": 0.01},
                         {"params": m.embed_fn.parameters(), "eps": 1e-15, "lr": 0.01}], betas=(0.9, 0.99), capturable=True)
        noise = torch.rand(4096, 64, device=dev)

        def step(_k=0):
            ret = m.forward(ro, rd, rgb, d, noise=noise)
            path_cpu.total_loss(ret, cfg["training"]).backward()
            opt.step(zero_grad=True)
        g = GraphedSteps(step, 1, warmup=2, stream=side)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        ms = timed(g.replay, reps)
    torch.cuda.synchronize()
    return ms


def walk_ms(dev, det):
    from mipsfusion_amd import sequence
    from tests.test_gpu_sequence import _small_two_room_cfg
    cfg = _small_two_room_cfg(quick=False)
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    gt, frames, schedule = synth.two_room_sequence(cfg, 300, kf_every=15)
    prev = torch.cuda.current_stream(dev)
    try:
        seq = sequence.GraphedSequence(cfg, dev, frames, kf_every=15, sampler="device", stream=work_stream(dev),
                                       schedule=schedule, deterministic=det)
        res = seq.run(gt)
    finally:
        torch.cuda.set_stream(prev)
    out = sequence.summarise(res, gt, cfg, "graphs")
    return {k: out[k] for k in ("ms_per_frame_mean", "ms_per_frame_median", "ate_rmse_m", "ate_max_m")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-walk", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m, k = scatter_inputs(dev)
    res = {"scatter_fast_ms": scatter_ms(m, k, False, args.reps),
           "scatter_det_ms": scatter_ms(m, k, True, args.reps)}
    print(json.dumps(res), flush=True)
    res["mapping_step_default_ms"] = mapping_step_ms(dev, False, args.reps)
    res["mapping_step_det_ms"] = mapping_step_ms(dev, True, args.reps)
    print(json.dumps(res), flush=True)
    if not args.no_walk:
        res["walk_default"] = walk_ms(dev, False)
        res["walk_det"] = walk_ms(dev, True)
    res["scatter_fast_ms_again"] = scatter_ms(m, k, False, args.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
