"""GPU (-m gpu): the fold of split bins inside hashgrid_scatter_persist_kernel (csrc/hashgrid.hip, scatter_item).

A bin whose records are cut into several parts leaves one partial slice per part; the workgroup that publishes the bin's last
partial slice folds them into dparams, in part order.  What is held here:

  value gate      EVERY element of dparams within the per-element float64 bound of tests/hashgrid_cpu.py (the one
                  tests/test_gpu_hashgrid_fp64.py uses), exact zeros where no corner lands -- for the fold inside the kernel and,
                  on the same inputs, for the fold as a launch of its own (MIPSF_SC_FOLD_LAUNCH=1).  The two are not compared bit
                  for bit: the order of a bin's records depends on the schedule in both.
  counter block   after every call every word of the kept block except `first` / `parts` reads zero: three calls in a row with
                  different liveness patterns, and three replays of one captured call with different inputs in its static buffers.
  it does fold    bins with parts > 1 exist (read from `parts` of the block, and equal to the CPU restatement of the plan).

Shapes: M live samples on ray-coherent points (rays of 64 samples), every (sample, level) pair live, so a one-slice dense bin
holds exactly M records: 64 (one part), 8192 / 8193 (one and two parts of MIPSF_SC_PART_DENSE = 8192), 20000 (three), 24577
(four; with a 2^13 table every hashed level is one slice of 24577 records: two parts of MIPSF_SC_PART = 24576)."""
import math
import os

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import FEAT_AOS, FEAT_LEVEL_MAJOR

from . import hashgrid_cpu as H

pytestmark = pytest.mark.gpu
PLS = float(2.0 ** (math.log2(256 / 16) / 15))
LAYOUTS = [("aos", FEAT_AOS), ("level_major", FEAT_LEVEL_MAJOR)]
# (M, log2 of the table size)
SHAPES = [(64, 14), (8192, 14), (8193, 14), (20000, 14), (24577, 13)]
SWITCH = "MIPSF_SC_FOLD_LAUNCH"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def ray_points(M, seed):
    """M points along rays of 64 samples each (the last ray is cut short), inside the unit box"""
    rng = np.random.default_rng(seed)
    n = (M + 63) // 64
    o = rng.uniform(0.05, 0.45, (n, 1, 3))
    d = rng.uniform(0.1, 0.5, (n, 1, 3))
    t = ((np.arange(64) + 0.5) / 64.0)[None, :, None]
    return np.ascontiguousarray((o + t * d).reshape(-1, 3)[:M].astype(np.float32))


def gradient(M, seed, pattern):
    """dout [M,16,2] fp32.  all: every pair live; tails: the second half of every ray dead; holes: 30 % of the samples and
    10 % of the pairs dead; none: all dead"""
    rng = np.random.default_rng(seed)
    dout = (rng.choice([-1.0, 1.0], (M, 16, 2)) * 2.0 ** rng.uniform(-20, 4, (M, 16, 2))).astype(np.float32)
    if pattern == "tails":
        dout[(np.arange(M) % 64) >= 32] = 0
    elif pattern == "holes":
        dout[rng.random(M) < 0.3] = 0
        dout[rng.random((M, 16)) < 0.1] = 0
    elif pattern == "none":
        dout[:] = 0
    else:
        assert pattern == "all"
    return dout


_CASES = {}


class Case:
    """inputs, float64 reference, bound and the expected parts of every bin; computed once, never written to"""

    def __init__(self, M, table, pattern, dev):
        self.M = M
        self.meta = _lib.make_grid_meta(16, 2, table, 16, PLS)
        self.lv = H.Levels(self.meta)
        self.x = ray_points(M, M + table)
        self.dout = gradient(M, M + 3, pattern)
        self.R = H.reference(self.lv, self.x, np.zeros(2 * self.lv.n_entries, np.float32), self.dout)
        plan = H.scatter_plan(self.lv, self.R, H.live_pairs(self.dout))
        self.parts = np.concatenate([p["parts"] for p in plan])
        self.dense_bins = sum(len(p["parts"]) for p in plan if p["dense"])       # (the dense levels come first)
        self.bound = H.bound_dp(self.lv, self.R, plan)
        self.xg = torch.from_numpy(self.x).to(dev)
        self.pg = torch.zeros(2 * self.lv.n_entries, device=dev)
        self.layout_words = _lib.hashgrid_counter_layout(self.meta)

    def dout_dev(self, layout, dout=None):
        d = self.dout if dout is None else dout
        d = d.reshape(self.M, 32) if layout == FEAT_AOS else np.ascontiguousarray(d.transpose(1, 0, 2))
        return torch.from_numpy(d).to(self.xg.device)


def case(M, table, pattern, dev):
    key = (M, table, pattern)
    if key not in _CASES:
        _CASES[key] = Case(M, table, pattern, dev)
    return _CASES[key]


def gate(tag, c, dp, base=None):
    """every element of dp within its bound of base + the float64 table gradient; entries no corner lands on keep base exactly"""
    got = dp.detach().cpu().numpy().reshape(-1, 2)
    e = c.R["entries"]
    other = np.ones(c.lv.n_entries, bool)
    other[e] = False
    want, bound = c.R["dp"], c.bound
    if base is None:
        assert not got[other].any(), f"{tag}: {np.count_nonzero(got[other])} non-zero values in entries no corner lands on"
    else:
        b2 = base.reshape(-1, 2)
        assert np.array_equal(got[other], b2[other]), f"{tag}: entries no corner lands on were changed"
        want = b2[e].astype(np.float64) + want                 # fl(base + s): the sum is rounded once more
        bound = bound * (1 + H.U) + H.U * np.abs(want)
    ratio, stray = H.worst_ratio(got[e], want, bound)
    print(f"\n  fold | {tag} | worst error / bound {ratio:.3f}", end="")
    assert stray == 0 and ratio <= 1.0, \
        f"{tag}: worst error / bound {ratio:.3f}; {stray} non-zero values where the float64 magnitude sum is exactly 0"


def block_ready(tag, c, counters, parts_want=None):
    """every word of the counter block except first / parts is zero; -> parts of every bin"""
    w = c.layout_words
    blk = counters.cpu().numpy().astype(np.int64)
    assert blk.size == w["end"] and w["first"] + w["n_bins"] == w["parts"]
    assert not blk[:w["first"]].any(), f"{tag}: counts / head / tickets / arrivals not left at zero: {np.flatnonzero(blk[:w['first']])[:8]}"
    assert not blk[w["parts"] + w["n_bins"]:].any(), f"{tag}: the block's padding was written"
    parts = blk[w["parts"]:w["parts"] + w["n_bins"]]
    if parts_want is not None:
        assert np.array_equal(parts, parts_want), f"{tag}: parts of the bins differ from the plan's restatement"
    return parts


class fold_launch:
    """the fold as a launch of its own (the switch is read by every call)"""

    def __enter__(self):
        self.old = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = self.old


@pytest.mark.parametrize("lname,layout", LAYOUTS)
@pytest.mark.parametrize("M,table", SHAPES)
def test_fold_values_and_block(dev, M, table, lname, layout):
    c = case(M, table, "all", dev)
    counters = ops._scatter_counters(dev, c.meta)
    dg = c.dout_dev(layout)
    dense = c.parts[:c.dense_bins]
    assert int(dense.max()) == (M + H.SC_PART_DENSE - 1) // H.SC_PART_DENSE, "a one-slice dense bin holds every sample"
    if M == 24577:
        assert int(c.parts[c.dense_bins:].max()) == 2, "a hashed bin crosses MIPSF_SC_PART"
    for fresh in (True, False):
        tag = f"M={M} {lname}" + (" fresh" if fresh else "")
        dp = torch.zeros_like(c.pg)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None, dparams_zero=fresh)
        parts = block_ready(tag, c, counters, c.parts)
        assert bool((parts > 1).any()) == (M > H.SC_PART_DENSE), f"{tag}: bins with several parts"
        gate(tag, c, dp)
        dq = torch.zeros_like(c.pg)
        with fold_launch():
            ops.hashgrid_bwd(c.xg, c.pg, dg, dq, c.meta, layout, None, dparams_zero=fresh)
        block_ready(tag + " (fold launch)", c, counters, c.parts)
        gate(tag + " (fold launch)", c, dq)


@pytest.mark.parametrize("lname,layout", LAYOUTS)
def test_fold_adds_into_a_nonzero_gradient(dev, lname, layout):
    c = case(20000, 14, "all", dev)
    rng = np.random.default_rng(5)
    base = (rng.choice([-1.0, 1.0], 2 * c.lv.n_entries) * 2.0 ** rng.uniform(-12, 6, 2 * c.lv.n_entries)).astype(np.float32)
    counters = ops._scatter_counters(dev, c.meta)
    dg = c.dout_dev(layout)
    dp = torch.from_numpy(base).to(dev)
    ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None)
    assert bool((block_ready("into non-zero", c, counters, c.parts) > 1).any())
    gate(f"into non-zero {lname}", c, dp, base)
    dq = torch.from_numpy(base).to(dev)
    with fold_launch():
        ops.hashgrid_bwd(c.xg, c.pg, dg, dq, c.meta, layout, None)
    gate(f"into non-zero {lname} (fold launch)", c, dq, base)


@pytest.mark.parametrize("lname,layout", LAYOUTS)
def test_all_dead_batch_has_no_items(dev, lname, layout):
    c = case(20000, 14, "all", dev)
    counters = ops._scatter_counters(dev, c.meta)
    dg = c.dout_dev(layout, gradient(c.M, 1, "none"))
    mark = torch.full_like(c.pg, 1.25)
    ops.hashgrid_bwd(c.xg, c.pg, dg, mark, c.meta, layout, None)
    assert bool((mark == 1.25).all()), "an all-dead gradient changed dparams"
    assert not block_ready("all dead", c, counters).any(), "an all-dead batch has no items"
    dp = torch.zeros_like(c.pg)
    ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None, dparams_zero=True)
    assert not bool(dp.any()), "an all-dead gradient wrote into a fresh dparams"
    block_ready("all dead, fresh", c, counters)


PATTERNS = ("all", "tails", "holes")


def test_three_calls_on_one_kept_block(dev):
    """different liveness patterns, hence different parts per bin, one after the other on the same block"""
    counters = None
    seen = []
    for pattern in PATTERNS + ("none",) + PATTERNS[::-1]:
        dp = None
        if pattern == "none":
            c = case(20000, 14, "all", dev)
            dg = c.dout_dev(FEAT_LEVEL_MAJOR, gradient(c.M, 1, "none"))
        else:
            c = case(20000, 14, pattern, dev)
            dg = c.dout_dev(FEAT_LEVEL_MAJOR)
        counters = ops._scatter_counters(dev, c.meta) if counters is None else counters
        assert counters is ops._scatter_counters(dev, c.meta), "one kept block for the grid"
        dp = torch.zeros_like(c.pg)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, FEAT_LEVEL_MAJOR, None, dparams_zero=True)
        if pattern == "none":
            assert not block_ready("kept block, none", c, counters).any() and not bool(dp.any())
            continue
        parts = block_ready(f"kept block, {pattern}", c, counters, c.parts)
        seen.append(tuple(parts))
        gate(f"kept block, {pattern}", c, dp)
    assert len(set(seen)) >= 2, "the liveness patterns give different parts"
    assert all(max(p) > 1 for p in seen)


def test_captured_call_replayed_with_other_inputs(dev):
    cases = [case(20000, 14, p, dev) for p in PATTERNS]
    c0 = cases[0]
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    xs, ds, dp = c0.xg.clone(), c0.dout_dev(FEAT_LEVEL_MAJOR).clone(), torch.zeros_like(c0.pg)
    with torch.cuda.stream(stream):              # the stream's kept block is made (zero) here, outside the capture
        ops.hashgrid_bwd(xs, c0.pg, ds, dp, c0.meta, FEAT_LEVEL_MAJOR, None, dparams_zero=True)
        counters = ops._scatter_counters(dev, c0.meta)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        assert ops._scatter_counters(dev, c0.meta) is counters
        dp.zero_()
        ops.hashgrid_bwd(xs, c0.pg, ds, dp, c0.meta, FEAT_LEVEL_MAJOR, None, dparams_zero=True)
    for c in cases[::-1]:
        xs.copy_(c.xg)
        ds.copy_(c.dout_dev(FEAT_LEVEL_MAJOR))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert bool((block_ready(f"replay, {PATTERNS[cases.index(c)]}", c, counters, c.parts) > 1).any())
        gate(f"replay, {PATTERNS[cases.index(c)]}", c, dp)
