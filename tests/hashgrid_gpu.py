"""What the GPU tests of csrc/hashgrid.hip share (tests/test_gpu_hashgrid_fp64.py: the shipped library;
tests/test_gpu_hashgrid_variants.py: the variant libraries of csrc/variants.mk): the grid metas, the cases -- inputs and float64
answer of tests/hashgrid_cpu.py, computed once a process and never written to -- and the assertions, which are the same for both:
EVERY element within its own derived bound, exactly zero where the float64 magnitude sum is zero."""
import math

import numpy as np
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import FEAT_AOS, FEAT_LEVEL_MAJOR

from . import hashgrid_cpu as H

PLS = float(2.0 ** (math.log2(256 / 16) / 15))
LAYOUTS = [("aos", FEAT_AOS), ("level_major", FEAT_LEVEL_MAJOR)]


def gmeta(table):
    if table != "hand":
        return _lib.make_grid_meta(16, 2, table, 16, PLS)
    m = _lib.GridMeta.from_buffer_copy(_lib.make_grid_meta(16, 2, 14, 16, PLS))
    for l, o in enumerate(H.cut_offsets(list(m.offsets)[:17], H.HAND_LEVEL, H.HAND_SIZE)):
        m.offsets[l] = o
    m.n_params = m.offsets[16] * 2
    return m


# ------------------------------------------------------------------------------------------- shared, computed once, never written to
_CASES = {}


class Case:
    def __init__(self, table, M, dead, dev, outside=False):
        self.meta = gmeta(table)
        self.lv = H.Levels(self.meta)
        self.M = M
        self.x, self.params, self.dout, self.kinds = H.build_inputs(self.lv, M, M + 7, dead, outside)
        self.R = H.reference(self.lv, self.x, self.params, self.dout)
        self.xg, self.pg = torch.from_numpy(self.x).to(dev), torch.from_numpy(self.params).to(dev)

    def dout_dev(self, layout, dout=None):
        d = self.dout if dout is None else dout
        d = d.reshape(self.M, 32) if layout == FEAT_AOS else np.ascontiguousarray(d.transpose(1, 0, 2))
        return torch.from_numpy(d).to(self.xg.device)


def case(table, M, dead, dev, outside=False):
    key = (table, M, dead, outside)
    if key not in _CASES:
        _CASES[key] = Case(table, M, dead, dev, outside)
    return _CASES[key]


def held(form, tag, got, want, bound):
    """every element within its bound, exact zeros where the bound is zero; -> the worst error / bound"""
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    ratio, stray = H.worst_ratio(got.reshape(np.shape(want)), want, bound)
    print(f"\n  fp64 | {form} | {tag} | worst error / bound {ratio:.3f}", end="")
    assert stray == 0 and ratio <= 1.0, \
        f"{form}, {tag}: worst error / bound {ratio:.3f}; {stray} non-zero values where the float64 magnitude sum is exactly 0"
    return ratio


def held_dparams(form, tag, c, dp, want, bound):
    got = dp.cpu().numpy().reshape(-1, 2)
    e = c.R["entries"]
    other = np.ones(c.lv.n_entries, bool)
    other[e] = False
    assert not got[other].any(), f"{form}, {tag}: {np.count_nonzero(got[other])} non-zero values in entries no corner lands on"
    return held(form, tag, got[e], want, bound)


def all_dead_gradient_writes_nothing(c, layout):
    """a gradient that is zero everywhere leaves dparams as it is, bit for bit, with and without records for the dead pairs"""
    dg = c.dout_dev(layout, np.zeros_like(c.dout))
    mark = torch.full_like(c.pg, 1.25)
    ops.hashgrid_bwd(c.xg, c.pg, dg, mark, c.meta, layout, None)
    assert bool((mark == 1.25).all()), "an all-dead gradient changed dparams"
    dp = torch.zeros_like(c.pg)
    ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None, dparams_zero=True)
    assert not bool(dp.any()), "an all-dead gradient wrote into a fresh dparams"
