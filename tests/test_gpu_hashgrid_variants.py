"""GPU (-m gpu): the routed hash-grid scatter (scatter_route_kernel, scatter_item, hashgrid_scatter_persist_kernel,
hashgrid_scatter_reduce_kernel) in every variant library of csrc/variants.mk, against the float64 restatement of
tests/hashgrid_cpu.py taken with THAT build's constants (H.BUILDS).

  maskless, small, slice10   paths the shipped library holds behind a size -- records without a corner mask (beyond 2^24 samples),
                             bins folded over more than 8 and 16 parts with most records past the staging capacity, 512 slices a
                             level (a 2^22 table) -- reached at test sizes by lowering the constant that gates them;
  the others                 the build switches hashgrid.hip keeps as the A/B evidence for its defaults.

A variant is loaded into this process (mipsfusion_amd._lib.use_library): ops.* runs unchanged, every buffer size is the
variant's own plan's, nothing is compiled and no process is started.  Each (variant, case, layout) is a test of its own.  Every
value assertion is held_dparams of tests/hashgrid_gpu.py -- EVERY element within k roundings of 2^-24 on the float64 magnitude sum
of its terms, k counted from the build's constants; exact zeros where that sum is zero and in entries no corner lands on -- into a
zero dparams, into the non-zero result (one more rounding) and into a dparams the caller vouches is zero.  Beside it: the kept
counter block reads zero in front of `first` after every call, and dx of the same call is the shipped library's bit for bit (the
dx kernels see none of the switches).

tests/test_hashgrid_fp64_cpu.py shows on the restatement that each case reaches what its variant is there for.  The worst
error / bound every variant reached on an MI355X is recorded in DESIGN.md, "The hash-grid kernels against float64"."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import FEAT_AOS

from . import hashgrid_cpu as H
from .hashgrid_gpu import LAYOUTS, all_dead_gradient_writes_nothing, case, held_dparams
from .test_gpu_scatter_fold import fold_launch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def get(name, dev):
    _, table, M, dead, _ = H.CASES_BY_NAME[name]
    return case(table, M, dead, dev)


_SHIPPED_DX = {}


def shipped_dx(name, lname, layout, c):
    """dx of the shipped library for the case (the call that also scatters), computed once"""
    key = (name, lname)
    if key not in _SHIPPED_DX:
        dx = torch.zeros(c.M, 3, device=c.xg.device)
        ops.hashgrid_bwd(c.xg, c.pg, c.dout_dev(layout), torch.zeros_like(c.pg), c.meta, layout, dx)
        _SHIPPED_DX[key] = dx.cpu().numpy()
    return _SHIPPED_DX[key]


def block_zero(tag, c):
    """the kept counter block (sized by the loaded build's plan) reads zero in front of `first`"""
    w = _lib.hashgrid_counter_layout(c.meta)
    blk = ops._scatter_counters(c.xg.device, c.meta).cpu().numpy()
    assert blk.size == w["end"]
    bad = np.flatnonzero(blk[:w["first"]])
    assert bad.size == 0, f"{tag}: counts / head / tickets / arrivals not left at zero: words {bad[:8]}"
    return blk[w["parts"]:w["parts"] + w["n_bins"]].astype(np.int64)


def run_pair(dev, variant, name, lname, layout):
    c = get(name, dev)
    R, build = c.R, H.BUILDS[variant]
    plan = H.scatter_plan(c.lv, R, build.live(c.dout), build)
    b = H.bound_dp(c.lv, R, plan, build)
    dx_want = shipped_dx(name, lname, layout, c)
    dg = c.dout_dev(layout)
    tag = f"{variant} {name} {lname}"
    with _lib.use_library(_lib.variant_path(variant)):
        dp = torch.zeros_like(c.pg)
        dx = torch.zeros(c.M, 3, device=dev)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, dx)
        parts = block_zero(tag, c)
        assert np.array_equal(parts, np.concatenate([p["parts"] for p in plan])), f"{tag}: parts of the bins differ from the plan's restatement"
        assert np.array_equal(dx.cpu().numpy().view(np.uint32), dx_want.view(np.uint32)), f"{tag}: dx differs from the shipped library's"
        first = dp.cpu().numpy().reshape(-1, 2)[R["entries"]].astype(np.float64)
        held_dparams("scatter", tag, c, dp, R["dp"], b)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None)       # into the non-zero result: one more rounding of the sum
        block_zero(tag + ", second call", c)
        want = first + R["dp"]
        held_dparams("scatter, second call", tag, c, dp, want, b * (1 + H.U) + H.U * np.abs(want))
        dq = torch.zeros_like(c.pg)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dq, c.meta, layout, None, dparams_zero=True)
        block_zero(tag + ", dparams_zero", c)
        held_dparams("scatter, dparams_zero", tag, c, dq, R["dp"], b)


PAIRS = [pytest.param(v, n, ln, lay, id=f"{v}-{n}-{ln}") for v, names in H.VARIANT_CASES.items() for n in names for ln, lay in LAYOUTS]


@pytest.mark.parametrize("variant,name,lname,layout", PAIRS)
def test_variant_scatter(dev, variant, name, lname, layout):
    run_pair(dev, variant, name, lname, layout)


@pytest.mark.parametrize("variant,name,lname,layout", [p for p in PAIRS if p.values[0] == "small"])
def test_small_parts_folded_by_a_launch(dev, variant, name, lname, layout):
    """bins in more than 8 and more than 16 parts through hashgrid_scatter_reduce_kernel (MIPSF_SC_FOLD_LAUNCH=1)"""
    with fold_launch():
        run_pair(dev, variant, name, lname, layout)


def test_maskless_routed_ahead(dev):
    """mipsf_hashgrid_route sees no gradient: every sample gets its (mask-less) records, the dead pairs add exact zeros"""
    c = get("t14_m9000", dev)
    build = H.BUILDS["maskless"]
    b = H.bound_dp(c.lv, c.R, H.scatter_plan(c.lv, c.R, None, build), build)
    with _lib.use_library(_lib.variant_path("maskless")):
        dp = torch.zeros_like(c.pg)
        routed = ops.hashgrid_route_ahead(c.xg, c.meta)
        ops.hashgrid_bwd(c.xg, c.pg, c.dout_dev(FEAT_AOS), dp, c.meta, FEAT_AOS, None, routed=routed)
        held_dparams("scatter, routed ahead", "maskless t14_m9000", c, dp, c.R["dp"], b)


@pytest.mark.parametrize("lname,layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["rt2", "rt4", "keepzero"])
def test_all_dead_gradient_writes_nothing(dev, variant, lname, layout):
    """rt2 / rt4: no group has a live level, no records; keepzero: every pair has records and each adds +-0"""
    with _lib.use_library(_lib.variant_path(variant)):
        all_dead_gradient_writes_nothing(get("t14_m9000", dev), layout)
        block_zero(f"{variant} all dead {lname}", get("t14_m9000", dev))


def test_use_library_hands_the_shipped_library_back(dev):
    shipped = _lib.lib()
    c = get("t14_m1", dev)
    ops._scatter_counters(dev, c.meta)
    with _lib.use_library(_lib.variant_path("slice10")) as h:
        assert _lib.lib() is h and h is not shipped
        assert not any(len(cache) for cache in _lib.KEPT_BLOCK_CACHES), "kept blocks of the shipped build handed to a variant"
        n = _lib.hashgrid_counter_layout(c.meta)["n_bins"]
        ops._scatter_counters(dev, c.meta)
    assert _lib.lib() is shipped
    assert not any(len(cache) for cache in _lib.KEPT_BLOCK_CACHES), "kept blocks of a variant handed to the shipped build"
    assert _lib.hashgrid_counter_layout(c.meta)["n_bins"] < n, "the size query was not the variant's own plan's"
