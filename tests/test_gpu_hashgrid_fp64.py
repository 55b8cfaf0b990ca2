"""GPU (-m gpu): every kernel of csrc/hashgrid.hip that the default (non-deterministic) path runs -- hashgrid_fwd_kernel in both
layouts with and without the Jacobian, hashgrid_dx_kernel + hashgrid_dx_reduce_kernel, hashgrid_dx_jac_kernel, scatter_route_kernel,
hashgrid_scatter_persist_kernel and hashgrid_scatter_reduce_kernel -- against the float64 restatement of tests/hashgrid_cpu.py.

Every assertion is: EVERY element within its own derived bound (k roundings of 2^-24 on the sum of the magnitudes of the element's
terms, tests/hashgrid_cpu.py), exactly zero where that sum is zero.  No outlier share, nothing relative to the array's maximum, no
measured tolerance.  tests/test_hashgrid_fp64_cpu.py holds the restatement, the bounds and the inputs to the fp32 oracle first.

The worst error / bound each form reached on an MI355X is recorded in DESIGN.md, "The hash-grid kernels against float64"."""
import numpy as np
import pytest
import torch

from mipsfusion_amd import ops
from mipsfusion_amd._lib import FEAT_AOS
from oracle import tcnn_cpu

from . import hashgrid_cpu as H
from .hashgrid_gpu import LAYOUTS, PLS, all_dead_gradient_writes_nothing, case, gmeta, held, held_dparams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def test_level_tables_are_the_oracles():
    for table in (10, 14, 19):
        a, b = H.Levels(gmeta(table)), H.Levels(tcnn_cpu.make_grid_meta(16, 2, table, 16, PLS))
        assert a.offsets == b.offsets and a.res == b.res and np.array_equal(a.scales, b.scales)
    hand = H.Levels(gmeta("hand"))
    assert hand.size(H.HAND_LEVEL) == H.HAND_SIZE and H.level_mode(hand.res[H.HAND_LEVEL], H.HAND_SIZE) == 2


# ----------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("M", H.FWD_M)
@pytest.mark.parametrize("table", [14, "hand"])
def test_forward_and_jacobian(dev, table, M):
    c = case(table, M, 0.3, dev)
    R = c.R
    assert np.array_equal(ops.hashgrid_indices(c.xg, c.meta).cpu().numpy().astype(np.int64), R["idx"])
    by, bj = H.bound_y(R), H.bound_J(R)
    worst = 0.0
    for name, layout in LAYOUTS:
        def std(y):
            y = y.cpu().numpy()
            return y.reshape(M, 16, 2) if layout == FEAT_AOS else y.transpose(1, 0, 2)
        y = ops.hashgrid_fwd(c.xg, c.pg, c.meta, layout)
        yj, jac = ops.hashgrid_fwd(c.xg, c.pg, c.meta, layout, with_jac=True)
        worst = max(worst, held("forward", f"{table} M={M} {name}", std(y), R["y"], by))
        worst = max(worst, held("forward (with the Jacobian)", f"{table} M={M} {name}", std(yj), R["y"], by))
        worst = max(worst, held("Jacobian", f"{table} M={M} {name}", jac.cpu().numpy().transpose(2, 0, 1, 3), R["J"], bj))


# ---------------------------------------------------------------------------------------------------------------------------- dx
def gather_dx(c, layout, dout_g, dx):
    ops.hashgrid_bwd(c.xg, c.pg, dout_g, None, c.meta, layout, dx)


@pytest.mark.parametrize("M", H.FWD_M)
@pytest.mark.parametrize("table", [14, "hand"])
def test_summed_dx_both_paths(dev, table, M):
    c = case(table, M, 0.3, dev)
    R = c.R
    b = H.bound_dx(R, 16)
    for name, layout in LAYOUTS:
        dg = c.dout_dev(layout)
        _, jac = ops.hashgrid_fwd(c.xg, c.pg, c.meta, layout, with_jac=True)
        for form, run in (("dx (gather)", lambda dx: gather_dx(c, layout, dg, dx)),
                          ("dx (saved Jacobian)", lambda dx: ops.hashgrid_dx_from_jac(jac, dg, dx, c.meta, layout))):
            dx = torch.zeros(M, 3, device=dev)
            run(dx)
            first = dx.cpu().numpy().astype(np.float64)
            held(form, f"{table} M={M} {name}", first, R["dx"], b)
            run(dx)                                  # dx accumulates: fl(dx0 + a) rounds the result once more
            want = first + R["dx"]
            held(form + ", second call", f"{table} M={M} {name}", dx, want, b * (1 + H.U) + H.U * np.abs(want))


@pytest.mark.parametrize("table", [14, "hand"])
def test_per_level_dx_through_the_public_api(dev, table):
    """One call per level with only that level's gradient non-zero: the other levels add exact zeros, so the result is that
    level's partial alone -- the words hashgrid_dx_kernel writes and no summed check can tell apart."""
    M = 257
    c = case(table, M, 0.3, dev)
    R = c.R
    _, jac = ops.hashgrid_fwd(c.xg, c.pg, c.meta, FEAT_AOS, with_jac=True)
    bl = H.bound_dxl(R)
    for level in range(16):
        d = np.zeros_like(c.dout)
        d[:, level] = c.dout[:, level]
        dg = c.dout_dev(FEAT_AOS, d)
        dx = torch.zeros(M, 3, device=dev)
        gather_dx(c, FEAT_AOS, dg, dx)
        held("per-level dx (gather)", f"{table} level {level}", dx, R["dxl"][:, level], bl[:, level])
        dxj = torch.zeros(M, 3, device=dev)
        ops.hashgrid_dx_from_jac(jac, dg, dxj, c.meta, FEAT_AOS)
        held("per-level dx (saved Jacobian)", f"{table} level {level}", dxj, R["dxl"][:, level], bl[:, level])


# ---------------------------------------------------------------------------------------------------------------- routed scatter
@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("lname,layout", LAYOUTS)
@pytest.mark.parametrize("name,table,M,dead,why", H.SCATTER_CASES)
def test_routed_scatter(dev, name, table, M, dead, why, lname, layout, fresh):
    c = case(table, M, dead, dev)
    R = c.R
    b = H.bound_dp(c.lv, R, H.scatter_plan(c.lv, R, H.live_pairs(c.dout)))
    dg = c.dout_dev(layout)
    dp = torch.zeros_like(c.pg)
    ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None, dparams_zero=fresh)
    first = dp.cpu().numpy().reshape(-1, 2)[R["entries"]].astype(np.float64)
    held_dparams("scatter" + (", dparams_zero" if fresh else ""), f"{name} {lname}", c, dp, R["dp"], b)
    if not fresh:                                    # a second call into the non-zero result: one more rounding of the sum
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None)
        want = first + R["dp"]
        held_dparams("scatter, second call", f"{name} {lname}", c, dp, want, b * (1 + H.U) + H.U * np.abs(want))


@pytest.mark.parametrize("name,table,M,dead,why", H.SCATTER_CASES)
def test_routed_scatter_routed_ahead(dev, name, table, M, dead, why):
    """mipsf_hashgrid_route sees no gradient: every sample gets its records, the dead pairs add exact zeros"""
    c = case(table, M, dead, dev)
    R = c.R
    b = H.bound_dp(c.lv, R, H.scatter_plan(c.lv, R, None))
    dp = torch.zeros_like(c.pg)
    routed = ops.hashgrid_route_ahead(c.xg, c.meta)
    ops.hashgrid_bwd(c.xg, c.pg, c.dout_dev(FEAT_AOS), dp, c.meta, FEAT_AOS, None, routed=routed)
    held_dparams("scatter, routed ahead", name, c, dp, R["dp"], b)


# ----------------------------------------------------------------------------------------------------- points outside the unit box
@pytest.mark.parametrize("lname,layout", LAYOUTS)
@pytest.mark.parametrize("table,M", H.OUTSIDE_CASES)
def test_points_outside_the_unit_box(dev, table, M, lname, layout):
    """x over [-1.5, 2.5]^3, where real rays put their samples: negative cells, wrapped corners, all three addressing modes
    (tests/test_hashgrid_fp64_cpu.py asserts that they occur) -- forward, Jacobian, d x by both paths and the routed scatter under
    the same derived bounds as the interior points"""
    c = case(table, M, 0.3, dev, outside=True)
    R = c.R
    tag = f"outside {table} M={M} {lname}"
    assert np.array_equal(ops.hashgrid_indices(c.xg, c.meta).cpu().numpy().astype(np.int64), R["idx"])

    def std(y):
        y = y.cpu().numpy()
        return y.reshape(M, 16, 2) if layout == FEAT_AOS else y.transpose(1, 0, 2)
    held("forward", tag, std(ops.hashgrid_fwd(c.xg, c.pg, c.meta, layout)), R["y"], H.bound_y(R))
    yj, jac = ops.hashgrid_fwd(c.xg, c.pg, c.meta, layout, with_jac=True)
    held("forward (with the Jacobian)", tag, std(yj), R["y"], H.bound_y(R))
    held("Jacobian", tag, jac.cpu().numpy().transpose(2, 0, 1, 3), R["J"], H.bound_J(R))
    dg = c.dout_dev(layout)
    for form, run in (("dx (gather)", lambda dx: gather_dx(c, layout, dg, dx)),
                      ("dx (saved Jacobian)", lambda dx: ops.hashgrid_dx_from_jac(jac, dg, dx, c.meta, layout))):
        dx = torch.zeros(M, 3, device=dev)
        run(dx)
        held(form, tag, dx, R["dx"], H.bound_dx(R, 16))
    b = H.bound_dp(c.lv, R, H.scatter_plan(c.lv, R, H.live_pairs(c.dout)))
    for fresh in (False, True):
        dp = torch.zeros_like(c.pg)
        ops.hashgrid_bwd(c.xg, c.pg, dg, dp, c.meta, layout, None, dparams_zero=fresh)
        held_dparams("scatter" + (", dparams_zero" if fresh else ""), tag, c, dp, R["dp"], b)


@pytest.mark.parametrize("lname,layout", LAYOUTS)
def test_all_dead_gradient_writes_nothing(dev, lname, layout):
    all_dead_gradient_writes_nothing(case(14, 9000, 0.01, dev), layout)
