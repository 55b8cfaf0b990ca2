"""CPU: tests/hashgrid_cpu.py (the float64 restatement of csrc/hashgrid.hip and its derived bounds) is held to the fp32 oracle and the
recorded vectors before tests/test_gpu_hashgrid_fp64.py holds the kernels to it:
  * its indices and cells are the oracle's and the recorded ones, its fraction the oracle's bit for bit;
  * the oracle (an honest fp32 implementation in the kernel's operation order: forward, per-level Jacobian, per-level and summed dx)
    and the recorded features stay inside the bounds;
  * the inputs the GPU cases use hold every planted kind, hit every addressing mode, give the part counts the cases are there
    for, have no unresolved double-rounding case and stay clear of underflow;
  * the variant libraries of csrc/variants.mk (tests/test_gpu_hashgrid_variants.py) exist, speak the ABI, are compiled with the
    constants the restatement takes for them (H.BUILDS), and their cases reach what each variant is there for: records whose
    corner membership the accumulate kernel recomputes, bins in more than 8 and 16 parts, records past the staging capacity (in
    the shipped build too), 512 slices a level, pairs that are live only through their routing group."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import tcnn_cpu

from . import hashgrid_cpu as H
from .conftest import load_golden

PLS = float(2.0 ** (math.log2(256 / 16) / 15))       # the project's per-level scale


def ometa(table):
    if table == "hand":
        m = tcnn_cpu.make_grid_meta(16, 2, 14, 16, PLS)
        return dataclasses.replace(m, offsets=H.cut_offsets(m.offsets, H.HAND_LEVEL, H.HAND_SIZE))
    return tcnn_cpu.make_grid_meta(16, 2, table, 16, PLS)


_CASES = {}


def case(table, M, dead=0.3):
    """(meta, levels, x, params, dout, kinds, float64 answer), built once"""
    key = (table, M, dead)
    if key not in _CASES:
        meta = ometa(table)
        lv = H.Levels(meta)
        x, params, dout, kinds = H.build_inputs(lv, M, M + 7, dead)
        _CASES[key] = (meta, lv, x, params, dout, kinds, H.reference(lv, x, params, dout))
    return _CASES[key]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def inside(got, want, bound, what, limit=1.0):
    ratio, stray = H.worst_ratio(got, want, bound)
    assert stray == 0 and ratio <= limit, f"{what}: worst error / bound {ratio:.3f}, {stray} non-zero values where the bound is 0"
    return ratio


@pytest.mark.parametrize("table", [10, 14, 19, "hand"])
def test_indices_cells_and_fraction_are_the_oracles(table):
    meta, lv, x, params, dout, kinds, R = case(table, 2000)
    assert np.array_equal(R["idx"], tcnn_cpu.hashgrid_indices(T(x), meta).numpy())
    for level in range(lv.n_levels):
        cell, frac = tcnn_cpu._cell_and_frac(T(x), meta.scales[level])
        assert np.array_equal(R["c"][:, level].astype(np.int64), cell.numpy())
        assert np.array_equal(R["f"][:, level], frac.numpy())
    assert ((R["idx"] >= 0) & (R["idx"] < np.diff(lv.offsets)[None, :, None])).all()


def test_hand_made_meta_is_mode_2():
    lv = H.Levels(ometa("hand"))
    assert lv.size(H.HAND_LEVEL) == H.HAND_SIZE and H.HAND_SIZE % 8 == 0
    assert [H.level_mode(lv.res[l], lv.size(l)) for l in range(16)] == [0, 0, 0, 1, 1, 2] + [1] * 10
    assert np.array_equal(np.diff(lv.offsets)[:3], [4096, 8000, 13824])
    assert lv.offsets[-1] == H.Levels(ometa(14)).offsets[-1] - (16384 - H.HAND_SIZE)


@pytest.mark.parametrize("tag,table", [("t10", 10), ("t19", 19)])
def test_recorded_indices_and_features(tag, table):
    g = load_golden("hashgrid.npz")
    lv = H.Levels(ometa(table))
    gen = torch.Generator().manual_seed(int(g[f"{tag}.param_seed"]))
    params = ((torch.rand(2 * lv.n_entries, generator=gen) * 2 - 1) * 0.5).numpy()
    x = g[f"{tag}.x"]
    R = H.reference(lv, x, params)
    assert R["fma"][1] == 0
    assert np.array_equal(R["idx"], g[f"{tag}.idx"].astype(np.int64))
    inside(g[f"{tag}.y"].reshape(-1, 16, 2), R["y"], H.bound_y(R), f"recorded {tag}.y")


def test_oracle_forward_and_summed_dx_inside_the_bounds():
    """The issue's trial: 2^14 table, M = 9000.  An honest fp32 implementation in the kernel's order has to fit."""
    for table, M in ((14, 9000), ("hand", 600)):
        meta, lv, x, params, dout, kinds, R = case(table, M)
        y = tcnn_cpu.hashgrid_forward(T(x), T(params), meta).numpy().reshape(M, 16, 2)
        ry = inside(y, R["y"], H.bound_y(R), "oracle forward")
        _, dx = tcnn_cpu.hashgrid_backward(T(x), T(params), T(dout.reshape(M, 32)), meta)
        rx = inside(dx.numpy(), R["dx"], H.bound_dx(R, 16), "oracle summed dx")
        print(f"\n  oracle / bound | {table} M={M} | forward {ry:.3f} | summed dx {rx:.3f}", end="")


@pytest.mark.parametrize("table", [14, "hand"])
def test_oracle_per_level_jacobian_and_dx_inside_the_bounds(table):
    M = 257
    meta, lv, x, params, dout, kinds, R = case(table, M)
    worst_j = worst_d = 0.0
    for level in range(16):
        for feat in range(2):                        # dout = a unit vector: dx IS the Jacobian word (x 1 and + 0 are exact)
            d = np.zeros((M, 16, 2), np.float32)
            d[:, level, feat] = 1.0
            _, dx = tcnn_cpu.hashgrid_backward(T(x), T(params), T(d.reshape(M, 32)), meta)
            worst_j = max(worst_j, inside(dx.numpy(), R["J"][:, level, :, feat], H.bound_J(R)[:, level, :, feat],
                                          f"oracle Jacobian, level {level}"))
        d = np.zeros((M, 16, 2), np.float32)
        d[:, level] = dout[:, level]
        _, dx = tcnn_cpu.hashgrid_backward(T(x), T(params), T(d.reshape(M, 32)), meta)
        worst_d = max(worst_d, inside(dx.numpy(), R["dxl"][:, level], H.bound_dxl(R)[:, level], f"oracle dx of level {level}"))
    print(f"\n  oracle / bound | {table} | Jacobian {worst_j:.3f} | per-level dx {worst_d:.3f}", end="")


def test_outside_cases_meet_what_the_bound_derivation_needs():
    """build_inputs(outside=True): points over [-1.5, 2.5]^3.  The bounds are derived for ANY cell the kernel's own fmaf and floor give,
    on the conditions asserted here: no unresolved fma, every |floor| below 2^31 (both counted in R["fma"][1]), no product near fp32's
    underflow.  And the cases reach what they are there for: negative cells, cells past the resolution, all three addressing modes,
    and an honest fp32 implementation (the oracle) inside the bounds out there."""
    from . import decoder_cpu
    assert (H.X_LO, H.X_HI) == (decoder_cpu.X_LO, decoder_cpu.X_HI)
    modes = set()
    for table, M in H.OUTSIDE_CASES:
        meta = ometa(table)
        lv = H.Levels(meta)
        x, params, dout, kinds = H.build_inputs(lv, M, M + 7, 0.3, outside=True)
        inside_x, _, _, _ = H.build_inputs(lv, M, M + 7, 0.3)
        assert x.min() < -1.3 and x.max() > 2.3 and ((x < 0) | (x > 1)).any(1).mean() > 0.4 and inside_x.shape == x.shape
        R = H.reference(lv, x, params, dout)
        assert R["fma"][1] == 0, f"{R['fma'][1]} unresolved fma or cells beyond 2^31"
        assert R["min_product"] > 2.0 ** -100
        cells = R["c"].astype(np.int64)
        assert (cells >= 2 ** 31).any(), "negative cells (uint32 values above 2^31)"
        assert ((cells < 2 ** 31) & (cells >= np.asarray(lv.res)[None, :, None])).any(), "cells past the level's resolution"
        modes |= R["modes"]
        assert np.array_equal(R["idx"], tcnn_cpu.hashgrid_indices(T(x), meta).numpy())
        y = tcnn_cpu.hashgrid_forward(T(x), T(params), meta).numpy().reshape(M, 16, 2)
        ry = inside(y, R["y"], H.bound_y(R), "oracle forward, outside")
        _, dx = tcnn_cpu.hashgrid_backward(T(x), T(params), T(dout.reshape(M, 32)), meta)
        rx = inside(dx.numpy(), R["dx"], H.bound_dx(R, 16), "oracle summed dx, outside")
        print(f"\n  oracle / bound | outside {table} M={M} | forward {ry:.3f} | summed dx {rx:.3f}", end="")
    assert modes == {0, 1, 2}


@pytest.mark.parametrize("table,M", [(14, 257), (14, 9000), ("hand", 3000), (10, 25000), (19, 3000)])
def test_every_planted_kind_is_present(table, M):
    dead = 0.01 if M in (9000, 25000) else 0.3
    meta, lv, x, params, dout, kinds, R = case(table, M, dead)
    c, f = R["c"], R["f"]
    inside_box = ((x > 0) & (x < 1)).all(1)
    k = kinds
    assert inside_box.sum() > M // 2
    assert ((x[k["near_low"]] < 0) & (x[k["near_low"]] > -0.11)).any(1).all() and k["near_low"].size > 0
    assert ((x[k["near_high"]] > 1) & (x[k["near_high"]] < 1.11)).any(1).all() and k["near_high"].size > 0
    assert (np.abs(x[k["far"]]).max(1) >= 2).all() and np.abs(x).max() <= 4 and k["far"].size > 0
    assert (c[k["cell_minus1"]] == 0xFFFFFFFF).any((1, 2)).all() and k["cell_minus1"].size > 0
    assert ((x[k["exact01"]] == 0) | (x[k["exact01"]] == 1)).any(1).all() and (x == 0).any() and (x == 1).any()
    # a face point: f == 0 on the chosen level, in a coordinate that is not 0 -- four corners with a zero weight.  (k - 0.5) / scale
    # is rounded to fp32, so some land an ulp beside the face: f = ulp or 1 - ulp, the extremes of a weight)
    face = k["face"]
    ff = f[face][:, [1, 4]]
    on_face = ((ff == 0) & (x[face][:, None, :] != 0)).any((1, 2))
    beside = (np.minimum(ff, 1 - ff) < 2.0 ** -12).any((1, 2))
    assert on_face.sum() > 0 and (on_face | beside).all()
    crowd = c[k["crowded"], 15]
    assert k["crowded"].size >= 4 and (crowd == crowd[0]).all()
    assert k["duplicate"].size > 0 and np.array_equal(x[k["duplicate"]], x[k["duplicate_of"]])
    assert not np.intersect1d(k["duplicate"], k["duplicate_of"]).size
    ray = x[k["ray"]].astype(np.float64)
    assert k["ray"].size == 64 and np.array_equal(k["ray"], np.arange(32, 96))
    assert np.abs(np.cross(ray[1:] - ray[0], ray[-1] - ray[0])).max() < 1e-7
    same_cell = (c[k["ray"]][1:, 0] == c[k["ray"]][:-1, 0]).all(1)
    assert same_cell.sum() >= 32                     # the dense run merge has runs to merge on level 0
    # params: both signs, magnitudes over 2^20; dout: over 2^40, with every kind of zero
    assert (params > 0).any() and (params < 0).any()
    assert np.abs(params).max() / np.abs(params).min() > 2.0 ** 19 and np.abs(params).min() >= 2.0 ** -20.01
    nz = np.abs(dout[dout != 0])
    assert nz.max() / nz.min() > 2.0 ** 38 and (dout > 0).any() and (dout < 0).any()
    live = H.live_pairs(dout)
    dead_sample = ~live.any(1)
    assert dead_sample.sum() > 0
    assert (dead_sample[27:32]).all() or dead_sample[31], "the tail of the first ray is dead"
    assert (~live[~dead_sample]).sum() > 0, "dead (sample, level) pairs of live samples"
    assert (live & ((dout[..., 0] == 0) | (dout[..., 1] == 0))).sum() > 0, "one feature of a live pair exactly zero"
    # entries that must come out exactly zero: untouched ones, and ones that only zero weights or dead pairs land on (the 2^10
    # table under 25000 samples has neither: every entry is hit)
    if table != 10:
        assert (R["A_dp"] == 0).any() and R["entries"].size < lv.n_entries


def test_every_addressing_mode_is_hit():
    assert case(10, 2000)[-1]["modes"] == {1}
    assert case(14, 2000)[-1]["modes"] == {0, 1}
    assert case("hand", 2000)[-1]["modes"] == {0, 1, 2}
    # dense walk: the conditional subtract, the real % (far outside) and the uint32 wrap-around each occur
    meta, lv, x, params, dout, kinds, R = case(14, 2000)
    c = R["c"][:, 0]
    raw = c[:, 0] + c[:, 1] * np.uint64(lv.res[0]) + c[:, 2] * np.uint64(lv.res[0] ** 2)
    size = np.uint64(lv.size(0))
    assert (raw < size).any() and ((raw & np.uint64(0xFFFFFFFF)) >= 2 * size).any() and (raw >= np.uint64(1 << 32)).any()


@pytest.mark.parametrize("name,table,M,dead,why", H.SCATTER_CASES)
def test_part_counts_of_the_scatter_cases(name, table, M, dead, why):
    meta, lv, x, params, dout, kinds, R = case(table, M, dead)
    plan = H.scatter_plan(lv, R, H.live_pairs(dout))
    ahead = H.scatter_plan(lv, R, None)
    for p, a in zip(plan, ahead):
        assert (p["records"] <= a["records"]).all() and (a["records"] <= M).all()
    if name == "t14_m9000":
        assert [p["dense"] for p in plan[:4]] == [True, True, True, False]
        assert list(plan[0]["parts"]) == [2] and list(plan[1]["parts"]) == [2], "dense one-slice bins in two parts"
        assert len(plan[2]["parts"]) == 2 and lv.size(2) - 8192 == 5632, "level 2: two slices, the second ragged"
        assert plan[2]["records"].min() > 0 and all(p["parts"].max() == 1 for p in plan[3:])
    if name == "t10_m25000":
        assert all(not p["dense"] and list(p["parts"]) == [2] for p in plan), "hashed one-slice bins in two parts"
        assert all(list(a["parts"]) == [2] for a in ahead)
    if name == "t14_m25000":
        assert list(plan[0]["parts"]) == [4] and list(plan[1]["parts"]) == [4], "dense one-slice bins in four parts"
        assert plan[2]["parts"].max() >= 2 and all(p["parts"].max() == 1 for p in plan[3:])
    if name == "t19_m3000":
        assert all(len(p["parts"]) == 64 for p in plan[9:])
    if name == "hand_m3000":
        p = plan[H.HAND_LEVEL]
        assert len(p["parts"]) == 2 and p["records"].min() > 0 and H.HAND_SIZE - 8192 == 4152
    if name == "t14_m1":
        assert sum(int(p["records"].sum() > 0) for p in plan) >= 1, "the one sample is live on some level"


@pytest.mark.parametrize("table,M,dead", [(t, m, 0.3) for t in (14, "hand") for m in H.FWD_M]
                         + [(c[1], c[2], c[3]) for c in H.SCATTER_CASES + H.MASK_EDGE_CASES])
def test_no_unresolved_rounding_and_no_underflow(table, M, dead):
    R = case(table, M, dead)[-1]
    assert R["fma"][1] == 0, f"{R['fma'][1]} positions whose single rounding could not be settled"
    assert R["min_product"] > 2.0 ** -100, f"smallest non-zero product 2^{math.log2(R['min_product']):.1f}"
    assert np.isfinite(R["y"]).all() and np.isfinite(R["dx"]).all() and np.isfinite(R["dp"]).all()


def test_fma32_rounds_once():
    """scale * x + 0.5 formed in float64 and then rounded to fp32 rounds twice where the float64 sum lands on an fp32 tie."""
    a = np.float32(1 + 2.0 ** -23)
    x = np.array([(1 + 2.0 ** -23) * 2.0 ** -30], np.float32)              # a x = 2^-30 (1 + 2^-22 + 2^-46): 0.5 + a x is inexact
    r, resolved, unresolved = H.fma32(a, x, 0.5)
    assert unresolved == 0
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(x[0])) + Fraction(1, 2)
    lo = np.float32(float(exact))
    cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
    best = min(cands, key=lambda q: abs(Fraction(float(q)) - exact))
    assert r[0] == best
    # a constructed double rounding: a x = 3 * 2^-25 - 3 * 2^-69, so fl64(0.5 + a x) IS the fp32 tie 0.5 + 3 * 2^-25, which
    # ties-to-even sends up to 0.5 + 2^-23; the exact sum lies below the tie and rounds down to 0.5 + 2^-24
    a2 = np.float32(1.5 + 3 * 2.0 ** -23)
    x2 = np.array([2.0 ** -24 * (1 - 2.0 ** -22)], np.float32)
    assert np.float32(np.float64(a2) * np.float64(x2[0]) + 0.5) == np.float32(0.5 + 2.0 ** -23)
    r2, resolved2, unresolved2 = H.fma32(a2, x2, 0.5)
    assert r2[0] == np.float32(0.5 + 2.0 ** -24) and resolved2 == 1 and unresolved2 == 0
    # and against exact rational arithmetic on positions of every size
    rng = np.random.default_rng(5)
    xs = (rng.uniform(-1, 1, 3000) * 2.0 ** rng.uniform(-40, 2, 3000)).astype(np.float32)
    sc = np.float32(4095.37)
    rs, _, un = H.fma32(sc, xs, 0.5)
    assert un == 0
    for q, got in zip(xs, rs):
        exact = Fraction(float(sc)) * Fraction(float(q)) + Fraction(1, 2)
        near = np.float32(float(exact))
        cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
        assert abs(Fraction(float(got)) - exact) == min(abs(Fraction(float(c)) - exact) for c in cands)


# ------------------------------------------------------------------- the variant libraries: the cases reach what they are there for
# (tests/test_gpu_hashgrid_variants.py runs them; here on the restatement alone)
def named(name):
    _, table, M, dead, _ = H.CASES_BY_NAME[name]
    return case(table, M, dead)


def variant_plan(variant, name):
    meta, lv, x, params, dout, kinds, R = named(name)
    build = H.BUILDS[variant]
    live = build.live(dout)
    return lv, R, dout, build, live, H.scatter_plan(lv, R, live, build)


def test_variant_records_are_the_makefiles():
    """H.BUILDS (the constants the restatement takes) and csrc/variants.mk (the flags the libraries are compiled with) agree"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "mipsfusion_amd", "csrc", "variants.mk")) as f:
        listed = H.parse_variants(f.read())
    assert list(listed) == list(H.BUILDS) and set(H.VARIANT_CASES) == set(H.BUILDS)
    for name, (unit, macros) in listed.items():
        assert unit == "hashgrid" and macros and set(macros) <= set(H.BUILD_MACROS), f"{name}: {macros}"
        want = dataclasses.replace(H.DEFAULT, **{H.BUILD_MACROS[m]: v for m, v in macros.items()})
        assert H.BUILDS[name] == want and want != H.DEFAULT, f"{name}: {H.BUILDS[name]} against {macros}"
    # the shipped constants are the sources' defaults
    with open(os.path.join(root, "mipsfusion_amd", "csrc", "hashgrid.hip")) as f:
        src = f.read()
    import re
    for macro, field in H.BUILD_MACROS.items():
        m = re.search(rf"#ifndef {macro}\n#define {macro} ([^\n/]*)", src)
        assert m, macro
        text = m.group(1).strip().replace("u", "")
        value = {"(1 << 24)": 1 << 24, "(10 * RT_BLOCK)": 0}.get(text)
        assert (int(text) if value is None else value) == getattr(H.DEFAULT, field), f"{macro}: {text}"
    assert H.DEFAULT.stage_cap == 10 * H.DEFAULT.rt_block and H.BUILDS["rtb256"].stage_cap == 2560 and H.BUILDS["small"].stage_cap == 512


@pytest.mark.parametrize("variant", list(H.BUILDS))
def test_variant_library_is_built_and_speaks_abi_2(variant):
    from mipsfusion_amd import _lib
    assert _lib.load(_lib.variant_path(variant)).mipsf_abi_version() == 2


@pytest.mark.parametrize("name", H.VARIANT_CASES["maskless"])
def test_maskless_cases_leave_membership_to_the_accumulate_kernel(name):
    """Beyond MIPSF_SC_MASKED_MAX_M a record is the bare sample index and scatter_item recomputes which of the 8 corners are in
    its slice.  That decides something where a sample has corners in two slices of a hashed level: it then has more records
    than one, and each must take only its own corners."""
    lv, R, dout, build, live, plan = variant_plan("maskless", name)
    M = dout.shape[0]
    if name == "t14_m1024":
        assert M == build.masked_max_m, "the last size that still carries masks"
        return
    assert M > build.masked_max_m
    split = [l for l, p in enumerate(plan) if not p["dense"] and p["records"].sum() > live[:, l].sum()]
    if name == "t10_m25000":
        # a 2^10 table has no level of more than one slice, so no sample can have two records on a level: what this case adds
        # is the mask-less record in bins of several parts, all 8 corners members (the pair walk with a full mask)
        assert not split and all(len(p["parts"]) == 1 and not p["dense"] and p["parts"][0] == 2 for p in plan)
        return
    assert split, "no hashed level where a sample has corners in two slices"
    if name == "hand_m3000":
        assert H.HAND_LEVEL in split and H.level_mode(lv.res[H.HAND_LEVEL], lv.size(H.HAND_LEVEL)) == 2
    if name == "t14_m1025":
        assert M == build.masked_max_m + 1


def test_small_cases_fold_many_parts_and_overflow_the_stage():
    build = H.BUILDS["small"]
    lv, R, dout, _, live, plan = variant_plan("small", "t14_m25000")
    assert max(int(p["parts"].max()) for p in plan if p["dense"]) > 16, "a dense bin in more than 16 parts (fold_entry: three rounds of 8)"
    lv10, R10, dout10, _, live10, plan10 = variant_plan("small", "t10_m25000")
    assert all(not p["dense"] and int(p["parts"].min()) > 8 for p in plan10), "every hashed bin in more than 8 parts"
    for lv_, R_, live_ in ((lv, R, live), (lv10, R10, live10)):
        rc = H.route_chunk_records(lv_, R_, live_, build)
        assert rc.shape[0] == (25000 + 2047) // 2048 and rc.max() > build.stage_cap
        assert np.maximum(rc - build.stage_cap, 0).sum() > rc.sum() // 2, "most records leave by the lane-per-record store"
    assert all(M > build.masked_max_m for M in (dout.shape[0], dout10.shape[0]))


def test_shipped_constants_reach_the_overflow_store_on_t19_m3000():
    meta, lv, x, params, dout, kinds, R = named("t19_m3000")
    rc = H.route_chunk_records(lv, R, H.DEFAULT.live(dout), H.DEFAULT)
    assert rc.shape == (2, 16) and H.DEFAULT.stage_cap == 5120
    assert rc[0].max() > H.DEFAULT.stage_cap, f"the first 2048 samples make at most {rc[0].max()} records a level"
    assert rc[0].min() < H.DEFAULT.stage_cap, "and a level that stays inside the stage"


def test_slice10_case_has_512_slices_a_level():
    lv, R, dout, build, live, plan = variant_plan("slice10", "t19_m3000")
    ns = [len(p["parts"]) for p in plan]
    assert max(ns) == H.SC_MAX_NS == 512 and ns.count(512) >= 1
    assert sum(ns) <= H.SC_MAX_BINS and sum(ns) <= 0xFFFF
    assert all(p["records"][-1] > 0 for p, n in zip(plan, ns) if n == 512), "the 512th slice of every such level has records"
    # dense levels cut into slices thinner than a cell's index span (res^2 + res + 1): the fast dense grouping declines them
    assert any(p["dense"] and len(p["parts"]) > 1 and lv.res[l] ** 2 + lv.res[l] + 1 > 1 << build.slice_log2 for l, p in enumerate(plan))
    for name in H.VARIANT_CASES["slice10"]:
        assert sum(len(p["parts"]) for p in variant_plan("slice10", name)[-1]) <= H.SC_MAX_BINS


@pytest.mark.parametrize("variant", ["rt2", "rt4"])
@pytest.mark.parametrize("name", H.VARIANT_CASES["rt2"])
def test_routing_groups_give_dead_pairs_records(variant, name):
    lv, R, dout, build, live, plan = variant_plan(variant, name)
    alone = H.live_pairs(dout)
    assert (live | ~alone).all() and (live & ~alone).sum() > 0, "no pair that is dead by itself and live through its group"
    G = 16 // build.rt_levels
    s, l = np.argwhere(live & ~alone)[0]
    assert alone[s, l % G::G].any() and not alone[s, l]
    assert (~live).sum() > 0, "and pairs that stay dead: the whole group is"
    shipped = H.scatter_plan(lv, R, alone)
    assert any((a["records"] != b["records"]).any() for a, b in zip(shipped, plan)), "the two plans do not differ"
    assert all((a["records"] <= b["records"]).all() for a, b in zip(shipped, plan))


def test_keepzero_plan_is_the_routed_ahead_plan():
    lv, R, dout, build, live, plan = variant_plan("keepzero", "t14_m9000")
    assert live is None
    ahead = H.scatter_plan(lv, R, None)
    assert all(np.array_equal(a["records"], b["records"]) for a, b in zip(ahead, plan))


@pytest.mark.parametrize("name", H.VARIANT_CASES["run1"])
def test_run1_bound_is_the_defaults_minus_the_run_merge(name):
    lv, R, dout, build, live, plan = variant_plan("run1", name)
    k1 = H.roundings_dp(lv, R, plan, build)
    k4 = H.roundings_dp(lv, R, H.scatter_plan(lv, R, H.live_pairs(dout)), H.DEFAULT)
    level = np.searchsorted(np.asarray(lv.offsets), R["entries"], side="right") - 1
    dense = np.array([p["dense"] for p in plan])[level]
    assert np.array_equal(k4[dense] - k1[dense], np.full(dense.sum(), H.SC_RUN - 1.0)) and np.array_equal(k4[~dense], k1[~dense])
    if name == "t14_m25000":
        assert dense.any()
    assert (H.bound_dp(lv, R, plan, build) <= H.bound_dp(lv, R, plan, H.DEFAULT)).all()


@pytest.mark.parametrize("variant,name", [(v, n) for v in ("fence", "run1") for n in H.VARIANT_CASES[v]])
def test_fence_and_run1_cases_have_split_bins(variant, name):
    assert max(int(p["parts"].max()) for p in variant_plan(variant, name)[-1]) >= 2
