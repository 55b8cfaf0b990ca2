"""CPU: holds tests/render_cpu.py -- the inputs and the float64 answer that tests/test_gpu_render_fp64.py compares the render,
loss and ray-gradient kernels with -- to its conditions: fp32 and float64 take the same branch at every discrete decision of
every case the GPU tests use, the planted ties and edges are really there (a missing one FAILS), ``counts`` is what the losses
count, the float64 loss gradients are the reference's recorded ones, and the yardstick (fp32 oracle against float64) is printed."""
import numpy as np
import pytest
import torch

from oracle import path_cpu

from . import render_cpu as R
from .conftest import load_golden

ALL = R.CASES
EDGE_MODES = [(k, m) for k in R.EDGE_CASES for m in ("invalid", "none")]


def test_case_list_covers_what_the_gpu_file_promises():
    shapes = [(n, s) for n, s, *_ in ALL]
    assert {s for n, s in shapes if n == 17} == {1, 2, 63, 64, 65, 127, 128, 129, 192, 255, 256}
    for s in (64, 192):
        assert {n for n, s_ in shapes if s_ == s} == {1, 15, 16, 17, 33}
    for lo, hi in ((0, 64), (64, 128), (128, 256)):
        sub = [c for c in ALL if lo < c[1] <= hi]
        assert {c[3] for c in sub} == {0.0, 0.01} and {c[4] for c in sub} == {0, 1}, (lo, hi)


@pytest.mark.parametrize("key", ALL, ids=R.case_id)
def test_inputs_are_on_the_lattice(key):
    c = R.case_of(key)
    N, S = key[:2]
    z, d, sdf = c["z"], c["target_d"], c["raw"][..., 3]
    assert c["raw"].dtype == z.dtype == d.dtype == c["target_rgb"].dtype == torch.float32 and c["counts"].dtype == torch.int32
    assert c["raw"].shape == (N, S, 10) and z.shape == (N, S) and d.shape == (N, 1) and c["counts"].shape == (N, 2)
    usual = torch.ones(N, dtype=torch.bool)
    if "no_depth_near" in c["planted"]:
        usual[c["planted"]["no_depth_near"]] = False             # (the one ray with samples below 0.25: test_planted_rays_are_there)
    assert bool(((z * 256) == (z * 256).round()).all()) and float(z.min()) > 0.0 and float(z.max()) <= 3.5
    assert not bool(usual.any()) or float(z[usual].min()) >= 0.25
    assert S == 1 or bool((z[:, 1:] > z[:, :-1]).all())
    assert bool(((d * 256) == (d * 256).round()).all()) and float(d.min()) >= 0.0 and float(d.max()) < 4.0
    assert bool(((sdf.abs() >= R.SDF_MIN) | (sdf == 0)).all())
    np.testing.assert_allclose(c["raw"][..., 5:].sum(-1).numpy(), 1.0, rtol=1e-6)
    cfg = c["cfg"]
    assert cfg["training"]["trunc"] * cfg["data"]["sc_factor"] == 0.125 and cfg["cam"]["depth_trunc"] == 3.0
    if N >= 7:
        assert bool((d == 0).any()), "a ray without depth"
    if N >= 15:
        assert bool((d >= 3.0).any()), "a depth that is positive but not valid"


def _same_decisions(c):
    a, b = R.decisions(c, torch.float32), R.decisions(c, torch.float64)
    for k in ("first", "any_crossing", "keep", "front", "back", "band", "valid"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["z_cut"].double(), b["z_cut"]), "z_min + band is exact in both formats"
    return b


@pytest.mark.parametrize("key", ALL, ids=R.case_id)
def test_fp32_and_float64_decide_alike_and_counts_are_the_losses_counts(key):
    c = R.case_of(key)
    dec = _same_decisions(c)
    assert torch.equal(c["counts"][:, 0].long(), dec["front"].sum(1)) and torch.equal(c["counts"][:, 1].long(), dec["band"].sum(1))
    # what sdf_losses itself counts: its two weights are 1 - count / total
    s, p = c["raw"][..., 3].double(), c["raw"][..., 5:].double()
    nf, nb = int(c["counts"][:, 0].sum()), int(c["counts"][:, 1].sum())
    assert nf + nb > 0
    ones_front = dec["front"].double()
    # fs = mse(s * front, front) * (1 - nf / total) with emd off: recover the weight sdf_losses used
    fs, _ = path_cpu.sdf_losses(c["z"].double(), c["target_d"].double(), s, p, 0.125, 5, 0.0)
    mse = float((((s * ones_front) - ones_front) ** 2).mean())
    if mse > 0:
        assert abs(float(fs) / mse - (1.0 - nf / (nf + nb))) < 1e-6
    # the maps' keep mask is what composite applies: a sample that is not kept has weight exactly 0
    w = R.reference(c)["weights"]
    assert bool((w[~dec["keep"]] == 0).all()) and bool((w[dec["keep"]] > 0).all())


@pytest.mark.parametrize("key,mode", EDGE_MODES, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else v)
def test_batches_without_depth_decide_alike(key, mode):
    c = R.with_depths(R.case_of(key), mode)
    dec = _same_decisions(c)
    assert not bool(dec["valid"].any())
    ref = R.reference(c, loss_weights=[1.0, 0.1, 1000.0, 10.0])
    nan = torch.isnan(ref["losses"])
    if mode == "invalid":
        assert int(c["counts"].sum()) > 0 and nan.tolist() == [False, True] + [False] * 6
        assert not bool(torch.isnan(ref["draw"]).any())
    else:
        assert int(c["counts"].sum()) == 0 and nan.tolist() == [False, True, True, True, False, True, True, False]
        assert bool(torch.isnan(ref["draw"][..., 3]).all()) and not bool(torch.isnan(ref["draw"][..., [0, 1, 2, 4, 5, 6, 7, 8, 9]]).any())
    assert bool(torch.isnan(ref["objective"]))


@pytest.mark.parametrize("key", ALL, ids=R.case_id)
def test_planted_rays_are_there(key):
    """every rule that fits (N, S) is planted and does what it is for; a tie count of zero is a failure"""
    N, S = key[:2]
    c = R.case_of(key)
    dec = R.decisions(c, torch.float64)
    sdf, z, d = c["raw"][..., 3], c["z"], c["target_d"][:, 0]
    need = [("all_positive", 1), ("all_negative", 1), ("last_pair", 2), ("lane_edge_63", 65), ("lane_edge_127", 129),
            ("lane_edge_191", 193), ("zero_sdf", 6), ("z_cut_tie", 2), ("band_ties", 2), ("saturated", 1), ("nothing_in_front", 1),
            ("no_depth_near", 1)]
    expect = [name for name, min_s in need if S >= min_s][:N]
    assert list(c["planted"]) == expect and list(c["planted"].values()) == list(range(len(expect)))
    P = c["planted"]
    if "all_positive" in P:
        r = P["all_positive"]
        assert bool((sdf[r] > 0).all()) and not dec["any_crossing"][r] and dec["first"][r] == 0
    if "all_negative" in P:
        r = P["all_negative"]
        assert bool((sdf[r] < 0).all()) and not dec["any_crossing"][r] and dec["first"][r] == 0
    if "last_pair" in P:
        r = P["last_pair"]
        assert dec["first"][r] == S - 2 and int(((sdf[r, 1:] * sdf[r, :-1]) < 0).sum()) == 1
    for edge in (63, 127, 191):
        if f"lane_edge_{edge}" in P:
            assert dec["first"][P[f"lane_edge_{edge}"]] == edge
    if "zero_sdf" in P:
        r = P["zero_sdf"]
        k = int(dec["first"][r])
        zeros = (sdf[r] == 0).nonzero().flatten().tolist()
        assert zeros == [1, 3] and k > 3, "the zeros lie before the first true crossing"
        assert not bool(torch.signbit(sdf[r, 1])) and bool(torch.signbit(sdf[r, 3])), "one +0.0 and one -0.0"
        assert float(sdf[r, 0]) > 0 > float(sdf[r, 2]) and float(sdf[r, 4]) > 0, "the sign changes through the zeros"
    if "z_cut_tie" in P:
        r = P["z_cut_tie"]
        tie = (z[r].double() == dec["z_cut"][r]) & (torch.arange(S) > dec["first"][r])
        assert int(tie.sum()) == 1 and not bool(dec["keep"][r][tie].any()), "a sample with z == z_cut, and it is not kept"
    if "band_ties" in P:
        r = P["band_ties"]
        lo, hi = z[r] == d[r] - 0.125, z[r] == d[r] + 0.125
        assert int(lo.sum()) == 1 and int(hi.sum()) == 1 and d[r] > 0
        assert bool(dec["band"][r][lo | hi].all()) and not bool((dec["front"][r] | dec["back"][r])[lo | hi].any())
    if "saturated" in P:
        r = P["saturated"]
        assert bool((sdf[r].abs() == 8).all())
        w32, w64 = R.reference_dtype(c, torch.float32)["weights"][r], R.reference(c)["weights"][r]
        assert bool((w32 == 0).all()) and bool((w64[dec["keep"][r]] > 0).all()) and float(w64.max()) < R.FLT_MIN
    if "nothing_in_front" in P:
        r = P["nothing_in_front"]
        assert 0 < float(d[r]) < 0.25 - 0.125 and int(c["counts"][r, 0]) == 0 and int(c["counts"][r, 1]) == 0
        assert bool(dec["back"][r].all())
    if "no_depth_near" in P:
        r = P["no_depth_near"]
        open_ = ~dec["front"][r] & ~dec["back"][r]
        assert float(d[r]) == 0 and int(open_.sum()) >= 1, "without depth, and samples that only d > 0 keeps out of the band"
        assert bool((z[r][open_] <= 0.125).all()) and bool((z[r] == 0.125).any()) and not bool(dec["band"][r].any())
        assert int(c["counts"][r].sum()) == 0
        others = (d == 0) & (torch.arange(N) != r)
        assert bool(dec["back"][others].all()), "every other ray without depth has all its samples behind d + T"


@pytest.mark.parametrize("tag,emd", [("emd", 0.01), ("noemd", 0.0)])
def test_float64_loss_gradients_are_the_recorded_ones(tag, emd):
    """the anchor: path_cpu.sdf_losses in float64 with autograd against the reference's recorded gradients, at the gate of
    tests/test_oracle_golden.py (rtol 1e-5 with atol 1e-9 there; here 1e-5 of each array's maximum)"""
    g = load_golden("losses.npz")
    T = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
    s, p = T(g["sdf"]).requires_grad_(True), T(g["prob"]).requires_grad_(True)
    fs, sd = path_cpu.sdf_losses(T(g["z_vals"]), T(g["target_d"]), s, p, float(g["truncation"]), 5, emd)
    # (the recorded values are the reference's fp32 results: the same 1e-5 for the two losses)
    assert R.value_error(fs, g[f"{tag}_fs"]) <= 1e-5 and R.value_error(sd, g[f"{tag}_sdf"]) <= 1e-5
    (3.0 * fs + 7.0 * sd).backward()
    assert R.value_error(s.grad, g[f"{tag}_dsdf"]) <= 1e-5
    if emd > 0:
        assert R.value_error(p.grad, g[f"{tag}_dprob"]) <= 1e-5


LW = [1.0, 0.1, 1000.0, 10.0]


@pytest.mark.parametrize("key", ALL, ids=R.case_id)
def test_yardstick_fp32_oracle_against_float64(key, capsys):
    """prints e32 per group (a figure, the GPU file's gates are built from it); asserts only that it is under the project's hard
    ceilings, without which the working gate could not be met by any fp32 code"""
    c = R.case_of(key)
    r64, r32 = R.reference(c, loss_weights=LW), R.reference_dtype(c, torch.float32, loss_weights=LW)
    sat = c["planted"].get("saturated")
    line = [R.case_id(key)]
    for k in R.MAP_NAMES:
        a, b = r32[k].clone(), r64[k].clone()
        if k == "disp_map" and sat is not None:
            assert bool(torch.isnan(a[sat])), "fp32: every weight of the saturated ray underflows, disp = 1 / max(1e-10, 0 / 0)"
            a[sat] = b[sat]
        e = R.value_error(a, b)
        assert e <= R.CEIL_VALUE, k
        line.append(f"{k} {e:.1e}")
    e = max(R.value_error(r32["losses"][j], r64["losses"][j]) for j in range(8))
    assert e <= R.CEIL_VALUE
    line.append(f"losses {e:.1e}")
    for name, errs in R.group_errors(r32["draw"], r64["draw"], R.DRAW_GROUPS).items():
        assert float(errs.max()) <= R.CEIL_GRAD, name
        line.append(f"draw.{name} {errs.max():.1e}")
    with capsys.disabled():
        print("\n  e32 " + "  ".join(line), end="")


@pytest.mark.parametrize("use_bound", [True, False])
def test_rays_bwd_reference_is_the_chain_rule(use_bound):
    c = R.make_case(3, 5, 1, emd_w=0.0, rgb_missing=0, use_bound=use_bound)
    cfg = c["cfg"]
    assert cfg["grid"]["use_bound_normalize"] == use_bound
    dxn = torch.randn(15, 3)
    d_o, d_d = R.rays_bwd_reference(dxn, c["z"], cfg)
    b = np.array(cfg["mapping"]["bound"], dtype=np.float64)
    div = (b[:, 1] - b[:, 0]) if use_bound else 2 * np.array(cfg["mapping"]["localMLP_max_len"], dtype=np.float64)
    gp = dxn.double().numpy().reshape(3, 5, 3) / div / cfg["training"]["norm_factor"]
    np.testing.assert_allclose(d_o.numpy(), gp.sum(1), rtol=1e-13)
    np.testing.assert_allclose(d_d.numpy(), (gp * c["z"].double().numpy()[..., None]).sum(1), rtol=1e-13)
