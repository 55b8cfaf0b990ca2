"""CPU: tests/chain_cpu.py held to its conditions -- its links agree with the unit restatements on its own intermediates, every case
is built within the candidate cap with every margin kept, the fp32 yardstick decides as the chain does and has headroom under the
ceilings, and every planted seam defect (chain_cpu.MUTATIONS) moves some compared group by ten working gates on some case.
tests/test_gpu_chain_fp64.py then holds the kernels to the chain."""
import warnings

import numpy as np
import pytest
import torch

from mipsfusion_amd import ops
from oracle import path_cpu

from . import chain_cpu as C
from . import decoder_cpu, hashgrid_cpu, render_cpu, step_cpu

LINK = 1e-12

# case -> (tiles, tiles holding samples of two rays, M mod 32): what chain_cpu.SPECS' shapes are there for
TILES = {"N1-S16": (1, 0, 16), "N5-S33": (6, 4, 5), "N17-S64": (34, 0, 0), "N17-S75": (40, 16, 27), "N33-S64": (66, 0, 0),
         "N16-S129": (65, 15, 16), "N8-S64-fixed": (16, 0, 0), "N17-S64-nodepth": (34, 0, 0)}


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (the mean of an empty selection: the batch without a valid depth)
        yield


def close(a, b, what, tol=LINK):
    a, b = C._np64(a), C._np64(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    scale = max(float(np.nanmax(np.abs(b))) if b.size else 0.0, 1e-300)
    err = float(np.nanmax(np.abs(a - b))) / scale if b.size and not np.isnan(b).all() else 0.0
    assert err <= tol, f"{what}: {err:.3e} of scale"


# ----------------------------------------------------------------------------------------------------------------- link agreement
@pytest.mark.parametrize("name", C.CASES)
def test_grid_link_is_the_unit_restatement(name):
    case, a = C.build_case(name), C.answer(name)
    M = case["N"] * case["S"]
    R = hashgrid_cpu.reference(case["levels"], a["xn"].numpy(), case["params"], a["dfeat"].numpy().reshape(M, 16, 2))
    close(a["fw"]["dec"]["feat"], R["y"].reshape(M, 32), "features")
    assert np.array_equal(a["entries"], R["entries"])
    close(a["dp"], R["dp"], "table gradient")
    close(a["dxn"] - a["back"]["dx"], R["dx"], "the grid's part of d xn")
    assert R["fma"][1] == 0 and a["fw"]["grid"]["modes"] >= {0, 1}, "dense and hashed levels both occur, no unresolved fma"


@pytest.mark.parametrize("name", C.CASES)
def test_decoder_link_is_the_unit_restatement_and_autograd(name):
    case, a = C.build_case(name), C.answer(name)
    feat, x = a["fw"]["dec"]["feat"], a["xn"]
    r = decoder_cpu.evaluate(case["weights"], feat, x, a["draw"], torch.float64)
    close(a["raw"].reshape(-1, 10), r["out"], "raw")
    close(a["dfeat"], r["dfeat"], "d feat")
    close(a["back"]["dx"], r["dx"], "d x of the decoder")
    for k, g, h in zip(ops.DECODER_PARAM_ORDER, a["grads"], r["grads"]):
        close(g, h, k)
    # autograd through the oracle's own decoder, the encoding and the features as leaves
    w = {k: t.double().requires_grad_(True) for k, t in zip(ops.DECODER_PARAM_ORDER, case["weights"])}
    fl = feat.clone().requires_grad_(True)
    pe = decoder_cpu.encoding(x, torch.float64)[0]
    out = path_cpu.decoder_forward(w, fl, pe, x.double())
    close(a["raw"].reshape(-1, 10), out, "raw (path_cpu.decoder_forward)")
    g = torch.autograd.grad((out * a["draw"]).sum(), [fl] + [w[k] for k in ops.DECODER_PARAM_ORDER])
    close(a["dfeat"], g[0], "d feat (autograd)")
    for k, mine, theirs in zip(ops.DECODER_PARAM_ORDER, a["grads"], g[1:]):
        close(mine, theirs, k + " (autograd)")


@pytest.mark.parametrize("name", C.CASES)
def test_render_link_is_the_unit_restatement(name):
    case, a = C.build_case(name), C.answer(name)
    rays, tr = C.rays_of(case), case["cfg"]["training"]
    unit = dict(raw=a["raw"], z=a["z_vals"], target_rgb=rays[:, 3:6], target_d=rays[:, 6:7], counts=a["counts"], cfg=case["cfg"],
                emd_w=case["emd_w"])
    r = render_cpu.reference_dtype(unit, torch.float64, loss_weights=torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"]],
                                                                                  dtype=torch.float64))
    close(a["rgb"], r["rgb"], "rgb")
    close(a["depth"], r["depth"], "depth")
    close(a["losses"], r["losses"], "losses")
    close(a["total"], r["objective"], "objective")
    close(a["draw"], r["draw"].reshape(-1, 10), "d raw")
    assert torch.equal(a["counts"], step_counts(case, a)), "counts by the placement kernel's rule on the fp32 z_vals"


def step_counts(case, a):
    T = case["cfg"]["training"]["trunc"] * case["cfg"]["data"]["sc_factor"]
    front, _, band = C.masks(a["z_vals"], C.rays_of(case)[:, 6:7], T, torch.float32)
    return torch.stack([front.sum(1), band.sum(1)], 1).to(torch.int32)


@pytest.mark.parametrize("name", C.CASES)
def test_pose_and_ray_gradients_are_autograd_through_the_composition(name):
    case, a = C.build_case(name), C.answer(name)
    rays, S = C.rays_of(case), case["S"]
    rot = case["rot"].double().clone().requires_grad_(True)
    trans = case["trans"].double().clone().requires_grad_(True)
    ro, rd = step_cpu.pose_rays(rot, trans, case["fixed"].double(), case["owner"], rays[:, :3].double())
    xn = C.normalise(path_cpu.ray_points(ro, rd, a["z_vals"].double()).double(), case["cfg"])
    close(xn.detach().float(), a["xn"], "xn", 0.0)
    g_o, g_d = torch.autograd.grad((xn * a["dxn"]).sum(), (ro, rd), retain_graph=True)
    close(a["d_rays_o"], g_o, "d rays_o")
    close(a["d_rays_d"], g_d, "d rays_d")
    masked = a["dxn"] * a["wants_dx"].repeat_interleave(S)[:, None].double()
    if bool(a["wants_dx"].any()):
        g_r, g_t = torch.autograd.grad((xn * masked).sum(), (rot, trans), retain_graph=True)
    else:
        g_r, g_t = torch.zeros_like(rot), torch.zeros_like(trans)
    close(a["d_rot"], g_r, "d rot")
    close(a["d_trans"], g_t, "d trans")
    # the rays of the fixed poses reach no pose: masking them changes nothing
    if bool(a["wants_dx"].any()):
        g_r2, g_t2 = torch.autograd.grad((xn * a["dxn"]).sum(), (rot, trans))
        close(g_r, g_r2, "d rot, unmasked"), close(g_t, g_t2, "d trans, unmasked")
    K, Fn = case["spec"]["K"], case["spec"]["F"]
    for k in range(K):
        if not bool(((case["owner"] % (Fn + K)) == Fn + k).any()):
            assert not bool(a["d_rot"][k].any()) and not bool(a["d_trans"][k].any()), "a pose without a ray: exactly 0.0"


# ------------------------------------------------------------------------------------------------------------ builder conditions
@pytest.mark.parametrize("name", C.CASES)
def test_case_is_built_within_the_conditions(name):
    case, a = C.build_case(name), C.answer(name)
    N, S, spec = case["N"], case["S"], case["spec"]
    assert int(case["tried"].max()) <= C.CAP
    print(f"\n  chain | {name} | accepted {case['share']:.0%} of {int(case['tried'].sum())} candidates, at most {int(case['tried'].max())} for a ray",
          end="")
    m = C.margins(case, a["fw"])
    for k in ("relu", "crossing", "compare", "cell"):
        assert bool((m[k] >= 1.0).all()), f"{k} margin of ray {int(m[k].argmin())}: {float(m[k].min()):.3f} of what is asked"
    assert C.tile_facts(N, S) == TILES[name]
    assert (spec["nu"], spec["nn"]) == (case["cfg"]["training"]["n_samples_d"], case["cfg"]["training"]["n_range_d"])
    # planted rays and what the case is there for
    d = C.rays_of(case)[:, 6]
    valid = (d > 0) & (d < case["cfg"]["cam"]["depth_trunc"])
    for slot, kind in spec.get("planted", {}).items():
        if kind in ("no_depth", "no_depth_negative"):
            assert float(d[slot]) <= 0.0
        elif kind == "beyond_trunc":
            assert float(d[slot]) >= case["cfg"]["cam"]["depth_trunc"]
        elif kind == "no_crossing":
            assert not bool(m["any_crossing"][slot])
    if spec.get("depth") == "none":
        assert not bool(valid.any()) and bool((d <= 0).any()) and bool((d > 0).any()) and bool(torch.isnan(a["losses"][1]))
        assert not bool(torch.isnan(a["losses"][[0, 2, 3]]).any())
    else:
        assert bool(valid.any()) and bool(m["any_crossing"].any()) and bool(torch.isfinite(a["losses"]).all())
        assert N < 3 or bool((d >= case["cfg"]["cam"]["depth_trunc"]).any()), "depth_trunc is low enough that rays lie beyond it"
    own = case["owner"] % (spec["F"] + spec["K"])
    pattern = spec["owner"]
    if pattern == "all_fixed":
        assert not bool(a["wants_dx"].any()) and not bool(a["d_rot"].any()) and a["dp"].any() and all(bool(g.any()) for g in a["grads"])
    if pattern == "two_of_three":
        assert spec["F"] == 0 and not bool((own == 2).any()) and bool(a["d_rot"][:2].any())
    if pattern == "alternate":
        assert bool((a["wants_dx"][1:] != a["wants_dx"][:-1]).all())
    if pattern == "last_fixed":
        assert a["wants_dx"].tolist() == [True] * (N - 1) + [False]
    if pattern == "one_optimised":
        assert spec["K"] == 1 and 0 < int(a["wants_dx"].sum()) < N and S > ops.RENDER_DRAW_MAX_S
    assert bool(case["cfg"]["grid"]["use_bound_normalize"]) == spec["bound"]
    # the points leave the unit box (the negative-cell wrap of the grid is part of the chain)
    assert name == "N1-S16" or float(a["xn"].min()) < 0.0 or float(a["xn"].max()) > 1.0 or not spec["bound"]


@pytest.mark.parametrize("name", C.CASES)
def test_yardstick_decides_as_the_chain_does(name):
    case, a, y = C.build_case(name), C.answer(name), C.yardstick(name)
    assert torch.equal(y["z_vals"], a["z_vals"]) and torch.equal(y["counts"], a["counts"])
    # its points within a quarter of the cell margin of the chain's
    sc = torch.from_numpy(case["levels"].scales.astype(np.float64))
    dist = float(((y["xn"].double() - a["xn"].double()).abs()[:, None, :] * sc[None, :, None] / (sc[None, :, None] + 1.0)).max())
    print(f"\n  chain | {name} | yardstick xn within 2^{np.log2(max(dist, 1e-300)):.2f} (scale + 1) of the chain's in pos; "
          f"margin 2^{np.log2(C.CELL_MARGIN):.0f}", end="")
    assert dist <= C.CELL_MARGIN / 4
    for level in range(16):
        c, _, _ = hashgrid_cpu.locate(case["levels"], y["xn"].numpy(), level)
        assert np.array_equal(c, a["fw"]["grid"]["c"][:, level]), f"grid cell, level {level}"
    dec = a["fw"]["dec"]
    assert torch.equal(y["pre"]["H1"] > 0, dec["H1"] > 0) and torch.equal(y["pre"]["G3"] > 0, dec["G3"] > 0), "ReLU"
    rays = C.rays_of(case)
    d64 = render_cpu.decisions(dict(raw=a["raw"], z=a["z_vals"], target_d=rays[:, 6:7], cfg=case["cfg"]), torch.float64)
    d32 = render_cpu.decisions(dict(raw=y["raw"], z=y["z_vals"], target_d=rays[:, 6:7], cfg=case["cfg"]), torch.float32)
    for k in ("first", "any_crossing", "keep", "front", "back", "band", "valid"):
        assert torch.equal(d64[k], d32[k]), k


def test_the_issue_cell_margin_is_widened_by_its_own_rule():
    """2^-20 is what the issue starts from; its rule widens the margin to four times what the yardstick shows"""
    worst = 0.0
    for name in C.CASES:
        case, a, y = C.build_case(name), C.answer(name), C.yardstick(name)
        sc = torch.from_numpy(case["levels"].scales.astype(np.float64))
        worst = max(worst, float(((y["xn"].double() - a["xn"].double()).abs()[:, None, :] * sc[None, :, None] / (sc[None, :, None] + 1.0)).max()))
    assert worst > C.CELL_MARGIN_ISSUE / 4, "the yardstick is within a quarter of 2^-20: the widening is not needed any more"
    assert 4 * worst <= C.CELL_MARGIN < 8 * worst, "four times the yardstick's distance, rounded up to a power of two"


# ------------------------------------------------------------------------------------------------------------------- headroom
@pytest.mark.parametrize("name", C.CASES)
def test_yardstick_has_headroom(name):
    e = C.e32(name)
    worst = max(e, key=lambda k: e[k] / C.ceiling(k))
    print(f"\n  chain | {name} | worst e32 {e[worst]:.2e} ({worst}, ceiling {C.ceiling(worst):.0e})", end="")
    for k, v in e.items():
        assert v < C.ceiling(k) / 4, f"{k}: e32 {v:.3e} leaves less than a quarter of the ceiling {C.ceiling(k):.0e}"


# ----------------------------------------------------------------------------------------------------------------- sensitivity
def as_result(m, case):
    res = {k: m[k] for k in ("rgb", "depth", "losses", "grads", "d_rot", "d_trans", "d_rays_o", "d_rays_d")}
    res["table"] = C.table_grad(m, case["levels"])[0]
    return res


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_every_mutation_is_seen(mutation):
    best = (0.0, None, None)
    for name in C.CASES:
        case, a = C.build_case(name), C.answer(name)
        m = C.chain(case, mutation)
        err = C.errors(as_result(m, case), a, case["levels"])
        for group, (v, _) in err.items():
            factor = v / C.gate(group, C.e32(name)[group])
            if factor > best[0]:
                best = (factor, name, group)
        if mutation == "counts_swapped" and name != "N17-S64-nodepth":
            assert not torch.equal(m["counts"], a["counts"])
    print(f"\n  chain | mutation {mutation} | seen by {best[1]}, group {best[2]}: {best[0]:.3g} working gates", end="")
    assert best[0] >= 10.0, f"{mutation}: no case moves a group by ten working gates (best {best})"
