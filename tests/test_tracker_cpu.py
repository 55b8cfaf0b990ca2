"""CPU: holds tests/tracker_cpu.py -- the inputs, the float64 answers and the derived bounds that tests/test_gpu_tracker_fp64.py
compares the particle, fitness and update kernels of the particle-swarm pre-tracker with -- to its conditions, on EVERY case with
nothing left out: the fp32 yardstick (the kernels' arithmetic in numpy fp32) lies within the bound on every word; the yardstick and
the float64 answer advance the same particles and take the same side of s <= 1; no bound is vacuous (below 1e-5 of the word's scale,
1e-2 on the ill-conditioned case, where it must have GROWN with the cancellation); every listed P and n occurs; every planted
particle lands in the branch it was planted for; no intermediate of the update's yardstick is subnormal.  The float64 path through
oracle/ro_cpu.py is held to the reference's own tensors (tests/golden/ro.npz) at the tolerances tests/test_oracle_golden.py uses for
the fp32 path.  Last, each of six one-line faults of the kernels, planted in the yardstick, breaks a bound: the bounds can see them."""
import math

import numpy as np
import pytest
import torch

from mipsfusion_amd import synth

from . import tracker_cpu as T
from .conftest import load_golden
from .test_oracle_golden import close, scene_from


def exceed(y, ans, bound):
    """the largest |y - ans| / bound over the words (0 / 0 is 0: a word held bit for bit that is equal)"""
    err = np.abs(np.asarray(y, dtype=np.float64) - np.asarray(ans, dtype=np.float64))
    assert not np.isnan(err).any() and not np.isnan(bound).any()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def particle_args(c):
    return c["pst"], c["state"], c["rays"], c["td"], c["cfg"]


def update_args(c):
    return c["mm"], c["pst7"], c["state"], c["rescale"]


# ------------------------------------------------------------------------------------------------------- coverage
def test_cases_cover_what_the_gpu_file_promises():
    pc, fc, uc = T.PARTICLE_CASES, T.FITNESS_CASES, T.UPDATE_CASES
    for cases in (pc, fc):
        assert {c[1] for c in cases} == {1, 3, 4, 5, 37} and {c[2] for c in cases} == {1, 63, 64, 65, 129}
    assert {(c[3], c[4]) for c in pc} == {(0, True), (0, False), (1, True), (1, False)}, "both orders with both normalisations"
    assert {c[5] for c in pc if c[4]} == {1.0, 2.0} and {c[5] for c in pc if not c[4]} == {1.0, 2.0}
    assert {c[6] for c in pc} == {"small", "wide"}
    assert {c[3] for c in fc} == {"raw10", "sdf-row", "sdf-point"} and any(c[4] for c in fc)
    assert {c[1] for c in uc} == {1, 2, 255, 256, 257, 1000}
    assert {c[2] for c in uc} == {"lattice-none", "lattice-ties", "lattice-tail", "generic", "ill"}
    assert {c[1] for c in uc if c[2] == "lattice-tail"} == {257, 1000}
    assert len({c[0] for c in pc + fc + uc}) == len(pc + fc + uc)
    for k in range(6):
        assert len({float(T.SEARCH_SMALL[k]), float(T.SEARCH_WIDE[k])}) == 2
    assert len(set(T.SEARCH_SMALL.tolist())) == 6 and len(set(T.SEARCH_WIDE.tolist())) >= 5, "the search size differs per component"
    assert abs(np.linalg.norm(T.PLANE_N) - 1.0) < 1e-15


# ------------------------------------------------------------------------------------------------------ particles
@pytest.mark.parametrize("key", T.PARTICLE_CASES, ids=T.case_id)
def test_particle_case(key):
    c = T.particle_case(key)
    P, n, st = c["P"], c["n"], c["state"]
    assert c["pst"].dtype == c["rays"].dtype == c["td"].dtype == st.dtype == np.float32
    assert not c["pst"][0].any(), "row 0 of the template is zero"
    R = st[T.ROT:T.ROT + 9].astype(np.float64).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R).max() < 0.999 and np.abs(R).min() > 1e-3, "a generic rotation"
    if n >= 23:
        assert (c["td"] == 0).sum() >= 2 and np.signbit(c["td"][c["td"] == 0]).any() and (c["td"] < 0).any(), "0.0, -0.0 and a negative depth"
    pst7a, xna, *_ = T.particle_answer(*particle_args(c))
    pst7a, xna = pst7a.numpy(), xna.numpy()
    assert pst7a.dtype == xna.dtype == np.float64 and xna.shape == (P, n, 3)
    b7, bx = T.particle_bound(*particle_args(c))
    y7, yx, inside32 = T.particles(T.F, *particle_args(c))
    _, _, inside64 = T.particles(T.E, *particle_args(c))
    # both formats take the same side of s <= 1, on every particle
    s64 = (pst7a[:, 1:4] ** 2).sum(1)
    assert np.array_equal(inside32, inside64) and np.array_equal(inside64, s64 <= 1.0)
    assert np.array_equal(pst7a[:, 0] == 0, ~(s64 < 1.0)), "qw == 0 exactly where s >= 1"
    # the restatement in float64 is the oracle's answer (E.v) to float64's own accuracy
    e7, ex, _ = T.particles(T.E, *particle_args(c))
    assert np.abs(e7.v - pst7a).max() < 1e-14 and np.abs(ex.v - xna).max() < 1e-13
    # the planted particles
    pl, r = c["planted"], pst7a
    assert pl["identity"] == 0 and r[0].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert (b7[0] == 0).all() and (y7.v[0] == r[0]).all(), "the identity particle is exact"
    if "wide" in key[0]:
        assert list(pl) == [name for name, _ in T.PLANTED[:P]]
        random_rows = np.arange(P) >= len(pl)
        assert (s64[random_rows] <= 0.5).all(), "random particles have s <= 1/2"
        if "s_is_1" in pl:
            assert s64[pl["s_is_1"]] == 1.0 and r[pl["s_is_1"], 0] == 0.0 and inside32[pl["s_is_1"]] and y7.v[pl["s_is_1"], 0] == 0.0
            assert b7[pl["s_is_1"], 0] == 0, "s == 1 exactly in both formats: qw == 0 is held bit for bit"
        if "s_above_1" in pl:
            assert s64[pl["s_above_1"]] == 1.25 and not inside32[pl["s_above_1"]] and r[pl["s_above_1"], 0] == 0.0
        if "s_is_0" in pl:
            assert s64[pl["s_is_0"]] == 0.0 and r[pl["s_is_0"], 0] == 1.0 and r[pl["s_is_0"], 4:].all() and b7[pl["s_is_0"], 0] == 0
    else:
        assert (s64 <= 0.5).all() and (s64[1:] > 0).all()
    # the words held bit for bit, the yardstick under the bound, no bound vacuous
    assert np.array_equal(y7.v[:, 1:], (c["pst"].astype(np.float64) * st[T.SEARCH:T.SEARCH + 6].astype(np.float64)).astype(np.float32))
    assert exceed(y7.v, pst7a, b7) <= 1.0 and exceed(yx.v, xna, bx) <= 1.0
    assert b7[:, 0].max() < 1e-5 and bx.max() < 1e-5 * np.abs(xna).max(), (b7[:, 0].max(), bx.max())
    assert np.abs(xna).max() < 4.0 and np.abs(xna).max() > 0.05


def test_particle_bound_is_a_small_multiple_of_its_yardstick():
    """U (A / div + |xn|), A = sum_k |aR_k| |c_k| + |t|: the bound stays within 22 of it (the count K of the longest path)"""
    for key in T.PARTICLE_CASES:
        c = T.particle_case(key)
        _, xna, a_rot, a_trans, _ = T.particle_answer(*particle_args(c))
        _, bx = T.particle_bound(*particle_args(c))
        sub, div, nf = T.norm_consts(c["cfg"])
        cam = np.abs(c["rays"].astype(np.float64) * c["td"].astype(np.float64)[:, None])
        A = np.einsum("pkj,nj->pnk", np.abs(a_rot.numpy()), cam) + np.abs(a_trans.numpy())[:, None, :, 0]
        unit = T.U * (A / (div * nf) + np.abs(xna.numpy()))
        assert (bx <= 22 * unit).all(), (key[0], float((bx / unit).max()))


# -------------------------------------------------------------------------------------------------------- fitness
@pytest.mark.parametrize("key", T.FITNESS_CASES, ids=T.case_id)
def test_fitness_case(key):
    c = T.fitness_case(key)
    P, n, sdf, td = c["P"], c["n"], c["sdf"], c["td"]
    assert not np.isnan(sdf).any()
    assert sdf.size < 4 or ((sdf > 0).any() and (sdf < 0).any()), "SDF values of mixed sign"
    ans = T.fitness_answer(sdf, td, c["trunc"]).numpy()
    bound = T.fitness_bound(sdf, td, c["trunc"])
    y = T.fitness(T.F, sdf, td, c["trunc"]).v
    assert ans.shape == y.shape == (P,) and ans.dtype == np.float64
    if c["none_valid"]:
        assert not (td > 0).any() and (td == 0).any() and np.signbit(td[td == 0]).any() and (td < 0).any()
        assert (ans == 0).all() and (bound == 0).all() and (y == 0).all(), "every depth invalid: exactly 0.0"
        return
    if n >= 23:
        assert 0.05 < (td <= 0).mean() < 0.2 and (td == 0).sum() >= 2 and np.signbit(td[td == 0]).any() and (td < 0).any()
    if c["form"] == "raw10":
        assert c["raw"].shape == (P * n, 10) and (np.delete(c["raw"], 3, axis=1) == T.RAW_SENTINEL).all()
        assert np.array_equal(c["raw"][:, 3].reshape(P, n), sdf)
    else:
        assert np.array_equal(T.unordered(c["raw"], P, n, c["form"] == "sdf-point"), sdf)
    assert exceed(y, ans, bound) <= 1.0
    assert (bound < 1e-5 * ans).all() and (ans > 0).all()
    # the count of the issue: (ceil(n / 64) + 6 + product + division) roundings on the sum of the valid |sdf trunc| / n
    total = (np.abs(sdf.astype(np.float64) * c["trunc"]) * (td > 0)[None, :]).sum(1) / n
    assert (bound <= (-(-n // 64) + 8) * T.U * total * (1 + 1e-6) + 2.0 ** -48).all()


# --------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("key", T.UPDATE_CASES, ids=T.case_id)
def test_update_case(key):
    c = T.update_case(key)
    P, kind, mm = c["P"], c["kind"], c["mm"]
    assert mm.dtype == c["pst7"].dtype == np.float32 and (mm > 0).all() and c["pst7"].shape == (P, 7)
    ans = T.update_answer(*update_args(c))
    bound = T.update_bound(*update_args(c))
    T.F.tiny = math.inf
    y, adv32, _, _ = T.update(T.F, *update_args(c))
    assert T.F.tiny >= T.FLT_MIN, f"an intermediate of the yardstick is subnormal: {T.F.tiny!r}"
    _, adv64, _, _ = T.update(T.E, *update_args(c))
    spec = T.advanced_fp32(mm)
    assert np.array_equal(adv32, spec) and np.array_equal(adv64, spec) and not spec[0]
    f64 = mm.astype(np.float64) * 1000.0
    if kind.startswith("lattice"):
        j = mm.astype(np.float64) * 1024
        assert np.array_equal(j, np.round(j)) and j.max() < 16384
        assert np.array_equal((mm * np.float32(1000)).astype(np.float64), f64), "mean_masked * 1000 is exact in fp32"
        assert np.array_equal(spec, f64 < f64[0]), "fp32 and float64 decide alike on every particle"
    ex = c["expect"]
    if kind == "lattice-ties":
        assert ex["ties"] or P == 2
        assert all(f64[r] == f64[0] and not spec[r] for r in ex["ties"]), "an exact tie with particle 0 is not advanced"
        assert ex["below"] and all(spec[r] and mm[r] == np.float32((T.LATTICE_J0 - 1) / 1024) for r in ex["below"])
        assert all(not spec[r] and mm[r] == np.float32((T.LATTICE_J0 + 1) / 1024) for r in ex["above"])
    if kind == "lattice-none":
        assert not spec.any() and (P < 4 or (f64[1:] == f64[0]).sum() >= 2), "nothing advanced, ties among them"
    if kind == "lattice-tail":
        assert list(np.nonzero(spec)[0]) == ex["advanced"] and spec.sum() == P - (P // 256) * 256 and not spec[:(P // 256) * 256].any()
    if kind == "generic":
        assert spec.any() and 0.005 < mm.min() and mm.max() < 0.06
    if kind == "ill":
        rel = (f64[0] - f64[spec]) / f64[0]
        assert spec.sum() > 50 and 2e-5 < rel.min() and rel.max() < 2e-4, "the advanced ones win by about 1e-4 of particle 0's value"
    # the answer's bookkeeping words
    assert ans[T.NBETTER] == spec.sum() and ans[T.SUCCESS] == float(spec.any()) and ans[T.FIT0] == f64[0]
    if not spec.any():
        st = c["state"].astype(np.float64)
        assert np.array_equal(ans[:12], st[:12]) and ans[T.MEAN_T:T.MEAN_T + 7].tolist() == [1, 0, 0, 0, 0, 0, 0] and ans[T.MEAN_SDF] == mm[0]
        sz = np.full(6, T.C_SZ)
        doubled = 2 * (T.RESCALE * float(mm[0]) * sz / np.linalg.norm(sz) + T.C_SZ)
        assert np.abs(ans[T.SEARCH:T.SEARCH + 6] - doubled).max() < 1e-15, "the doubled form of the search size"
    else:
        assert (np.abs(ans[T.MEAN_T + 1:T.MEAN_T + 7]) > 0).all(), "|mean transform| is differentiable where the bound differentiates it"
    # the yardstick under the bound on every word; no bound vacuous
    assert y.v.shape == ans.shape == bound.shape == (T.STATE_USED,)
    assert exceed(y.v, ans, bound) <= 1.0
    assert y.v[T.NBETTER] == spec.sum() and y.v[T.FIT0] == np.float32(mm[0]) * np.float32(1000)
    vac = bound / T.update_scale(ans)
    if kind == "ill":
        assert vac.max() < 1e-2
        assert vac.max() > 1e-4, "the bound has grown with the cancellation (every other case stays below 1e-5)"
    else:
        assert vac.max() < 1e-5, (int(vac.argmax()), float(vac.max()))


# ----------------------------------------------------------------------------------- the float64 path and the reference
def test_float64_answers_match_the_reference_tensors():
    """tests/golden/ro.npz: the reference's own pst7, absolute poses and mean masked SDF of the first round"""
    g = load_golden("ro.npz")
    cfg = synth.config_plumbing()
    rows, cols = g["rows"], g["cols"]
    state = np.zeros(T.STATE_FLOATS, np.float32)
    state[T.ROT:T.ROT + 9], state[T.TRANS:T.TRANS + 3] = g["init_pose"][:3, :3].reshape(9), g["init_pose"][:3, 3]
    state[T.SEARCH:T.SEARCH + 6] = np.float32(g["c1"])
    rays, td = np.ascontiguousarray(g["rays_dir"][rows, cols]), np.ascontiguousarray(g["depth"][rows, cols])
    pst7, xn, a_rot, a_trans, world = T.particle_answer(g["pst"], state, rays, td, cfg)
    assert pst7.dtype == torch.float64
    close(pst7, g["pst7_0"], rtol=0, atol=1.2e-7)
    close(a_rot, g["abs_rot0"], rtol=1e-6, atol=1e-7)
    close(a_trans, g["abs_trans0"], rtol=1e-6, atol=1e-7)
    m = scene_from(g, cfg)
    m.eval()
    with torch.no_grad():
        raw = m.run_network(world.to(torch.float32))
    mms = T.fitness_answer(raw[..., 3].numpy(), td, float(g["trunc"]))
    close(mms, g["mean_masked0"], rtol=2e-5, atol=1e-7)
    # and the restatement's normalisation is run_network's: bound normalisation of the plumbing config
    b = torch.from_numpy(g["bound"])
    close(xn, (world - b[:, 0]) / (b[:, 1] - b[:, 0]), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------ the bounds see the faults
def test_a_wrong_rotation_addend_breaks_the_xn_bound():
    """aR[5] used for aR[2] in the transform"""
    for key in T.PARTICLE_CASES:
        c = T.particle_case(key)
        xna = T.particle_answer(*particle_args(c))[1].numpy()
        _, yx, _ = T.particles(T.F, *particle_args(c), mutation="aR5_for_aR2")
        assert exceed(yx.v, xna, T.particle_bound(*particle_args(c))[1]) > 1e3, key[0]


def test_the_wrong_sign_of_the_half_length_breaks_the_xn_bound():
    """sub of the use_bound = False form taken as +L"""
    hit = 0
    for key in T.PARTICLE_CASES:
        c = T.particle_case(key)
        if c["cfg"]["grid"]["use_bound_normalize"]:
            continue
        xna = T.particle_answer(*particle_args(c))[1].numpy()
        _, yx, _ = T.particles(T.F, *particle_args(c), mutation="sub_plus_L")
        assert exceed(yx.v, xna, T.particle_bound(*particle_args(c))[1]) > 1e3, key[0]
        hit += 1
    assert hit >= 2


def test_a_transposed_sample_index_breaks_the_order_contract():
    """i * P + p against p * n + i in one kernel only: the fitness reads another particle's points (P = 5, n = 65)"""
    P, n = 5, 65
    c = T.fitness_case(next(k for k in T.FITNESS_CASES if k[1] == P and k[2] == n and not k[4]))
    ans, bound = T.fitness_answer(c["sdf"], c["td"], c["trunc"]).numpy(), T.fitness_bound(c["sdf"], c["td"], c["trunc"])
    for pm in (False, True):
        misread = T.unordered(T.ordered(c["sdf"], pm), P, n, not pm)
        assert exceed(T.fitness(T.F, misread, c["td"], c["trunc"]).v, ans, bound) > 1e3
        same = T.unordered(T.ordered(c["sdf"], pm), P, n, pm)
        assert exceed(T.fitness(T.F, same, c["td"], c["trunc"]).v, ans, bound) <= 1.0


@pytest.mark.parametrize("mutation", ["loop_P_and_not_255", "le_for_lt", "no_double"])
def test_update_faults_break_a_bound_or_a_count(mutation):
    """the loop bound P & ~255 (the last partial stride dropped), f <= f0 for f < f0, the failed round's * 2.0f dropped"""
    caught = []
    for key in T.UPDATE_CASES:
        c = T.update_case(key)
        ans, bound = T.update_answer(*update_args(c)), T.update_bound(*update_args(c))
        with np.errstate(all="ignore"):
            y, _, _, _ = T.update(T.F, *update_args(c), mutation=mutation)
        bad = np.isnan(y.v).any() or y.v[T.NBETTER] != ans[T.NBETTER] or exceed(np.nan_to_num(y.v), ans, bound) > 1.0
        if bad:
            caught.append(key[0])
    want = {"loop_P_and_not_255": {"P257-lattice-tail", "P1000-lattice-tail", "P255-generic", "P2-lattice-ties"},
            "le_for_lt": {"P255-lattice-ties", "P257-lattice-ties", "P257-lattice-none"},
            "no_double": {"P1-lattice-none", "P257-lattice-none"}}[mutation]
    assert want <= set(caught), (mutation, caught)
