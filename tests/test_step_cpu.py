"""CPU: holds tests/step_cpu.py -- the inputs and the independent answers that tests/test_gpu_step_fp64.py compares the placement,
pose, frequency, normalisation and Adam kernels with -- to its conditions: fp32 and float64 decide front / back / band alike on
EVERY sample of every placement case, the planted ties and edges are really there (a missing one FAILS), the owner layouts hold the
waves they promise, every fp32 yardstick lies inside its own ceiling, an fp32 restatement of the pose backward in another summation
order meets the working gate, and the derived Adam bound holds an fp32 restatement of adam1 and rejects two mutated ones."""
import numpy as np
import pytest
import torch

from oracle import tcnn_cpu

from . import step_cpu as P


# ------------------------------------------------------------------------------------------------------ placement
def test_placement_cases_cover_what_the_gpu_file_promises():
    depth = [c for c in P.PLACE_CASES if c[7] == "depth"]
    assert {c[1] + c[2] for c in depth} >= {1, 2, 63, 64, 65, 128, 129, 255, 256}
    pairs = {(c[1], c[2]) for c in depth}
    assert (0, 1) in pairs and (1, 0) in pairs and any(nn > nu > 0 for nu, nn in pairs)
    assert {c[3] for c in P.PLACE_CASES} == {1, 3, 4, 5, 33}
    assert {c[3] for c in depth if (c[1], c[2]) == (43, 21)} == {1, 3, 4, 5, 33}
    assert any(c[7] == "none" for c in P.PLACE_CASES) and any(c[1] == 0 and c[2] > 0 for c in depth)
    for flag in (0, 1):
        assert {c[5] for c in P.PLACE_CASES if c[4] == flag} == {True, False}, "both normalisations with and without jitter"
    assert any(c[6] == 2.0 and c[5] for c in P.PLACE_CASES) and any(c[6] == 2.0 and not c[5] for c in P.PLACE_CASES)


@pytest.mark.parametrize("key", P.PLACE_CASES, ids=P.place_id)
def test_placement_inputs_and_decisions(key):
    c = P.place_case(key)
    cfg, N, S = c["cfg"], c["N"], c["S"]
    z = P.place_z(c)
    assert z.dtype == torch.float32 and z.shape == (N, S)
    assert cfg["training"]["trunc"] * cfg["data"]["sc_factor"] == 0.125 and cfg["cam"]["near"] == 0 and cfg["cam"]["far"] == 4
    assert bool((z[:, 1:] >= z[:, :-1]).all()), "sorted (the depth-guided list alone is sorted by construction)"
    if c["noise"] is not None:
        assert bool((c["noise"] == 0).any()) and bool((c["noise"] == P.ONE_BELOW).any()) and float(c["noise"].max()) < 1.0
    if c["target_d"] is None:
        assert c["n_near"] == 0 and c["tables"][1] is None
        return
    d = c["target_d"]
    assert bool(((d * 16) == (d * 16).round()).all()), "depths on the lattice of 1/16"
    # d - T and d + T are exact in fp32, so fp32 and float64 decide alike on EVERY sample -- none is left out
    a, b = P.masks(z, d, torch.float32), P.masks(z, d, torch.float64)
    for x, y, name in zip(a, b, ("front", "back", "band")):
        assert torch.equal(x, y), name
    assert torch.equal((d - 0.125).double(), d.double() - 0.125) and torch.equal((d + 0.125).double(), d.double() + 0.125)
    counts = P.place_counts(z, d)
    assert torch.equal(counts[:, 0].long(), b[0].sum(1)) and torch.equal(counts[:, 1].long(), b[2].sum(1))
    assert bool((c["rows"] < 0).any()) or N == 1
    assert torch.equal(c["table"][c["rows"], 6:7], d), "the table rows hold the rays' depths (negative rows index from the end)"
    assert bool(((c["owner"] % (P.POSE_F + P.POSE_K)) < P.POSE_F).any()) or N < 2, "a ray of a fixed pose"


def _lattice(nu, perturb):
    return P.place_case(next(c for c in P.PLACE_CASES if c[0].startswith(f"lattice{nu}-p{perturb}")))


@pytest.mark.parametrize("nu", [33, 17])
def test_planted_rays_are_there(nu):
    c = _lattice(nu, 0)
    z, d, pl = P.place_z(c), c["target_d"], c["planted"]
    front, back, band = P.masks(z, d, torch.float64)
    assert list(pl) == ["ties_even", "ties_odd", "no_depth_zero", "no_depth_negative", "below_all", "above_all", "at_far"]
    assert bool(((z * 16) == (z * 16).round()).all()), "without jitter every sample lies on the lattice of 1/16"
    ties = lambda r: int((z[r, 1:] == z[r, :-1]).sum())        # noqa: E731
    zu, zoff, znd = c["tables"]
    r = pl["ties_even"]
    assert float(d[r]) == 1.0 and ties(r) >= (5 if nu == 33 else 3), "several uniform samples equal depth-guided ones on one ray"
    if nu == 33:
        lo, hi = z[r] == 0.875, z[r] == 1.125
        assert int(lo.sum()) == 2 and int(hi.sum()) == 2, "z == d - T and z == d + T, each as a tie"
        assert bool(band[r][lo | hi].all()) and not bool((front[r] | back[r])[lo | hi].any())
    r = pl["ties_odd"]
    lo, hi = z[r] == d[r] - 0.125, z[r] == d[r] + 0.125
    assert int(lo.sum()) == 1 and int(hi.sum()) == 1 and bool(band[r][lo | hi].all()) and ties(r) >= 2
    for name in ("no_depth_zero", "no_depth_negative"):
        r = pl[name]
        assert float(d[r]) <= 0 and ties(r) == 9, "the near list is linspace(near, far): every entry ties a uniform one"
        assert not bool(band[r].any()) and not bool(front[r].any())
    r = pl["no_depth_zero"]
    open_ = ~front[r] & ~back[r]
    assert int(open_.sum()) >= 2 and bool((z[r][open_] <= 0.125).all()), "samples at z <= T that only d > 0 keeps out of the band"
    r = pl["below_all"]
    assert float(z[r, 0]) < 0 and int((z[r] < 0).sum()) == 3 and float(d[r]) > 0
    r = pl["above_all"]
    assert bool((z[r, :nu] == zu).all()) and float(z[r, nu]) > 4.0 and bool(front[r, :nu].all()) and int(back[r].sum()) == 2
    r = pl["at_far"]
    assert ties(r) >= 2 and float(z[r, -1]) == 4.25
    # points that leave the box, and points inside it
    ro, rd = P.pose_rays(c["rot"], c["trans"], c["fixed"], c["owner"], c["table"][c["rows"], :3])
    xn = P.place_xn(ro.contiguous(), rd.contiguous(), z, c["cfg"])
    assert bool(((xn < 0) | (xn > 1)).any()) and bool(((xn > 0) & (xn < 1)).all(1).any())


def test_jitter_reaches_both_ends():
    c = _lattice(33, 1)
    still = dict(c, noise=None, cfg=dict(c["cfg"], training=dict(c["cfg"]["training"], perturb=0)))
    z0, z1 = P.place_z(still), P.place_z(c)
    N = c["N"]
    assert not torch.equal(z0, z1) and bool((c["noise"][:N - 1, 0] == 0).all()) and float(c["noise"][N - 1, 0]) == P.ONE_BELOW
    assert torch.equal(z1[:N - 1, 0], z0[:N - 1, 0]), "noise 0 on the first sample leaves it at the lower edge of its interval"
    assert float(z1[N - 1, 0]) > float(z0[N - 1, 0]) and float(z1[0, -1]) <= float(z0[0, -1])
    assert bool((z1[:, 1:] >= z1[:, :-1]).all()), "noise below 1 keeps the samples in order"


# ------------------------------------------------------------------------------------------------------- pose path
def test_pose_cases_cover_what_the_gpu_file_promises():
    assert {c[0] for c in P.POSE_CASES} == set(P.POSE_NS) and {c[1:3] for c in P.POSE_CASES} == set(P.POSE_FK)
    for fk in P.POSE_FK:
        assert {c[0] for c in P.POSE_CASES if c[1:3] == fk} == set(P.POSE_NS)
        assert {c[3] for c in P.POSE_CASES if c[1:3] == fk} == set(P.LAYOUTS)
    distinct = set()
    kinds, mid, neg, unowned = set(), False, False, False
    for key in P.POSE_CASES:
        c = P.pose_case(key)
        N, F, K = key[:3]
        own = c["owner"] % (F + K)
        assert int(c["owner"].min()) >= -(F + K) and int(c["owner"].max()) < F + K, "no owner out of range"
        for w in range(N // 64):
            wave = own[64 * w: 64 * w + 64]
            distinct.add(int(wave.unique().numel()))
            mid = mid or (int(wave.unique().numel()) == 2 and bool(wave[31] != wave[32]))
        neg = neg or bool((c["owner"] < 0).any())
        unowned = unowned or any(int((own == F + k).sum()) == 0 for k in range(K))
        kinds |= {P.QUAT_KINDS[(key[4] + k) % 6] for k in range(K)}
    assert {1, 2, 4, 5, 64} <= distinct, "waves with one owner, a boundary, exactly PR_MAXSEG owners, one more, and 64"
    assert mid and neg and unowned and kinds == set(P.QUAT_KINDS)
    q = P.pose_case(next(c for c in P.POSE_CASES if c[2] >= 6))["rot"]
    norms = sorted(float(x) for x in q[:6].norm(dim=1))
    assert abs(norms[0] - 0.5) < 1e-6 and abs(norms[-1] - 2.0) < 1e-6 and any(abs(n - 1.001) < 1e-5 for n in norms)
    assert any(float(x[0]) == 0.0 for x in q[:6]) and any(x.tolist() == [1.0, 0.0, 0.0, 0.0] for x in q[:6])


def _gate_check(a, ref, y32, groups, ceiling, what):
    err, e32 = P.group_errors(a, ref, groups), P.group_errors(y32, ref, groups)
    for name, _ in groups:
        assert float(e32[name].max()) <= ceiling, f"{what}: the yardstick of {name} is above the ceiling"
        if a is not y32:
            gate = P.working_gate(e32[name], ceiling)
            n = int(np.argmax(err[name] / gate))
            assert bool((err[name] <= gate).all()), f"{what}: {name} of row {n}: {err[name][n]:.2e} (gate {gate[n]:.2e}, e32 {e32[name][n]:.2e})"
    return max(float(e.max()) for e in e32.values())


@pytest.mark.parametrize("key", P.POSE_CASES, ids=P.pose_id)
def test_pose_yardstick_and_emulation_meet_the_gate(key):
    """the fp32 chain of the reference (e32) is under the ceilings, and pose_rays_bwd restated in fp32 with ANOTHER summation order
    is inside max(8 e32, 64 * 2^-24): the gate is one that fp32 code can meet, whatever order it adds in"""
    c = P.pose_case(key)
    r64, r32 = P.pose_reference(c, torch.float64), P.pose_reference(c, torch.float32)
    assert torch.equal(r64[0].float(), r32[0]), "rays_o is the translation itself"
    _gate_check(r32[1], r64[1], r32[1], P.RAY_GROUP, P.CEIL_VALUE, "rays_d")
    em_rot, em_trans = P.emulate_pose_bwd(c)
    _gate_check(em_rot, r64[2], r32[2], P.POSE_GROUPS_ROT, P.CEIL_GRAD, "emulation")
    _gate_check(em_trans, r64[3], r32[3], P.POSE_GROUPS_TRANS, P.CEIL_GRAD, "emulation")
    own = c["owner"] % (key[1] + key[2])
    for k in range(key[2]):
        if int((own == key[1] + k).sum()) == 0:
            assert bool((r64[2][k] == 0).all()) and bool((r64[3][k] == 0).all()), "a pose without a ray: float64 gradient exactly 0"


def test_place_pose_bwd_cases_and_yardstick():
    assert {c[0] for c in P.PPB_CASES} == set(P.PPB_NS) and {c[1] for c in P.PPB_CASES} == set(P.PPB_SS)
    assert {(c[0], c[1], c[2]) for c in P.PPB_CASES} == {(n, s, u) for n in P.PPB_NS for s in P.PPB_SS for u in (True, False)}
    assert any(c[3] == 2.0 and c[2] for c in P.PPB_CASES) and any(c[3] == 2.0 and not c[2] for c in P.PPB_CASES)
    fixed_mixed = False
    for key in P.PPB_CASES:
        c = P.ppb_case(key)
        own = c["owner"] % (c["F"] + c["K"])
        fixed_mixed = fixed_mixed or (bool((own < c["F"]).any()) and bool((own >= c["F"]).any()))
        r64, r32 = P.ppb_reference(c, torch.float64), P.ppb_reference(c, torch.float32)
        _gate_check(r32[0], r64[0], r32[0], P.POSE_GROUPS_ROT, P.CEIL_GRAD, P.ppb_id(key))
        _gate_check(r32[1], r64[1], r32[1], P.POSE_GROUPS_TRANS, P.CEIL_GRAD, P.ppb_id(key))
    assert fixed_mixed


# ------------------------------------------------------------------------------------- frequency and normalisation
@pytest.mark.parametrize("n_freq", P.FREQ_NFREQ)
@pytest.mark.parametrize("M", P.FREQ_MS)
def test_frequency_answer_and_yardstick(M, n_freq):
    x, dout = P.freq_case(M, n_freq)
    flat = x.reshape(-1)
    if M >= 3:
        assert {0.0, 0.5, 1.0} <= set(flat.tolist()) and float(flat.min()) < 0 and float(flat.max()) > 1
    o64, dx64 = P.freq_reference(x, dout, n_freq, torch.float64)
    o32, dx32 = P.freq_reference(x, dout, n_freq, torch.float32)
    # the answer, rounded once, is the oracle's own forward and backward
    assert torch.equal(o64.float(), tcnn_cpu.frequency_forward(x, n_freq))
    assert P.value_error(dx64, tcnn_cpu.frequency_backward(x, dout, n_freq)) <= 1e-5
    assert P.value_error(o32, o64) <= P.CEIL_VALUE
    assert float(P.group_errors(dx32, dx64, (("dx", slice(0, 3)),))["dx"].max()) <= P.CEIL_GRAD


# ------------------------------------------------------------------------------------------------------------ Adam
ADAM_CPU_NS = [n for n in P.ADAM_NS if n <= 16385]


@pytest.mark.parametrize("hyper", P.ADAM_HYPER, ids=lambda h: f"lr{h[0]:g}-b{h[1]:g},{h[2]:g}-eps{h[3]:g}-wd{h[4]:g}")
def test_adam_bound_holds_the_emulation_and_rejects_the_mutations(hyper):
    lr, b1, b2, eps, wd = hyper
    killed = {"no_wd": 0, "eps_in_sqrt": 0}
    for n in ADAM_CPU_NS:
        for step in (1, 3, 1000):
            state = P.adam_state(n)
            want = P.adam_answer(*state, step, lr, b1, b2, eps, wd)
            bound = P.adam_bound(*state, step, lr, b1, b2, eps, wd)
            got = P.adam1_f32(*state, step, lr, b1, b2, eps, wd)
            for name, a, r, b in zip("pmv", got, want, bound):
                worst = float(((a.double() - r).abs() / b).max())
                assert worst <= 1.0, f"{name}: n {n} step {step}: the fp32 restatement is at {worst:.2f} of the bound"
                assert worst >= 1e-3 or n < 100, f"{name}: the bound is {1 / max(worst, 1e-30):.0f} times what fp32 needs: too loose"
            for mut in killed:
                bad = P.adam1_f32(*state, step, lr, b1, b2, eps, wd, mutation=mut)
                killed[mut] += sum(int(((a.double() - r).abs() > b).sum()) for a, r, b in zip(bad, want, bound))
    assert killed["eps_in_sqrt"] > 0, "eps inside the square root stays inside the bound"
    assert (killed["no_wd"] > 0) == (wd != 0), "dropped weight decay stays inside the bound"


def test_adam_state_holds_the_planted_elements():
    p, g, m, v = P.adam_state(1025)
    assert float(g[0]) == 0 and float(v[0]) == 0 and float(m[0]) == 0 and float(v[1]) == 0 and float(m[1]) != 0
    assert float(g[2]) == 0 and float(v[2]) > 0 and float(p[3]) == 0
    nz = g[g != 0].abs()
    assert float(nz.min()) <= 2e-12 and float(nz.max()) >= 5e-3 and int((g == 0).sum()) > 100
    # dense semantics: an element with g = 0 and m != 0 still moves
    p1, m1, v1 = P.adam_answer(p, g, m, v, 1, 0.01, 0.9, 0.99, 1e-8, 0.0)
    assert float(p1[1]) != float(p[1]) and float(p1[0]) == float(p[0])


def test_adam_scalars_are_torchs():
    """adam_answer is torch.optim.Adam: one step of it in float64 on the same state"""
    p, g, m, v = (t.double() for t in P.adam_state(1023))
    lr, b1, b2, eps, wd = P.f32(0.001), P.f32(0.9), P.f32(0.999), P.f32(1e-8), P.f32(1e-6)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    q.grad = g.clone()
    opt.state[q] = dict(step=torch.tensor(4.0), exp_avg=m.clone(), exp_avg_sq=v.clone())
    opt.step()
    p1, m1, v1 = P.adam_answer(*P.adam_state(1023), 5, 0.001, 0.9, 0.999, 1e-8, 1e-6)
    np.testing.assert_allclose(q.detach().numpy(), p1.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(opt.state[q]["exp_avg"].numpy(), m1.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(opt.state[q]["exp_avg_sq"].numpy(), v1.numpy(), rtol=1e-12, atol=1e-300)
