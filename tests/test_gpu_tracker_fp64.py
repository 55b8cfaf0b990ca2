"""GPU (-m gpu): the three kernels of the particle-swarm pre-tracker against INDEPENDENT float64 answers (tests/tracker_cpu.py;
tests/test_tracker_cpu.py holds the inputs, the answers and the bounds to their conditions):

  particles   ro_particles_kernel (csrc/ro.hip) through mipsf_ro_particles: pst7[:, 1:7] BIT FOR BIT fl32(pst * search); qw and every
              word of xn under their derived bounds against oracle/ro_cpu.py (pose_6d_to_7d, particle_points) and
              oracle/path_cpu.py (normalise_points) in float64; both sample orders, both normalisations, norm_factor 1 and 2, P in
              {1, 3, 4, 5, 37}, n in {1, 63, 64, 65, 129}, the planted particles (identity, s == 1, s > 1, s == 0).
  fitness     ro_fitness_kernel (csrc/elementwise.hip) through mipsf_ro_fitness (stride 10, sentinels in the other columns) and
              mipsf_ro_fitness_sdf (stride 1, both orders) against ro_cpu.mean_masked_sdf in float64; every depth invalid: 0.0.
  update      ro_update_kernel through mipsf_ro_update: every word of state[0:29] under its bound against ro_cpu.swarm_update in
              float64 on the advanced set fp32 decides; count, flag and f0 exactly; the nothing-advanced branch word by word.
  order       ro_particles -> an analytic SDF on the host from the device's own xn -> the stride-1 fitness in the SAME order, held to
              the float64 mean over particle p's own points (P = 5, n = 65: a transposed index reads another particle's point).
  carry       two rounds at P = 37, n = 65, each held to the restatement from the state the device left: words 12..17 as the update
              writes them are what the particle kernel reads.

Every output buffer lies between guard words and is pre-filled; the inputs and the guards are compared bit for bit after every
launch.  Nothing is asserted about the fp32 restatement (tracker_cpu's F): the lines printed say in how many words the device
differs from it.  Measured on an MI355X: see DESIGN.md, "The particle-swarm tracker's kernels against float64"."""
import ctypes as C

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, ops
from mipsfusion_amd._lib import dptr, lib, stream_ptr

from . import tracker_cpu as T

pytestmark = pytest.mark.gpu

GUARD = 64                            # floats before and after every output buffer
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def report(kernel, tag, name, worst, off, words):
    """worst: (the worst error / bound over the words that are not the float64 answer rounded once, the number of those that are)"""
    print(f"\n  fp64 | {kernel} | {tag} | {name} | worst error / bound {worst[0]:.3f} ({worst[1]} of {words} words are float64 rounded once)"
          f" | {off} words off the fp32 restatement", end="")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def off_words(a, b):
    return int((bits(a) != bits(b)).sum())


def guarded(dev, words):
    """-> the whole buffer and the view the kernel gets; all of it pre-filled"""
    buf = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + words]


def assert_guards(kernel, tag, name, buf):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all(), f"{kernel} {tag}: a write before the start of {name}"
    assert (b[-GUARD:] == SENTINEL).all(), f"{kernel} {tag}: a write past the end of {name}"


def upload(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrays]


def assert_untouched(kernel, tag, tensors, arrays, names):
    for t, a, name in zip(tensors, arrays, names):
        assert off_words(t.cpu().numpy().reshape(-1), np.asarray(a).reshape(-1)) == 0, f"{kernel} {tag}: the input {name} was written"


def worst_ratio(kernel, tag, name, got, ans, bound):
    """every word under its bound (a bound of 0: the word is equal); -> what ``report`` prints"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ans.shape == bound.shape, (got.shape, ans.shape, bound.shape)
    assert not np.isnan(got).any(), f"{kernel} {tag}: NaN in {name}"
    err = np.abs(got - ans)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[i] <= 1.0, f"{kernel} {tag}: {name}{list(i)} = {got[i]!r} against {ans[i]!r}: off by {err[i]:.3e}, bound {bound[i]:.3e}"
    # a word that IS the float64 answer rounded once cannot be nearer: where its bound is that one known rounding, the ratio is 1 by
    # construction.  The figure printed is the worst of the other words.
    once = got == ans.astype(np.float32).astype(np.float64)
    return float(np.where(once, 0.0, ratio).max()), int(once.sum())


def render_cfg(cfg):
    return ops.make_render_cfg(cfg, cfg["mapping"]["bound"], cfg["mapping"]["localMLP_max_len"], 1, 0, 0.0)


# ------------------------------------------------------------------------------------------------------ launches
def run_particles(dev, tag, pst, state, rays, td, cfg, point_major):
    """-> xn [P,n,3], pst7 [P,7] (numpy fp32, xn back in (particle, point) order)"""
    P, n = pst.shape[0], rays.shape[0]
    rc = render_cfg(cfg)
    assert bool(rc.use_bound) == cfg["grid"]["use_bound_normalize"] and float(rc.norm_factor) == cfg["training"]["norm_factor"]
    ins = upload(dev, pst, state, rays, td)
    xbuf, xn = guarded(dev, P * n * 3)
    pbuf, p7 = guarded(dev, P * 7)
    _lib.check(lib().mipsf_ro_particles(dptr(ins[0]), dptr(ins[1]), dptr(ins[2]), dptr(ins[3]), C.byref(rc), dptr(xn), dptr(p7), P, n,
                                        1 if point_major else 0, stream_ptr()), "ro_particles")
    torch.cuda.synchronize()
    assert_untouched("ro_particles", tag, ins, (pst, state, rays, td), ("pst", "state", "rays_d_cam", "target_d"))
    assert_guards("ro_particles", tag, "xn", xbuf)
    assert_guards("ro_particles", tag, "pst7", pbuf)
    return T.unordered(xn.cpu().numpy().reshape(P * n, 3), P, n, point_major), p7.cpu().numpy().reshape(P, 7)


def run_fitness(dev, tag, raw, td, trunc, P, n, form):
    ins = upload(dev, raw, td)
    obuf, out = guarded(dev, P)
    if form == "raw10":
        rcode = lib().mipsf_ro_fitness(dptr(ins[0]), 10, dptr(ins[1]), trunc, dptr(out), P, n, stream_ptr())
    else:
        rcode = lib().mipsf_ro_fitness_sdf(dptr(ins[0]), dptr(ins[1]), trunc, dptr(out), P, n, 1 if form == "sdf-point" else 0, stream_ptr())
    _lib.check(rcode, "ro_fitness")
    torch.cuda.synchronize()
    assert_untouched("ro_fitness", tag, ins, (raw, td), ("raw", "target_d"))
    assert_guards("ro_fitness", tag, "mean_masked", obuf)
    return out.cpu().numpy()


def run_update(dev, tag, mm, pst7, state, rescale):
    """-> the 32 words of the state after the launch"""
    ins = upload(dev, mm, pst7)
    sbuf, st = guarded(dev, T.STATE_FLOATS)
    st.copy_(torch.from_numpy(state))
    _lib.check(lib().mipsf_ro_update(dptr(ins[0]), dptr(ins[1]), dptr(st), T.SDF_WEIGHT, rescale, mm.shape[0], stream_ptr()), "ro_update")
    torch.cuda.synchronize()
    assert_untouched("ro_update", tag, ins, (mm, pst7), ("mean_masked", "pst7"))
    assert_guards("ro_update", tag, "state", sbuf)
    new = st.cpu().numpy()
    assert off_words(new[T.STATE_USED:], state[T.STATE_USED:]) == 0, f"ro_update {tag}: state words 29..31 were written"
    return new


# ------------------------------------------------------------------------------------------------------- checks
def check_particles(tag, xn, p7, pst, state, rays, td, cfg):
    pst7a, xna, *_ = T.particle_answer(pst, state, rays, td, cfg)
    b7, bx = T.particle_bound(pst, state, rays, td, cfg)
    y7, yx, _ = T.particles(T.F, pst, state, rays, td, cfg)
    want = (pst.astype(np.float64) * state[T.SEARCH:T.SEARCH + 6].astype(np.float64)).astype(np.float32)
    assert off_words(p7[:, 1:], want) == 0, f"ro_particles {tag}: pst7[:, 1:7] is not fl32(pst * search) bit for bit"
    worst_ratio("ro_particles", tag, "pst7", p7, pst7a.numpy(), b7)
    r7 = worst_ratio("ro_particles", tag, "qw", p7[:, 0], pst7a.numpy()[:, 0], b7[:, 0])
    rx = worst_ratio("ro_particles", tag, "xn", xn, xna.numpy(), bx)
    report("ro_particles", tag, "qw", r7, off_words(p7[:, 0], y7.v[:, 0]), p7.shape[0])
    report("ro_particles", tag, "xn", rx, off_words(xn, yx.v), xn.size)


def check_update(tag, new, mm, pst7, state, rescale):
    ans, bound = T.update_answer(mm, pst7, state, rescale), T.update_bound(mm, pst7, state, rescale)
    y, adv, _, _ = T.update(T.F, mm, pst7, state, rescale)
    ratio = worst_ratio("ro_update", tag, "state", new[:T.STATE_USED], ans, bound)
    assert new[T.NBETTER] == adv.sum(), f"ro_update {tag}: {new[T.NBETTER]} particles advanced, fp32 decides {adv.sum()}"
    assert new[T.SUCCESS] == (1.0 if adv.any() else 0.0)
    assert off_words(new[T.FIT0], np.float32(mm[0]) * np.float32(T.SDF_WEIGHT)) == 0, f"ro_update {tag}: word 20 is not fl32(mean_masked[0] * 1000)"
    if not adv.any():
        assert off_words(new[:12], state[:12]) == 0, f"ro_update {tag}: nothing advanced, but the pose was written"
        assert off_words(new[T.MEAN_T:T.MEAN_T + 7], np.array([1, 0, 0, 0, 0, 0, 0], np.float32)) == 0
        assert off_words(new[T.MEAN_SDF], mm[0]) == 0
    report("ro_update", tag, f"state[0:29], {int(adv.sum())} advanced", ratio, off_words(new[:T.STATE_USED], y.v), T.STATE_USED)


# -------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("key", T.PARTICLE_CASES, ids=T.case_id)
def test_particles(dev, key):
    c = T.particle_case(key)
    a = (c["pst"], c["state"], c["rays"], c["td"], c["cfg"])
    xn, p7 = run_particles(dev, key[0], *a, c["point_major"])
    check_particles(key[0], xn, p7, *a)


@pytest.mark.parametrize("key", T.FITNESS_CASES, ids=T.case_id)
def test_fitness(dev, key):
    c = T.fitness_case(key)
    got = run_fitness(dev, key[0], c["raw"], c["td"], c["trunc"], c["P"], c["n"], c["form"])
    ans, bound = T.fitness_answer(c["sdf"], c["td"], c["trunc"]).numpy(), T.fitness_bound(c["sdf"], c["td"], c["trunc"])
    ratio = worst_ratio("ro_fitness", key[0], "mean_masked", got, ans, bound)
    if c["none_valid"]:
        assert off_words(got, np.zeros(c["P"], np.float32)) == 0, "every depth invalid: exactly +0.0"
    report("ro_fitness", key[0], "mean_masked", ratio, off_words(got, T.fitness(T.F, c["sdf"], c["td"], c["trunc"]).v), got.size)


@pytest.mark.parametrize("key", T.UPDATE_CASES, ids=T.case_id)
def test_update(dev, key):
    c = T.update_case(key)
    new = run_update(dev, key[0], c["mm"], c["pst7"], c["state"], c["rescale"])
    check_update(key[0], new, c["mm"], c["pst7"], c["state"], c["rescale"])


def host_sdf(xn, cfg):
    """the analytic SDF of the device's own points, rounded to fp32 [P,n]"""
    return T.plane_sdf(xn, cfg).astype(np.float32)


@pytest.mark.parametrize("point_major", [0, 1], ids=["particle-major", "point-major"])
def test_order_contract(dev, point_major):
    """The answer is the float64 mean over particle p's OWN points (the answer's points, not the device's rows), so either kernel
    indexing the other way breaks it.  Bound: the fitness bound on the SDF values fed, plus what the SDF inherits from xn: the plane
    is linear, |d sdf| <= sum_k |n_k| norm_factor div_k |d xn_k|, and its cast to fp32 adds U |sdf|; the mean of trunc * that over
    the valid points."""
    c = T.particle_case(next(k for k in T.PARTICLE_CASES if k[1] == 5 and k[2] == 65))
    P, n, cfg, td = c["P"], c["n"], c["cfg"], c["td"]
    tag = f"P{P}-n{n}-pm{point_major}"
    a = (c["pst"], c["state"], c["rays"], td, cfg)
    xn, _ = run_particles(dev, tag, *a, point_major)
    sdf = host_sdf(xn, cfg)
    got = run_fitness(dev, tag, T.ordered(sdf, point_major), td, T.TRUNC, P, n, "sdf-point" if point_major else "sdf-row")
    _, xna, *_ = T.particle_answer(*a)
    _, bx = T.particle_bound(*a)
    sdf_own = T.plane_sdf(xna.numpy(), cfg)
    _, div, nf = T.norm_consts(cfg)
    e_sdf = (bx * (np.abs(T.PLANE_N) * nf * div)).sum(-1) + T.U * np.abs(sdf_own)
    ans = T.fitness_answer(sdf_own, td, T.TRUNC).numpy()
    bound = T.fitness_bound(sdf, td, T.TRUNC) + (T.TRUNC * e_sdf * (td > 0)[None, :]).sum(1) / n
    assert (bound < 1e-5 * ans).all(), "the bound of the order contract is not vacuous"
    ratio = worst_ratio("order", tag, "mean_masked", got, ans, bound)
    report("order", tag, "mean_masked over the particle's own points", ratio, off_words(got, T.fitness(T.F, sdf, td, T.TRUNC).v), got.size)


def test_two_rounds_carry_the_state(dev):
    c = T.particle_case(("carry-P37-n65-pm1-bound-nf1-small", 37, 65, 1, True, 1.0, "small"))
    P, n, cfg, td, pm = c["P"], c["n"], c["cfg"], c["td"], c["point_major"]
    state = c["state"].copy()
    for rnd in range(2):
        tag = f"round{rnd}"
        xn, p7 = run_particles(dev, tag, c["pst"], state, c["rays"], td, cfg, pm)
        check_particles(tag, xn, p7, c["pst"], state, c["rays"], td, cfg)
        sdf = host_sdf(xn, cfg)
        mm = run_fitness(dev, tag, T.ordered(sdf, pm), td, T.TRUNC, P, n, "sdf-point")
        ratio = worst_ratio("ro_fitness", tag, "mean_masked", mm, T.fitness_answer(sdf, td, T.TRUNC).numpy(), T.fitness_bound(sdf, td, T.TRUNC))
        report("ro_fitness", tag, "mean_masked", ratio, off_words(mm, T.fitness(T.F, sdf, td, T.TRUNC).v), mm.size)
        new = run_update(dev, tag, mm, p7, state, T.RESCALE)
        check_update(tag, new, mm, p7, state, T.RESCALE)
        assert off_words(new[T.SEARCH:T.SEARCH + 6], state[T.SEARCH:T.SEARCH + 6]) == 6, "the round moved every word of the search size"
        state = new
