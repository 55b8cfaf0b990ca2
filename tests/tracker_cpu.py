"""Inputs, float64 answers and derived per-element bounds for the particle-swarm pre-tracker's three kernels: ro_particles_kernel and
ro_update_kernel (csrc/ro.hip) and ro_fitness_kernel (csrc/elementwise.hip, through mipsf_ro_fitness and mipsf_ro_fitness_sdf).
No tests here and no GPU: tests/test_tracker_cpu.py holds this helper to its conditions, tests/test_gpu_tracker_fp64.py holds the
kernels to it.

The ANSWERS are code the repository already has, evaluated in float64 on the fp32 words the device gets: oracle/ro_cpu.py
(pose_6d_to_7d, particle_points, mean_masked_sdf, swarm_update) and oracle/path_cpu.py (normalise_points).  Nothing in them is
rounded to fp32.  ONE thing is decided in fp32, because it is the specification: the reference compares fp32 fitness values
(`fitness < fitness[0]`), so the advanced set is taken on fl32(mean_masked * 1000); the weights, the sums and everything after them
are float64 of the exact product.  The kernel's fp32 literals (0.00001f, 1e-5f, 0.0001f) enter as the values their fp32 forms hold.

The RESTATEMENT (pose7, particles, fitness, update below) is the kernels' arithmetic written once more, operation by operation in
the kernels' parenthesisation (the library is built with -ffp-contract=off), over an abstract number.  Two numbers run through it:

  F   numpy fp32 (float64 where the kernel widens: the normalisation, the update's sums).  This is the YARDSTICK: what a correct fp32
      kernel gives if sqrt and division round as numpy's do.  It is used on the CPU only, to hold the bounds to their conditions; the
      GPU test may print in how many words the device differs from it and asserts nothing about it.
  E   float64 value + a first-order bound on |fp32 result - value|.  This is the BOUND.  Every fp32 operation (+ - * / sqrt and the
      cast from double) adds ONE rounding, U |result| with U = 2^-24, to the errors its operands carry, which are pushed through to
      first order: |a| e_b + |b| e_a for a product, (e_a + |a / b| e_b) / |b| for a quotient, e_a / (sqrt(a) + sqrt(a - e_a)) for a
      root.  So a word's bound is the sum, over the roundings on the paths that reach it, of U times the magnitude each acts on,
      carried to that word: the count of roundings on the longest path is written beside each formula below.  Where every operand is
      exact, the rounding is not bounded but KNOWN, |fl32(v) - v|: the planted particles (identity, s == 1, s == 0) and the lattice
      fitness values stay exact as far as the arithmetic is, and their words are held bit for bit by a bound of 0.  Operations in
      double add nothing (2^-53 against 2^-24).  Nothing here is measured.

The update's weights are the exception to running the errors through operation by operation: f0 - f cancels, and every weight
carries the SAME error of f0.  Their errors, U (|f0| + |f_p| + |w_p|) from the two products and the subtraction, go through the
Jacobian of the answer itself (autograd through ro_cpu.swarm_update in float64), which sees that a common shift of all weights
leaves a normalised mean almost alone; the roundings after the weights run through E as everywhere else."""
import functools
import math

import numpy as np
import torch

from oracle import path_cpu, ro_cpu

from .step_cpu import bound64, place_cfg

U = 2.0 ** -24                       # one fp32 rounding
FLT_MIN = 2.0 ** -126
WAVE = 64
SDF_WEIGHT = 1000.0                  # exact in fp32


def f32c(x):
    """the value an fp32 literal or scalar argument holds, as a python float"""
    return float(np.float32(x))


C_WSUM, C_NQ, C_SZ = f32c(0.00001), f32c(1e-5), f32c(0.0001)
TRUNC, RESCALE = f32c(0.1), 0.5

# state layout (include/mipsf.h MIPSF_RO_*)
ROT, TRANS, SEARCH, SUCCESS, MEAN_SDF, FIT0, MEAN_T, NBETTER, STATE_USED, STATE_FLOATS = 0, 9, 12, 18, 19, 20, 21, 28, 29, 32


# ==================================================================================================== the two numbers
def _scalar(x, wide):
    x = float(x)
    assert wide or f32c(x) == x, f"{x!r} is not an fp32 value: a literal's own representation error would count as kernel error"
    return x


class F:
    """fp32 values (float64 after .wide()); ``tiny`` is the smallest non-zero fp32 magnitude any operation has produced"""
    tiny = math.inf

    def __init__(self, v):
        self.v = np.asarray(v)
        assert self.v.dtype in (np.float32, np.float64), self.v.dtype

    @property
    def is_wide(self):
        return self.v.dtype == np.float64

    def _o(self, o):
        if isinstance(o, F):
            assert o.v.dtype == self.v.dtype, "fp32 and double operands mixed"
            return o.v
        return self.v.dtype.type(_scalar(o, self.is_wide))

    def _mk(self, v):
        v = np.asarray(v)
        assert v.dtype == self.v.dtype
        if v.dtype == np.float32:
            nz = np.abs(v[v != 0])
            if nz.size:
                F.tiny = min(F.tiny, float(nz.min()))
        return F(v)

    def __add__(self, o): return self._mk(self.v + self._o(o))
    def __sub__(self, o): return self._mk(self.v - self._o(o))
    def __rsub__(self, o): return self._mk(self._o(o) - self.v)
    def __mul__(self, o): return self._mk(self.v * self._o(o))
    def __truediv__(self, o): return self._mk(self.v / self._o(o))
    def __rtruediv__(self, o): return self._mk(self._o(o) / self.v)
    def __getitem__(self, i): return F(self.v[i])

    def sqrt(self):
        with np.errstate(invalid="ignore"):
            return self._mk(np.sqrt(self.v))

    def abs(self): return F(np.abs(self.v))
    def wide(self): return F(self.v.astype(np.float64))

    def narrow(self):
        v = self.v.astype(np.float32)
        return F(v)._mk(v)

    def sum(self):
        assert self.is_wide, "the kernels sum in double only"
        return F(np.asarray(self.v.sum()))

    def const(self, x): return F(np.full(self.v.shape, _scalar(x, self.is_wide), self.v.dtype))
    def dec(self): return self.v                                   # the values a comparison of the kernel sees
    def f32(self): return self.v.astype(np.float32)


def _known(v):
    """|fl32(v) - v|: the rounding of an exactly known value"""
    return np.abs(v.astype(np.float32).astype(np.float64) - v)


class E:
    """float64 value ``v`` and first-order bound ``e`` on |fp32 result - v| (see the module docstring)"""

    def __init__(self, v, e=None, wide=False):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)
        self.is_wide = wide

    def _o(self, o):
        if isinstance(o, E):
            assert o.is_wide == self.is_wide, "fp32 and double operands mixed"
            return o.v, o.e
        return np.float64(_scalar(o, self.is_wide)), np.float64(0.0)

    def _r(self, v, e):
        """the operation's own rounding on top of the carried error e"""
        v, e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)
        if not self.is_wide:
            e = e + np.where(e == 0, _known(v), U * np.abs(v))
        return E(v, e, self.is_wide)

    def __add__(self, o):
        ov, oe = self._o(o)
        return self._r(self.v + ov, self.e + oe)

    def __sub__(self, o):
        ov, oe = self._o(o)
        return self._r(self.v - ov, self.e + oe)

    def __rsub__(self, o):
        ov, oe = self._o(o)
        return self._r(ov - self.v, self.e + oe)

    def __mul__(self, o):
        ov, oe = self._o(o)
        return self._r(self.v * ov, np.abs(self.v) * oe + np.abs(ov) * self.e)

    def __truediv__(self, o):
        ov, oe = self._o(o)
        q = self.v / ov
        return self._r(q, (self.e + np.abs(q) * oe) / np.abs(ov))

    def __rtruediv__(self, o):
        ov, oe = self._o(o)
        q = ov / self.v
        return self._r(q, (oe + np.abs(q) * self.e) / np.abs(self.v))

    def __getitem__(self, i): return E(self.v[i], self.e[i], self.is_wide)

    def sqrt(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            root = np.sqrt(self.v)
            # |sqrt(a') - sqrt(a)| = |a' - a| / (sqrt(a') + sqrt(a)) <= e / (sqrt(a) + sqrt(max(a - e, 0)))
            low = np.sqrt(np.maximum(self.v - self.e, 0.0))
            e = np.where(self.e == 0, 0.0, self.e / (root + low))
        return self._r(root, e)

    def abs(self): return E(np.abs(self.v), self.e, self.is_wide)
    def wide(self): return E(self.v, self.e, True)
    def narrow(self): return E(self.v, self.e, False)._r(self.v, self.e)

    def sum(self):
        assert self.is_wide, "the kernels sum in double only"
        return E(self.v.sum(), self.e.sum(), True)

    def const(self, x): return E(np.full(self.v.shape, _scalar(x, self.is_wide)), None, self.is_wide)
    def dec(self): return self.v                                   # float64 decides on the float64 value
    def f32(self): return self.v.astype(np.float32)                # (the fitness products are exact in double: this IS the fp32 product)


def where(c, a, b):
    if isinstance(a, F):
        return F(np.where(c, a.v, b.v))
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e), a.is_wide)


def stack(items, axis):
    if isinstance(items[0], F):
        return F(np.stack([np.broadcast_to(i.v, items[0].v.shape) for i in items], axis))
    return E(np.stack([i.v for i in items], axis), np.stack([i.e for i in items], axis), items[0].is_wide)


# ==================================================================================================== the restatement
def quat_to_mat(w, x, y, z):
    """csrc/ro.hip quat_to_mat.  Longest path to a word: 4 squares + 3 sums + the division (two_s: 8), the two products and their
    sum or difference (3), the product with two_s (1), the diagonal's subtraction from 1 (1): 13 roundings"""
    two_s = 2.0 / (((w * w + x * x) + y * y) + z * z)
    return [1.0 - two_s * (y * y + z * z), two_s * (x * y - z * w), two_s * (x * z + y * w),
            two_s * (x * y + z * w), 1.0 - two_s * (x * x + z * z), two_s * (y * z - x * w),
            two_s * (x * z - y * w), two_s * (y * z + x * w), 1.0 - two_s * (x * x + y * y)]


def mat_mul3(a, b):
    """csrc/ro.hip mat_mul3: (a0 b0 + a1 b1) + a2 b2: 3 roundings on the longest path (a product and two sums)"""
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def pose7(N, pst, search):
    """pose_6D_to_7D of ro_particles_kernel.  r = pst * search: ONE correctly rounded product, held bit for bit.  qw: s takes the
    product's rounding twice (r^2), the square's and two sums': 5 roundings on s; 1 - s and the root add one each: 7.  The error of
    s reaches qw through the root as e_s / (2 qw): proportional to U s / qw.  -> r [P,6], s [P], qw [P], inside [P] (s <= 1)"""
    r = N(pst) * N(search)
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    s = (r0 * r0 + r1 * r1) + r2 * r2
    inside = s.dec() <= 1.0
    qw = where(inside, (1.0 - s).sqrt(), s.const(0.0))
    return r, s, qw, inside


def norm_consts(cfg):
    """make_norm (csrc/common.h) in double: x -> ((x - sub) / div) / norm_factor"""
    b, h = bound64(cfg)
    b, h = b.numpy(), h.numpy()
    if cfg["grid"]["use_bound_normalize"]:
        sub, div = b[:, 0], b[:, 1] - b[:, 0]
    else:
        sub, div = -h, 2 * h
    return sub, div, float(cfg["training"]["norm_factor"])


def particles(N, pst, state, rays, td, cfg, mutation=None):
    """ro_particles_kernel -> pst7 [P,7], xn [P,n,3] (particle p, lattice point i), inside [P].

    Roundings on the longest path to a word of xn: r (1), dR through quat_to_mat (13, r's own counted once), aR through mat_mul3
    (3), c = ray * depth (1), the product aR c (1), two sums and the translation (3; the translation itself carries 2: r and the
    sum), the cast of the normalised double (1): K = 22 on U (sum_k |aR_k| |c_k| + |t|) / (div norm_factor), of which the last acts
    on |xn| alone.  E charges each of them against the magnitude it really acts on, so the bound is a small multiple of U (A / div +
    |xn|), not 22 times it."""
    sub, div, nf = norm_consts(cfg)
    if mutation == "sub_plus_L" and not cfg["grid"]["use_bound_normalize"]:
        sub = -sub
    r, s, qw, inside = pose7(N, pst, state[SEARCH:SEARCH + 6])
    rot = [N(state[ROT + k]) for k in range(9)]
    aR = mat_mul3(rot, quat_to_mat(qw, r[:, 0], r[:, 1], r[:, 2]))
    if mutation == "aR5_for_aR2":
        aR[2] = aR[5]
    t = [N(state[TRANS + k]) + r[:, 3 + k] for k in range(3)]
    d = N(td)
    c = [N(rays[:, k]) * d for k in range(3)]
    xn = []
    for k in range(3):
        m = [aR[3 * k + j][:, None] * c[j][None, :] for j in range(3)]
        w = ((m[0] + m[1]) + m[2]) + t[k][:, None]
        xn.append((((w.wide() - float(sub[k])) / float(div[k])) / nf).narrow())
    return stack([qw] + [r[:, k] for k in range(6)], 1), stack(xn, -1), inside


def fitness(N, sdf, td, trunc):
    """ro_fitness_kernel on the SDF values sdf [P,n] (particle p, point j): per lane the sum over j = lane, lane + 64, ..., then the
    xor tree, then / n.  Roundings on the longest path: the product with trunc (1), ceil(n / 64) lane sums, 6 tree levels, the
    division (1), each on at most the sum of |sdf trunc| over the valid points."""
    P, n = sdf.shape
    steps = -(-n // WAVE)
    pad = steps * WAVE - n
    sd = np.pad(sdf, ((0, 0), (0, pad))).reshape(P, steps, WAVE)
    valid = np.pad(td > 0, (0, pad)).reshape(steps, WAVE)            # lanes past n add nothing; -0.0 > 0 is false
    acc = N(np.zeros((P, WAVE), np.float32))
    for k in range(steps):
        term = (N(sd[:, k, :]) * trunc).abs()
        acc = where(np.broadcast_to(valid[k][None, :], (P, WAVE)), acc + term, acc)     # (+ 0.0f for an invalid depth is exact)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0] / float(n)


def update(N, mm, pst7, state, rescale, mutation=None, exact_weights=False):
    """ro_update_kernel -> the 29 words of the state it writes, the advanced set [P], f [P], w [P].

    exact_weights: the weights' own errors are dropped here (update_bound carries them through the Jacobian instead).

    Roundings after the weights, longest path to a rotation word: the product pst7 w (1, summed in double), the cast of the sum (1),
    wsum: cast and + 0.00001f (2), the division (1), the norm: 4 squares, 3 sums, the root, + 1e-5f (9), the division (1),
    quat_to_mat (13), mat_mul3 (3): 31, each on a magnitude of at most 1.  The search size: mt (5) -> |.| + 0.0001f (1), the norm
    of six (6 squares, 5 sums, the root: 12), rescale mean_sdf (mean_sdf: 5; the product 1), * sz (1), / nrm (1), + 0.0001f (1),
    * 2.0f is exact: 28."""
    m = N(mm)
    f = m * SDF_WEIGHT
    f0 = f[0]
    adv = (f.f32() <= f0.f32()) if mutation == "le_for_lt" else (f.f32() < f0.f32())
    live = adv
    if mutation == "loop_P_and_not_255":
        live = adv & (np.arange(len(mm)) < (len(mm) & ~255))
    w = where(live, f0 - f, m.const(0.0))
    w_full = w
    if exact_weights:
        w = E(w.v, None, False)
    s_n = int(live.sum())
    s_w, s_wm = w.wide().sum(), (w * m).wide().sum()
    s_t = [(N(pst7[:, k]) * w).wide().sum() for k in range(7)]
    wsum = s_w.narrow() + C_WSUM
    ok = s_n > 0
    rot = [N(state[ROT + k]) for k in range(9)]
    trans = [N(state[TRANS + k]) for k in range(3)]
    if ok:
        mean_sdf = s_wm.narrow() / wsum
        mt = [s_t[k].narrow() / wsum for k in range(7)]
        nq = (((mt[0] * mt[0] + mt[1] * mt[1]) + mt[2] * mt[2]) + mt[3] * mt[3]).sqrt() + C_NQ
        mt = [mt[k] / nq for k in range(4)] + mt[4:]
        rot = mat_mul3(rot, quat_to_mat(mt[0], mt[1], mt[2], mt[3]))
        trans = [trans[k] + mt[4 + k] for k in range(3)]
    else:
        mean_sdf = m[0]
        mt = [f0.const(1.0)] + [f0.const(0.0)] * 6
    sz = [mt[1 + k].abs() + C_SZ for k in range(6)]
    n2 = sz[0] * sz[0]                                               # (the kernel's 0.f + sz0^2 is exact)
    for k in range(1, 6):
        n2 = n2 + sz[k] * sz[k]
    nrm = n2.sqrt()
    search = []
    for k in range(6):
        v = ((mean_sdf * rescale) * sz[k]) / nrm + C_SZ
        search.append(v if ok or mutation == "no_double" else v * 2.0)
    words = rot + trans + search + [f0.const(1.0 if ok else 0.0), mean_sdf, f0] + mt + [f0.const(float(s_n))]
    return stack(words, 0), adv, f, w_full


# ========================================================================================================== answers
def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def particle_answer(pst, state, rays, td, cfg):
    """float64: oracle/ro_cpu.py pose_6d_to_7d and particle_points, oracle/path_cpu.py normalise_points, / norm_factor
    -> pst7 [P,7], xn [P,n,3], a_rot [P,3,3], a_trans [P,3,1], world [P,n,3] (float64 tensors)"""
    pst7 = ro_cpu.pose_6d_to_7d(t64(pst) * t64(state[SEARCH:SEARCH + 6])[None])
    cam = t64(rays) * t64(td)[:, None]
    world, a_rot, a_trans = ro_cpu.particle_points(t64(state[ROT:ROT + 9]).reshape(3, 3), t64(state[TRANS:TRANS + 3]).reshape(3, 1), pst7, cam)
    b, h = bound64(cfg)
    xn = path_cpu.normalise_points(world, cfg["grid"], b, h).reshape(world.shape) / cfg["training"]["norm_factor"]
    return pst7, xn, a_rot, a_trans, world


def fitness_answer(sdf, td, trunc):
    """float64: oracle/ro_cpu.py mean_masked_sdf on the SDF values sdf [P,n] -> [P]"""
    raw = torch.zeros(sdf.shape + (4,), dtype=torch.float64)
    raw[..., 3] = t64(sdf)
    return ro_cpu.mean_masked_sdf(lambda world: raw, raw, torch.from_numpy(td)[:, None], trunc)


def advanced_fp32(mm):
    """the specification's decision: fl32(mean_masked * 1000) < fl32(mean_masked[0] * 1000)"""
    f = mm.astype(np.float32) * np.float32(SDF_WEIGHT)
    return f < f[0]


def _update_words(fit, mm, pst7, state, rescale, better):
    rot, trans, search, info = ro_cpu.swarm_update(t64(mm), t64(pst7), t64(state[ROT:ROT + 9]).reshape(3, 3),
                                                   t64(state[TRANS:TRANS + 3]).reshape(3, 1), f32c(rescale), fit=fit, better=better,
                                                   consts=(C_WSUM, C_NQ, C_SZ))
    one = lambda x: torch.as_tensor(x, dtype=torch.float64).reshape(1)      # noqa: E731
    return torch.cat([rot.reshape(9), trans.reshape(3), search.reshape(6), one(float(info["success"])), one(info["mean_sdf"]),
                      one(info["fitness0"]), info["mean_transform"].reshape(7), one(float(better.sum()))])


def update_answer(mm, pst7, state, rescale, jacobian=False):
    """float64: oracle/ro_cpu.py swarm_update on the exact products mean_masked * 1000, the advanced set as fp32 decides it
    -> the 29 words (and their Jacobian [29,P] by the fitness values)"""
    better = torch.from_numpy(advanced_fp32(mm))
    fit = t64(mm) * SDF_WEIGHT
    fn = lambda x: _update_words(x, mm, pst7, state, rescale, better)       # noqa: E731
    words = fn(fit)
    if not jacobian:
        return words.numpy()
    return words.numpy(), torch.autograd.functional.jacobian(fn, fit).numpy()


# =========================================================================================================== bounds
def _slack(e, v):
    """float64's own roundings in the answer, 2^-48 of the magnitude -- except where the bound is 0: such a word is exact in every
    format, and is held bit for bit"""
    return e + np.where(e > 0, 2.0 ** -48 * np.abs(v), 0.0)


def particle_bound(pst, state, rays, td, cfg):
    """-> E pst7 [P,7], E xn [P,n,3]: bounds on |device - particle_answer| (E.v is the answer up to float64's own roundings, which
    2^-48 of the magnitude covers)"""
    p7, xn, _ = particles(E, pst, state, rays, td, cfg)
    return _slack(p7.e, p7.v), _slack(xn.e, xn.v)


def fitness_bound(sdf, td, trunc):
    out = fitness(E, sdf, td, trunc)
    return _slack(out.e, out.v)


def update_bound(mm, pst7, state, rescale):
    """-> bound [29] on |device - update_answer|.

    Weights: f0 and f_p carry the rounding of their products, U |f0| and U |f_p|, and the subtraction adds U |w_p| (all three are
    the KNOWN roundings where the product is exact: the lattice cases).  An error d f_p moves word k by J[k,p] d f_p, the
    subtraction's own rounding by the same derivative (w_p = f0 - f_p), and the error of f0 moves every weight at once: J[k,0].
    Everything after the weights: update() in E with exact weights."""
    words, adv, f, w = update(E, mm, pst7, state, rescale, exact_weights=True)
    e_sub = w.e - f.e - f.e[0]                                       # the subtraction's own rounding
    e_p = np.where(adv, f.e + e_sub, 0.0)
    e_p[0] = f.e[0]
    ans, J = update_answer(mm, pst7, state, rescale, jacobian=True)
    return _slack(words.e + np.abs(J) @ e_p, ans)


def update_scale(ans):
    """the scale of each of the 29 words, for the condition that no bound is vacuous: a rotation and a quaternion are of size 1;
    translation, search size and the mean transform's vector part are each measured by the largest word of their group (a component
    that happens to be small is still known only as well as the vector); the scalars by themselves"""
    s = np.ones(STATE_USED)
    s[TRANS:TRANS + 3] = np.abs(ans[TRANS:TRANS + 3]).max()
    s[SEARCH:SEARCH + 6] = np.abs(ans[SEARCH:SEARCH + 6]).max()
    s[MEAN_SDF], s[FIT0] = abs(ans[MEAN_SDF]), abs(ans[FIT0])
    s[MEAN_T + 1:MEAN_T + 4] = max(np.abs(ans[MEAN_T + 1:MEAN_T + 4]).max(), C_SZ)
    s[MEAN_T + 4:MEAN_T + 7] = max(np.abs(ans[MEAN_T + 4:MEAN_T + 7]).max(), C_SZ)
    return s


# ============================================================================================================ cases
def ordered(x, point_major):
    """[P,n,...] -> the rows of the device buffer: particle * n + point, or point * P + particle"""
    x = np.asarray(x)
    if point_major:
        x = np.swapaxes(x, 0, 1)
    return np.ascontiguousarray(x).reshape((-1,) + x.shape[2:])


def unordered(rows, P, n, point_major):
    """the inverse of ``ordered``"""
    rows = np.asarray(rows)
    if point_major:
        return np.ascontiguousarray(np.swapaxes(rows.reshape((n, P) + rows.shape[1:]), 0, 1))
    return rows.reshape((P, n) + rows.shape[1:])


def make_state(gen, search):
    """[32] fp32: a generic rotation (no axis of it along a coordinate axis), a translation inside both boxes, the search size;
    words 18..31 hold values no round would leave there"""
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    q = (q / q.norm()).numpy()
    w, x, y, z = q
    R = np.array([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])
    state = np.zeros(STATE_FLOATS, np.float32)
    state[ROT:ROT + 9] = R
    state[TRANS:TRANS + 3] = np.array([1.0, 3.0, 1.0]) + 0.25 * torch.randn(3, generator=gen, dtype=torch.float64).numpy()
    state[SEARCH:SEARCH + 6] = search
    state[SUCCESS:] = -4242.5 - np.arange(STATE_FLOATS - SUCCESS)
    return state


SEARCH_SMALL = (np.float32(0.02) * np.array([1.0, 1.25, 0.75, 1.5, 0.5, 1.125], np.float32)).astype(np.float32)
SEARCH_WIDE = np.array([2.0, 1.0, 0.5, 0.25, 0.5, 0.125], np.float32)      # with the planted particles (exact values)
PLANTED = (("identity", (0, 0, 0, 0, 0, 0)),                 # row 0 of the template: r = 0, qw = 1, the pose itself
           ("s_is_1", (0.5, 0, 0, 0, 0, 0)),                  # r = (1, 0, 0): s == 1, qw == 0: a half turn
           ("s_above_1", (0.5, 0.5, 0, 0.25, 0, 0)),          # r = (1, 0.5, 0): s = 1.25 > 1: qw = 0, |q|^2 = 1.25
           ("s_is_0", (0, 0, 0, 0.5, -0.25, 1.0)))            # a translation only

# (name, P, n, point_major, use_bound, norm_factor, search): every P in {1,3,4,5,37}, every n in {1,63,64,65,129}
PARTICLE_CASES = (("P1-n1-pm0-bound-nf1-small", 1, 1, 0, True, 1.0, "small"),
                  ("P3-n63-pm1-len-nf1-wide", 3, 63, 1, False, 1.0, "wide"),
                  ("P4-n64-pm0-len-nf2-wide", 4, 64, 0, False, 2.0, "wide"),
                  ("P5-n65-pm1-bound-nf2-wide", 5, 65, 1, True, 2.0, "wide"),
                  ("P37-n129-pm0-bound-nf1-small", 37, 129, 0, True, 1.0, "small"),
                  ("P37-n65-pm1-len-nf1-wide", 37, 65, 1, False, 1.0, "wide"),
                  ("P5-n129-pm0-len-nf1-small", 5, 129, 0, False, 1.0, "small"),
                  ("P1-n65-pm1-bound-nf1-small", 1, 65, 1, True, 1.0, "small"))


def case_id(c):
    return c[0]


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def make_template(gen, P, search_kind):
    """pst [P,6] fp32, row 0 zero; "wide": the planted rows next, the random ones with s <= 1/3; "small": uniform in [-1, 1]"""
    pst = (2.0 * torch.rand(P, 6, generator=gen) - 1.0).numpy().astype(np.float32)
    if search_kind == "wide":
        pst[:, :3] *= np.float32(0.25)                                 # |r| <= (0.5, 0.25, 0.125): s <= 0.33
        for row, (_, vals) in enumerate(PLANTED[:P]):
            pst[row] = vals
    pst[0] = 0.0
    return pst


def make_lattice(gen, n):
    """camera directions [n,3] (z forward) and depths [n]: 0.5 .. 3.5, about one in nine <= 0 (exactly 0.0, -0.0, a negative)"""
    rays = (torch.randn(n, 3, generator=gen) * torch.tensor([0.6, 0.6, 0.2]) + torch.tensor([0.0, 0.0, 1.0])).numpy().astype(np.float32)
    td = (0.5 + 3.0 * torch.rand(n, generator=gen)).numpy().astype(np.float32)
    bad = np.arange(n)[4::9]
    td[bad] = np.array([0.0, -0.0, -1.5], np.float32)[np.arange(len(bad)) % 3]
    return rays, td


@functools.lru_cache(maxsize=None)
def particle_case(key):
    name, P, n, pm, use_bound, nf, kind = key
    gen = torch.Generator().manual_seed(_seed(name))
    cfg = place_cfg(1, 0, perturb=0, use_bound=use_bound, norm_factor=nf)
    state = make_state(gen, SEARCH_WIDE if kind == "wide" else SEARCH_SMALL)
    pst = make_template(gen, P, kind)
    rays, td = make_lattice(gen, n)
    planted = {pname: row for row, (pname, _) in enumerate(PLANTED[:P])} if kind == "wide" else {"identity": 0}
    return dict(name=name, P=P, n=n, point_major=pm, cfg=cfg, state=state, pst=pst, rays=rays, td=td, planted=planted)


# ---- fitness: (name, P, n, form): "raw10" (mipsf_ro_fitness, stride 10, SDF in column 3), "sdf-row" / "sdf-point" (mipsf_ro_fitness_sdf)
RAW_SENTINEL = np.float32(1.0e6)                                     # every column but the SDF's: it would show if read
FITNESS_CASES = (("P1-n1-raw10", 1, 1, "raw10", False), ("P3-n63-sdf-row", 3, 63, "sdf-row", False),
                 ("P4-n64-sdf-point", 4, 64, "sdf-point", False), ("P5-n65-raw10", 5, 65, "raw10", False),
                 ("P37-n129-sdf-point", 37, 129, "sdf-point", False), ("P37-n129-raw10", 37, 129, "raw10", False),
                 ("P5-n129-sdf-row", 5, 129, "sdf-row", False), ("P37-n65-sdf-row", 37, 65, "sdf-row", False),
                 ("P1-n65-sdf-point", 1, 65, "sdf-point", False), ("P3-n1-sdf-row", 3, 1, "sdf-row", False),
                 ("P5-n65-raw10-no-valid-depth", 5, 65, "raw10", True), ("P4-n129-sdf-point-no-valid-depth", 4, 129, "sdf-point", True))


@functools.lru_cache(maxsize=None)
def fitness_case(key):
    """sdf [P,n] fp32 of mixed sign, depths as make_lattice's (or none valid), and the buffer ``raw`` as the entry point takes it"""
    name, P, n, form, none_valid = key
    gen = torch.Generator().manual_seed(_seed(name))
    sdf = (0.4 * torch.randn(P, n, generator=gen)).numpy().astype(np.float32)
    _, td = make_lattice(gen, n)
    if none_valid:
        td = np.where(np.arange(n) % 3 == 0, np.float32(0.0), np.where(np.arange(n) % 3 == 1, np.float32(-0.0), -td)).astype(np.float32)
    if form == "raw10":
        raw = np.full((P * n, 10), RAW_SENTINEL, np.float32)
        raw[:, 3] = sdf.reshape(-1)
    else:
        raw = ordered(sdf, form == "sdf-point")
    return dict(name=name, P=P, n=n, form=form, sdf=sdf, td=td, raw=raw, trunc=TRUNC, none_valid=none_valid)


# ---- update: (name, P, kind)
UPDATE_CASES = tuple((f"P{P}-{kind}", P, kind) for P, kind in (
    (1, "lattice-none"), (2, "lattice-ties"), (255, "lattice-ties"), (256, "lattice-ties"), (257, "lattice-ties"), (1000, "lattice-ties"),
    (257, "lattice-none"), (257, "lattice-tail"), (1000, "lattice-tail"),
    (2, "generic"), (255, "generic"), (256, "generic"), (257, "generic"), (1000, "generic"), (256, "ill")))
LATTICE_J0 = 300                                                      # particle 0: mean_masked = 300 / 1024


def swarm_poses(gen, P):
    """pst7 [P,7] fp32 as the particle kernel's arithmetic leaves them (the yardstick's), from a random template at SEARCH_SMALL"""
    r, _, qw, _ = pose7(F, make_template(gen, P, "small"), SEARCH_SMALL)
    return np.concatenate([qw.v[:, None], r.v], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def update_case(key):
    """mean_masked [P], pst7 [P,7], state [32] fp32; ``expect``: what the case was planted for.

    Lattice: mean_masked = j / 1024, j < 16384: j * 1000 < 2^24, so mean_masked * 1000 is exact in fp32 and both formats decide
    f < f0 alike on every particle."""
    name, P, kind = key
    gen = torch.Generator().manual_seed(_seed(name))
    state = make_state(gen, SEARCH_SMALL)
    pst7 = swarm_poses(gen, P)
    expect = {}
    if kind.startswith("lattice"):
        j = LATTICE_J0 + torch.randint(-200, 201, (P,), generator=gen).numpy()
        j[0] = LATTICE_J0
        if kind == "lattice-ties":
            plan = [LATTICE_J0 - 1, LATTICE_J0, LATTICE_J0 + 1, LATTICE_J0, LATTICE_J0 - 1, LATTICE_J0 + 1]
            rows = [1] if P == 2 else [1, 2, 3, P - 3, P - 2, P - 1]
            for r, v in zip(rows, plan):
                j[r] = v
            expect = dict(ties=[r for r, v in zip(rows, plan) if v == LATTICE_J0], below=[r for r, v in zip(rows, plan) if v < LATTICE_J0],
                          above=[r for r, v in zip(rows, plan) if v > LATTICE_J0])
        elif kind == "lattice-none":
            j = np.maximum(j, LATTICE_J0)                            # ties and worse: nothing is advanced
            if P > 3:
                j[1], j[P - 1] = LATTICE_J0, LATTICE_J0
            expect = dict(advanced=[])
        elif kind == "lattice-tail":                                 # all advanced weight in the last partial stride of 256
            tail = np.arange(P) >= (P // 256) * 256
            j = np.where(tail, np.minimum(j, LATTICE_J0 - 1), np.maximum(j, LATTICE_J0))
            j[0] = LATTICE_J0
            expect = dict(advanced=list(np.nonzero(tail)[0]))
        assert j.max() < 16384 and j.min() > 0
        mm = (j.astype(np.float64) / 1024.0).astype(np.float32)
    elif kind == "generic":                                          # the size real rounds produce: a few 1e-2
        mm = (0.03 * (1.0 + 0.3 * torch.randn(P, generator=gen).clamp(-2.5, 2.5))).numpy().astype(np.float32)
        mm[0] = np.float32(0.033)
        if P == 2:
            mm[1] = np.float32(0.027)                                # the one other particle is advanced
    elif kind == "ill":                                              # the advanced ones beat particle 0 by about 1e-4 of its value
        u = torch.rand(P, generator=gen).numpy()
        better = np.arange(P) % 3 == 1
        mm = (0.03 * np.where(better, 1.0 - 1e-4 * (0.5 + u), 1.0 + 0.2 * u)).astype(np.float32)
        mm[0] = np.float32(0.03)
    else:
        raise ValueError(kind)
    return dict(name=name, P=P, kind=kind, mm=mm, pst7=pst7, state=state, rescale=RESCALE, expect=expect)


# ---- the order contract and the carry: an analytic SDF on the host, from the device's own xn
PLANE_N = np.array([0.36, -0.48, 0.8])                               # a unit normal along no axis
PLANE_D = 1.1


def plane_sdf(xn, cfg):
    """float64 [.., 3] normalised points -> the signed distance to the plane n . x = d in de-normalised (world) coordinates"""
    sub, div, nf = norm_consts(cfg)
    world = np.asarray(xn, dtype=np.float64) * nf * div + sub
    return world @ PLANE_N - PLANE_D
