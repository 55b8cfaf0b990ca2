"""float64 restatement of csrc/hashgrid.hip with a DERIVED error bound for every element (numpy only: no torch, no GPU).

The kernels' cell and fraction come from one fmaf and one subtraction, so `locate` below copies them bit for bit; everything
after that is a short chain of fp32 roundings over a sum.  `reference` evaluates every sum in float64 from the kernel's own
fp32 fraction and returns, beside each value, the sum A of the magnitudes of its terms.  An fp32 evaluation with k roundings
on its longest path is then within gamma_k * A of the float64 value (gamma_k = k u / (1 - k u), u = 2^-24; Higham, Accuracy
and Stability of Numerical Algorithms, Lemma 3.1), and the float64 value itself is within n * 2^-53 * A of the exact one.
No tolerance here is measured: each k is a count of roundings in the kernel's source, written as a sum with one comment per
term.  Where A is exactly zero the kernel's value has to be exactly zero.

The build keeps every multiply and add apart (csrc/Makefile: -ffp-contract=off), so `a + b * c` in the source is two roundings
and only an explicit fmaf is one.

Inputs stay clear of fp32 underflow (tests/test_hashgrid_fp64_cpu.py asserts that the smallest non-zero product is above
2^-100), so no bound needs an absolute floor.
"""
import dataclasses
import re
from fractions import Fraction

import numpy as np

U = 2.0 ** -24                   # unit roundoff of fp32
U64 = 2.0 ** -53                 # ... of float64
_U32 = np.uint64(0xFFFFFFFF)
P1, P2 = 2654435761, 805459861   # hashgrid.hip P1, P2



@dataclasses.dataclass(frozen=True)
class Build:
    """The compile-time constants of the routed scatter (hashgrid.hip) that decide what a record, a part and a rounding is.
    One instance per library build: DEFAULT is the shipped library, BUILDS[name] the variant `name` of csrc/variants.mk (the
    defaults with that variant's -D overrides; tests/test_hashgrid_fp64_cpu.py asserts that the two lists agree)."""
    max_slice: int = 8192            # MIPSF_SC_MAX_SLICE: a level of up to this many entries is one slice
    slice_log2: int = 13             # MIPSF_SC_SLICE_LOG2: slices of a larger level
    part: int = 24576                # MIPSF_SC_PART: records per work item, hashed level
    part_dense: int = 8192           # MIPSF_SC_PART_DENSE: ... dense level
    run: int = 4                     # MIPSF_SC_RUN: records merged in registers per thread on a dense level
    masked_max_m: int = 1 << 24      # MIPSF_SC_MASKED_MAX_M: up to this many samples a record carries its corner mask
    rt_block: int = 512              # MIPSF_RT_BLOCK: threads of a routing workgroup, SC_ROUTE_UNR = 4 samples each
    rt_levels: int = 1               # MIPSF_RT_LEVELS: levels routed by one workgroup
    stage_cap_words: int = 0         # MIPSF_SC_STAGE_CAP: records a routing workgroup stages per level (0: 10 * rt_block)
    skip_zero: int = 1               # MIPSF_SC_SKIP_ZERO: 0 = dead pairs get records too
    # switches that change how the kernels work and nothing a record, a part or a rounding count depends on
    route_fast: int = 1              # MIPSF_SC_ROUTE_FAST
    planar: int = 1                  # MIPSF_SC_PLANAR
    stage: int = 1                   # MIPSF_SC_STAGE
    agg_max: int = 1                 # MIPSF_SC_AGG_MAX
    publish_wt: int = 1              # MIPSF_SC_PUBLISH_WT

    @property
    def stage_cap(self):
        return self.stage_cap_words or 10 * self.rt_block

    @property
    def route_chunk(self):
        """consecutive samples of one routing workgroup (RT_BLOCK * SC_ROUTE_UNR)"""
        return 4 * self.rt_block

    def live(self, dout, n_levels=None):
        """[M,L] bool, the (sample, level) pairs scatter_route_kernel gives records, or None for all of them.
        MIPSF_SC_SKIP_ZERO = 0: the routing kernel is not shown dout at all.  MIPSF_RT_LEVELS > 1: a workgroup routes the
        levels group, group + G, group + 2 G, ... (G = ceil(L / RT_LEVELS)) from ONE liveness mask -- a sample is live when
        its gradient is non-zero on any of them -- so a pair that is dead by itself gets records through its group (they add
        exact zeros: the part counts move, the sums do not)."""
        if not self.skip_zero:
            return None
        live = live_pairs(dout)
        if self.rt_levels > 1:
            L = live.shape[1]
            G = (L + self.rt_levels - 1) // self.rt_levels
            for g in range(G):
                live[:, g::G] = live[:, g::G].any(1, keepdims=True)
        return live


# macro of csrc/variants.mk -> field of Build
BUILD_MACROS = {"MIPSF_SC_MAX_SLICE": "max_slice", "MIPSF_SC_SLICE_LOG2": "slice_log2", "MIPSF_SC_PART": "part",
                "MIPSF_SC_PART_DENSE": "part_dense", "MIPSF_SC_RUN": "run", "MIPSF_SC_MASKED_MAX_M": "masked_max_m",
                "MIPSF_RT_BLOCK": "rt_block", "MIPSF_RT_LEVELS": "rt_levels", "MIPSF_SC_STAGE_CAP": "stage_cap_words",
                "MIPSF_SC_SKIP_ZERO": "skip_zero", "MIPSF_SC_ROUTE_FAST": "route_fast", "MIPSF_SC_PLANAR": "planar",
                "MIPSF_SC_STAGE": "stage", "MIPSF_SC_AGG_MAX": "agg_max", "MIPSF_SC_PUBLISH_WT": "publish_wt"}
DEFAULT = Build()
BUILDS = {
    "maskless": Build(masked_max_m=1024),
    "small": Build(masked_max_m=1024, stage_cap_words=512, part=2048, part_dense=1024),
    "slice10": Build(max_slice=1024, slice_log2=10),
    "general": Build(route_fast=0),
    "rt2": Build(rt_levels=2),
    "rt4": Build(rt_levels=4),
    "interleaved": Build(planar=0),
    "nostage": Build(stage=0),
    "agg8": Build(agg_max=8),
    "fence": Build(publish_wt=0),
    "keepzero": Build(skip_zero=0),
    "run1": Build(run=1),
    "rtb256": Build(rt_block=256),
}
# the shipped library's, under the names the kernels use
SC_MAX_SLICE, SC_SLICE_LOG2, SC_PART, SC_PART_DENSE, SC_RUN = (DEFAULT.max_slice, DEFAULT.slice_log2, DEFAULT.part,
                                                               DEFAULT.part_dense, DEFAULT.run)
SC_MAX_NS, SC_MAX_BINS = 512, 8192     # hashgrid.hip: slices a level, bins a table (check_plan refuses more)


def parse_variants(text):
    """csrc/variants.mk -> {name: (unit, {macro: value})}"""
    names = re.findall(r"^VARIANTS\s*\+=\s*(\w+)\s*$", text, re.M)
    out = {}
    for name in names:
        unit = re.search(rf"^{name}_UNIT\s*=\s*(\w+)\s*$", text, re.M).group(1)
        flags = re.search(rf"^{name}_FLAGS\s*=\s*(.*)$", text, re.M).group(1).split()
        macros = {}
        for f in flags:
            m = re.fullmatch(r"-D(\w+)=(\d+)", f)
            assert m, f"variant {name}: flag {f} is not -DNAME=<integer>"
            macros[m.group(1)] = int(m.group(2))
        out[name] = (unit, macros)
    return out


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------- rounding counts
K_WEIGHT = (3      # corner_weights: `1.0f - cell.f[d]`, one per dimension
            + 2)   # corner_weights: `t = t * (...)`, twice (the first factor is taken as it is)
K_FWD = (K_WEIGHT
         + 8)      # hashgrid_fwd_kernel: `a0 = fmaf(w[c], v[c].x, a0)`, c = 0..7: corner 0's term passes through all 8
K_JAC = (2         # level_jacobian: `1.0f - cell.f[d0]`, `1.0f - cell.f[d1]`
         + 2       # level_jacobian: `wgt = wgt * (...)`, twice, starting from scale
         + 1       # level_jacobian: `v[right].x - v[left].x`
         + 1       # level_jacobian: `wgt * (...)`
         + 3)      # level_jacobian: `s0 = s0 + ...`, sub = 1..3 (sub = 0 adds to 0.f: exact)
K_DXL = (K_JAC
         + 1       # hashgrid_dx_kernel / hashgrid_dx_jac_kernel: `s0 * gy.x`, `s1 * gy.y`
         + 1)      # ... their sum
K_DX = (K_DXL
        + 15       # hashgrid_dx_reduce_kernel: `a += dxl[...]`, l = 1..15 (l = 0 adds to 0.f); dx_jac_kernel: `a[d] += ...`
        + 1)       # `dx[t] += a`
K_SCATTER = (K_WEIGHT
             + 1   # scatter_item: `wgt * gy.x`
             + 1)  # scatter_item: `(float)a.x` -- the fp64 slice sum leaves as fp32 (to dparams or to a partial slice)


def K_SCATTER_DENSE_RUN(build=DEFAULT):
    """scatter_item, dense level: `sum[c][0] = sum[c][0] + wgt * gy.x`, up to SC_RUN records per run, the first onto 0.0f"""
    return build.run - 1


# + (parts - 1): fold_entry `a.x += v[k].x` over the bin's parts in part order, eight loads at a time (the slots past the last part
#   hold 0.f: exact), the first onto 0.f; `cur.x += a.x` is exact onto the zero a fresh dparams holds.  An accumulate into
#   non-zero dparams rounds the RESULT once more: + u |value|.


class Levels:
    """The level table, from the ctypes GridMeta of mipsfusion_amd._lib or the oracle's dataclass."""

    def __init__(self, meta):
        self.n_levels = L = int(meta.n_levels)
        self.scales = np.array([meta.scales[l] for l in range(L)], dtype=np.float32)
        self.res = [int(meta.resolutions[l]) for l in range(L)]
        self.offsets = [int(meta.offsets[l]) for l in range(L + 1)]

    def size(self, level):
        return self.offsets[level + 1] - self.offsets[level]

    @property
    def n_entries(self):
        return self.offsets[-1]


def cut_offsets(offsets, level, size):
    """The offsets of a table whose `level` holds `size` entries; the later levels move up."""
    offsets = [int(o) for o in offsets]
    shift = size - (offsets[level + 1] - offsets[level])
    return offsets[:level + 1] + [o + shift for o in offsets[level + 1:]]


HAND_LEVEL, HAND_SIZE = 5, 12344      # the hand-made meta: level 5 of the 2^14 table (hashed, 16384) cut to 12344 = 8 * 1543


# ------------------------------------------------------------------------------------------------------------ cell and fraction
def fma32(a, x, c):
    """fl32(a * x + c) with ONE rounding.  -> (result, cases resolved exactly, cases left unresolved).
    a * x is exact in float64 (24 x 24 bits).  s = fl64(a x + c) rounds once; TwoSum gives its residual.  Where the residual is
    zero, fl32(s) is the single rounding.  Where it is not, s and the exact sum still lie on the same side of every fp32
    rounding boundary (the boundaries are float64 numbers) unless s IS a boundary: then the residual's sign decides."""
    p = np.float64(np.float32(a)) * x.astype(np.float64)
    c = np.float64(c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    back = r.astype(np.float64)
    away = np.where(s > back, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    other = np.nextafter(r, away).astype(np.float64)
    tie = (err != 0) & (s != back) & (2.0 * (s - back) == other - back)
    unresolved = int((~np.isfinite(s)).sum())
    resolved = 0
    for i in np.flatnonzero(tie):
        lo, hi = sorted((Fraction(float(back.flat[i])), Fraction(float(other.flat[i]))))
        exact = Fraction(float(p.flat[i])) + Fraction(float(c))
        r.flat[i] = np.float32(float(hi if exact > (lo + hi) / 2 else lo))     # (exact != the midpoint: err != 0)
        resolved += 1
    return r, resolved, unresolved


def locate(levels, x, level):
    """hashgrid.hip locate().  -> c [M,3] uint64 (holding uint32 values), f [M,3] fp32, (resolved, unresolved)"""
    pos, n_res, n_unres = fma32(levels.scales[level], x, 0.5)
    fl = np.floor(pos)
    n_unres += int((np.abs(fl) >= 2.0 ** 31).sum())            # (int)fl is undefined out there
    c = fl.astype(np.int64).astype(np.int32).view(np.uint32).astype(np.uint64)
    f = (pos - fl).astype(np.float32)                          # fp32 subtraction, as the kernel's
    return c, f, (n_res, n_unres)


def level_is_hashed(res, size):
    stride = 1
    for _ in range(3):
        if stride > size:
            break
        stride = (stride * res) & 0xFFFFFFFF
    return size < stride


def level_mode(res, size):
    """0: dense walk with wrap-around, then % size; 1: hash & (size - 1); 2: hash % size"""
    if not level_is_hashed(res, size):
        return 0
    return 1 if size & (size - 1) == 0 else 2


def corner_indices(c, res, size):
    """hashgrid.hip corner_index for the 8 corners.  c [M,3] uint64 -> [M,8] int64 entry index inside the level"""
    mode = level_mode(res, size)
    out = np.empty((c.shape[0], 8), dtype=np.int64)
    for k in range(8):
        cx = (c[:, 0] + np.uint64(k & 1)) & _U32
        cy = (c[:, 1] + np.uint64((k >> 1) & 1)) & _U32
        cz = (c[:, 2] + np.uint64((k >> 2) & 1)) & _U32
        if mode == 0:
            idx = (cx + cy * np.uint64(res) + cz * np.uint64(res * res)) & _U32      # < 2^55 before the mask
            idx = idx % np.uint64(size)
        else:
            h = cx ^ ((cy * np.uint64(P1)) & _U32) ^ ((cz * np.uint64(P2)) & _U32)
            idx = (h & np.uint64(size - 1)) if mode == 1 else (h % np.uint64(size))
        out[:, k] = idx.astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------------------------ the answer
def reference(levels, x, params, dout=None):
    """x [M,3] fp32, params [2 * entries] fp32, dout [M,L,2] fp32 (None: forward and Jacobian only).  float64 throughout.
    -> dict: idx [M,L,8]; y, A_y [M,L,2]; J, A_J [M,L,3,2]; dxl, A_dxl [M,L,3]; dx, A_dx [M,3];
       entries [E] (global entry numbers, ascending: every entry a corner lands on), dp, A_dp [E,2], n_dp [E];
       min_product (smallest non-zero |w g| and |w scale dv|), fma (resolved, unresolved), modes (set of addressing modes)"""
    M, L = x.shape[0], levels.n_levels
    table = params.astype(np.float64).reshape(-1, 2)
    R = dict(idx=np.empty((M, L, 8), np.int64), f=np.empty((M, L, 3), np.float32), c=np.empty((M, L, 3), np.uint64),
             y=np.empty((M, L, 2)), A_y=np.empty((M, L, 2)), J=np.empty((M, L, 3, 2)), A_J=np.empty((M, L, 3, 2)),
             modes=set())
    if dout is not None:
        g_all = dout.astype(np.float64)
        R.update(dxl=np.empty((M, L, 3)), A_dxl=np.empty((M, L, 3)))
        ent, val, mag = [], [], []
    n_res = n_unres = 0
    min_product = np.inf
    for level in range(L):
        off, size, res = levels.offsets[level], levels.size(level), levels.res[level]
        scale = np.float64(levels.scales[level])
        c, f32, (a, b) = locate(levels, x, level)
        n_res, n_unres = n_res + a, n_unres + b
        idx = corner_indices(c, res, size)
        R["modes"].add(level_mode(res, size))
        f = f32.astype(np.float64)
        omf = 1.0 - f
        w = np.empty((M, 8))
        for k in range(8):
            w[:, k] = ((f[:, 0] if k & 1 else omf[:, 0]) * (f[:, 1] if k & 2 else omf[:, 1])) * (f[:, 2] if k & 4 else omf[:, 2])
        v = table[off + idx]                                               # [M,8,2]
        R["idx"][:, level], R["f"][:, level], R["c"][:, level] = idx, f32, c
        R["y"][:, level] = (w[:, :, None] * v).sum(1)
        R["A_y"][:, level] = (w[:, :, None] * np.abs(v)).sum(1)
        for d in range(3):
            d0, d1 = (1 if d == 0 else 0), (1 if d == 2 else 2)
            J, A = np.zeros((M, 2)), np.zeros((M, 2))
            for sub in range(4):
                b0, b1 = sub & 1, (sub >> 1) & 1
                wo = (f[:, d0] if b0 else omf[:, d0]) * (f[:, d1] if b1 else omf[:, d1])
                left = (b0 << d0) | (b1 << d1)
                dv = v[:, left | (1 << d)] - v[:, left]
                J += wo[:, None] * dv
                A += wo[:, None] * np.abs(dv)
                t = np.abs(scale * wo[:, None] * dv)
                if (t > 0).any():
                    min_product = min(min_product, float(t[t > 0].min()))
            R["J"][:, level, d], R["A_J"][:, level, d] = scale * J, scale * A
        if dout is not None:
            g = g_all[:, level]                                            # [M,2]
            R["dxl"][:, level] = (R["J"][:, level] * g[:, None, :]).sum(-1)
            R["A_dxl"][:, level] = (R["A_J"][:, level] * np.abs(g)[:, None, :]).sum(-1)
            wg = w[:, :, None] * g[:, None, :]                             # [M,8,2]
            t = np.abs(wg)
            if (t > 0).any():
                min_product = min(min_product, float(t[t > 0].min()))
            ent.append((off + idx).ravel())
            val.append(wg.reshape(-1, 2))
            mag.append(t.reshape(-1, 2))
    R["fma"], R["min_product"] = (n_res, n_unres), min_product
    if dout is not None:
        R["dx"], R["A_dx"] = R["dxl"].sum(1), R["A_dxl"].sum(1)
        ent, val, mag = np.concatenate(ent), np.concatenate(val), np.concatenate(mag)
        entries, inv = np.unique(ent, return_inverse=True)
        E = entries.size
        R["entries"] = entries
        R["dp"] = np.stack([np.bincount(inv, val[:, k], E) for k in range(2)], 1)
        R["A_dp"] = np.stack([np.bincount(inv, mag[:, k], E) for k in range(2)], 1)
        R["n_dp"] = np.bincount(inv, minlength=E)
    return R


# ------------------------------------------------------------------------------------------------------------------ the bounds
# the float64 side: the weight is three float64 products of rounded 1 - f (6 roundings), each sum has n terms
def bound_y(R):
    return (gamma(K_FWD) + (6 + 8) * U64) * R["A_y"]


def bound_J(R):
    return (gamma(K_JAC) + (6 + 5) * U64) * R["A_J"]


def bound_dxl(R):
    return (gamma(K_DXL) + (6 + 5 + 3) * U64) * R["A_dxl"]


def bound_dx(R, L):
    return (gamma(K_DX) + (6 + 5 + 3 + L) * U64) * R["A_dx"]


def _slices(levels, level, build):
    """-> (slices of the level, the shift that takes an entry index to its slice)"""
    size = levels.size(level)
    if size <= build.max_slice:
        return 1, 31
    return (size + (1 << build.slice_log2) - 1) >> build.slice_log2, build.slice_log2


def scatter_plan(levels, R, live=None, build=DEFAULT):
    """The records and parts of every bin of the routed scatter (hashgrid.hip make_plan, scatter_route_kernel, part_of).
    live [M,L] bool: the (sample, level) pairs that get records (None: all, as after mipsf_hashgrid_route, which sees no dout);
    for a build other than the shipped one it is build.live(dout).
    A record is a sample with at least one corner in the bin's slice.
    -> list per level of dict(dense, shift, records [slices], parts [slices])"""
    plan = []
    for level in range(levels.n_levels):
        size = levels.size(level)
        ns, shift = _slices(levels, level, build)
        idx = R["idx"][:, level]
        if live is not None:
            idx = idx[live[:, level]]
        sl = idx >> shift                                                  # [m,8]
        key = np.unique(np.arange(sl.shape[0])[:, None] * ns + sl)         # distinct (sample, slice)
        records = np.bincount(key % ns, minlength=ns)
        dense = not level_is_hashed(levels.res[level], size)
        part = build.part_dense if dense else build.part
        plan.append(dict(dense=dense, shift=shift, records=records, parts=(records + part - 1) // part))
    return plan


def route_chunk_records(levels, R, live=None, build=DEFAULT):
    """[chunks, L]: the records one routing workgroup makes on one level (scatter_route_kernel: a workgroup takes
    RT_BLOCK * SC_ROUTE_UNR consecutive samples; the records past MIPSF_SC_STAGE_CAP leave by the lane-per-record store)."""
    M = R["idx"].shape[0]
    chunk = build.route_chunk
    n_chunks = (M + chunk - 1) // chunk
    out = np.zeros((n_chunks, levels.n_levels), np.int64)
    for level in range(levels.n_levels):
        ns, shift = _slices(levels, level, build)
        sample = np.arange(M) if live is None else np.flatnonzero(live[:, level])
        sl = R["idx"][sample, level] >> shift
        key = np.unique(sample[:, None] * ns + sl)                         # distinct (sample, slice)
        out[:, level] = np.bincount((key // ns) // chunk, minlength=n_chunks)
    return out


def live_pairs(dout):
    """scatter_route_kernel: a pair is dead when both feature gradients are zero (-0 included)"""
    return ~((dout[..., 0] == 0) & (dout[..., 1] == 0))


def roundings_dp(levels, R, plan, build=DEFAULT):
    """[E]: fp32 roundings on the longest path of every entry's sum, routed scatter into a dparams that is zero on entry"""
    entries = R["entries"]
    level = np.searchsorted(np.asarray(levels.offsets), entries, side="right") - 1
    k = np.empty(entries.size)
    for l in range(levels.n_levels):
        m = level == l
        parts = plan[l]["parts"][(entries[m] - levels.offsets[l]) >> plan[l]["shift"]]
        k[m] = K_SCATTER + (K_SCATTER_DENSE_RUN(build) if plan[l]["dense"] else 0) + np.maximum(parts, 1) - 1
    return k


def bound_dp(levels, R, plan, build=DEFAULT):
    """[E,2]: the routed scatter into a dparams that is zero on entry; plan = scatter_plan(..., build)"""
    k = roundings_dp(levels, R, plan, build)
    # float64 side: the weight (6), the product, the reference's n-term sum; the kernel's fp64 LDS atomics: n more
    return (gamma(k) + (7 + 2 * R["n_dp"]) * U64)[:, None] * R["A_dp"]


def worst_ratio(got, want, bound):
    """-> (largest error / bound over the elements with a non-zero bound, elements with a zero bound that are not exactly 0)"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want), np.asarray(bound)
    err = np.abs(got - want)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if not np.isfinite(got).all():
        ratio = np.inf
    return ratio, int(np.count_nonzero(got[~pos]))


# ------------------------------------------------------------------------------------------------------------------- the inputs
X_LO, X_HI = -1.5, 2.5           # the range real rays reach (decoder_cpu.X_LO, X_HI; this module imports no torch)


def build_inputs(levels, M, seed, dead_share=0.3, outside=False):
    """-> x [M,3], params [2 * entries], dout [M,L,2] (fp32), kinds {name: sample indices planted}.
    dead_share: about this share of the (sample, level) pairs carries a zero gradient (ray tails, whole samples, single pairs).
    outside: x is drawn over [X_LO, X_HI]^3, as the samples of real rays are -- three points in four lie outside the unit box, on
    negative cells and on cells past the level's resolution, whose corners wrap (the planted kinds stay as they are)."""
    rng = np.random.default_rng(seed)
    L = levels.n_levels
    sc = levels.scales.astype(np.float64)
    x = rng.random((M, 3)).astype(np.float32)
    if outside:
        x = (np.float32(X_LO) + np.float32(X_HI - X_LO) * x).astype(np.float32)
    else:
        x = np.clip(x, np.float32(1e-3), np.float32(1 - 1e-3))              # the interior
    kinds = {}
    taken = np.zeros(M, bool)
    if M >= 128:                                                            # 64 consecutive samples of one ray
        ray = np.arange(32, 96)
        t = (np.arange(64) / 160.0)[:, None]
        x[ray] = (np.array([0.11, 0.23, 0.37]) + t * np.array([0.6, 0.64, 0.48])).astype(np.float32)
        kinds["ray"] = ray
        taken[ray] = True
    if M >= 63:
        k = max(1, M // 32)
        pool = rng.permutation(np.flatnonzero(~taken))
        cursor = 0

        def take(name, n=k):
            nonlocal cursor
            ids = pool[cursor:cursor + n]
            cursor += n
            kinds[name] = ids
            return ids, np.arange(ids.size), rng.integers(0, 3, ids.size)

        ids, r, ax = take("near_low")
        x[ids, ax] = (-rng.uniform(1e-4, 0.1, ids.size)).astype(np.float32)
        ids, r, ax = take("near_high")
        x[ids, ax] = (1.0 + rng.uniform(1e-4, 0.1, ids.size)).astype(np.float32)
        ids, r, ax = take("far")
        x[ids] = rng.uniform(-4, 4, (ids.size, 3)).astype(np.float32)
        x[ids, ax] = (rng.choice([-1.0, 1.0], ids.size) * rng.uniform(2, 4, ids.size)).astype(np.float32)
        ids, r, ax = take("cell_minus1")                                    # pos in [-1, 0) on level lv: c = (uint32)-1
        lv = rng.integers(0, L, ids.size)
        x[ids, ax] = (-(0.5 + rng.uniform(0.05, 0.95, ids.size)) / sc[lv]).astype(np.float32)
        ids, r, ax = take("exact01")
        x[ids, ax] = (r % 2).astype(np.float32)
        ids, r, ax = take("face")                                           # on a cell face of level 1 (dense) or 4 (hashed)
        lv = np.where(r % 2 == 0, 1, min(4, L - 1))
        kk = rng.integers(1, np.asarray(levels.res)[lv] - 1)
        x[ids, ax] = ((kk - 0.5) / sc[lv]).astype(np.float32)
        ids, r, ax = take("crowded", max(k, 4))                             # one cell of the finest level
        c0 = np.floor(sc[L - 1] * np.array([0.61803, 0.31415, 0.27182]) + 0.5)
        x[ids] = ((c0 + rng.uniform(0.1, 0.9, (ids.size, 3)) - 0.5) / sc[L - 1]).astype(np.float32)
        ids, r, ax = take("duplicate")
        src = pool[(np.arange(ids.size) * 7) % max(1, cursor - ids.size)]  # copies of samples planted above
        x[ids] = x[src]
        kinds["duplicate_of"] = src
    params = (rng.choice([-1.0, 1.0], 2 * levels.n_entries) * 2.0 ** rng.uniform(-20, 0, 2 * levels.n_entries)).astype(np.float32)
    dout = (rng.choice([-1.0, 1.0], (M, L, 2)) * 2.0 ** rng.uniform(-30, 10, (M, L, 2))).astype(np.float32)
    s = dead_share / 3.0
    if M >= 63:
        n_groups = (M + 31) // 32
        tails = rng.random(n_groups) < min(1.0, s * 32 / 8.5)
        tails[0] = True
        for gi in np.flatnonzero(tails):                                    # dead ray tails (a ray: 32 consecutive samples)
            end = min(M, 32 * gi + 32)
            dout[max(32 * gi, end - int(rng.integers(1, 17))):end] = 0
        whole = rng.random(M) < s
        whole[M // 2] = True
        dout[whole] = 0                                                     # dead whole samples
    pair = rng.random((M, L)) < s
    one = rng.random((M, L)) < 0.1
    if M > 1:
        pair[0, 3 % L] = True
        one[M - 1, 5 % L] = True
    dout[pair] = 0                                                          # dead (sample, level) pairs
    feat = rng.integers(0, 2, (M, L))
    dout[one, feat[one]] = 0                                                # one feature of a pair exactly zero
    return np.ascontiguousarray(x), params, np.ascontiguousarray(dout), kinds


# the routed-scatter cases of tests/test_gpu_hashgrid_fp64.py: (name, table, M, dead_share, what the part counts must show)
#   table: log2 of the hashmap size, or "hand" for the hand-made meta
SCATTER_CASES = [
    ("t14_m9000", 14, 9000, 0.01, "dense bins in two parts, ragged second slice of level 2"),
    ("t10_m25000", 10, 25000, 0.01, "every (hashed, one-slice) bin in two parts"),
    ("t14_m25000", 14, 25000, 0.01, "dense one-slice bins in four parts"),
    ("t19_m3000", 19, 3000, 0.3, "64 slices per hashed level"),
    ("hand_m3000", "hand", 3000, 0.3, "a hashed level of 12344 entries: % addressing, two slices"),
    ("t14_m1", 14, 1, 0.3, "one sample"),
]
FWD_M = [1, 63, 64, 65, 255, 256, 257, 9000]
# points over [X_LO, X_HI]^3 (build_inputs(outside=True)): (table, M) -- a 2^16 and a 2^19 table, and the hand-made meta for the
# % addressing; every kernel form runs them in both layouts, under the same derived bounds
OUTSIDE_CASES = [(16, 257), (19, 130), ("hand", 257)]
# the two sides of the `maskless` variant's limit (MIPSF_SC_MASKED_MAX_M = 1024): 1024 samples still carry corner masks
MASK_EDGE_CASES = [
    ("t14_m1024", 14, 1024, 0.3, "the last batch size whose records carry the corner mask"),
    ("t14_m1025", 14, 1025, 0.3, "the first batch size whose records are bare sample indices"),
]
# the cases every variant library of csrc/variants.mk runs (tests/test_gpu_hashgrid_variants.py), and what
# tests/test_hashgrid_fp64_cpu.py shows them to reach
VARIANT_CASES = {
    "maskless": ["t14_m9000", "t10_m25000", "t19_m3000", "hand_m3000", "t14_m1024", "t14_m1025"],
    "small": ["t14_m25000", "t10_m25000"],
    "slice10": ["t19_m3000", "hand_m3000", "t14_m9000"],
    **{v: ["t14_m9000", "t19_m3000", "hand_m3000", "t14_m1"] for v in ("general", "nostage", "agg8", "interleaved", "rtb256")},
    **{v: ["t14_m9000", "t19_m3000"] for v in ("rt2", "rt4", "keepzero")},
    **{v: ["t14_m25000", "t10_m25000"] for v in ("fence", "run1")},
}
CASES_BY_NAME = {c[0]: c for c in SCATTER_CASES + MASK_EDGE_CASES}
