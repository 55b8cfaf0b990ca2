"""Inputs and the float64 answer for the decoder kernels (csrc/decoder.hip, csrc/decoder16.hip, csrc/wgrad16.hip,
csrc/decoder_dev.h): MLP_reg.forward written out layer by layer, and its backward written out by hand, in plain torch on the host,
parameterised by dtype.  float64 is the answer; float32 (``e32``) is the yardstick: how far plain fp32 arithmetic lands from
float64 on the same inputs.  No tests here and no GPU: tests/test_decoder_cpu.py holds this helper to its conditions (among them:
the forward equals oracle/path_cpu.decoder_forward and the backward equals autograd through it, to 1e-12),
tests/test_gpu_decoder_fp64.py holds the kernels to it.

Encoding.  The argument is formed in fp32 exactly as the kernels form it, fma(ldexp(x_d, k), pi_f, s * pi_f / 2)
(step_cpu.freq_args); the sine is taken in the working dtype, its derivative is (2^k pi_f) * cos(arg).  The yardstick takes the
float64 sine and cosine rounded once to fp32 (what a correctly rounded fp32 sine gives).

Normalisations (``errors``).  Outputs: absolute error over the group's scale (rgb: the batch's largest float64 |rgb|; sdf: 1;
entropy: log2 5; prob: 1).  dfeat, dx, dembed_pos: every row divided by that row's max |dout| (the kernel's and the reference's
alike), then the absolute error over the largest such normalised float64 magnitude of the live rows: without the division the
samples with a small incoming gradient -- it spans e^-16 .. e^-6 -- are never looked at.  A row whose max |dout| lies below
fp32's smallest normal number is divided by that number instead (FLT_MIN, as render_cpu counts such entries): its gradients are
subnormal fp32 numbers, which hold 2^-149 absolutely and no relative precision, in any fp32 arithmetic.  Parameter gradients: per
tensor, absolute error over the tensor's largest float64 magnitude.  Each group has a largest and an rms error.

Gates (``gates``).  (a) the largest error <= min(max(GATE_FACTOR * e32_max, GATE_FLOOR, extra_max), ceiling); (b) the rms error <=
max(GATE_FACTOR * e32_rms, extra_rms).  GATE_FACTOR, GATE_FLOOR and the ceilings are render_cpu's.  (a) catches a wrong element,
tile or index, (b) an arithmetic one class worse than fp32.  ``extra`` is the allowance for the hardware sine and cosine, from the
reference alone: the float64 restatement evaluated a second time with every encoding entry moved by E_SIN * s and every cosine by
E_COS * s (s a fixed seeded +-1 pattern); 4 times the per-group largest and rms change (4: a random sign pattern gives the
typical effect, not the worst case).  ``extra`` is never below the result's own rounding to fp32, 2^-24 of each float64 entry
under the same normalisation (``_reference``): it matters only where the yardstick is exact, a batch of one sample.  For the
parameter gradients it is never below ``summation_floor`` either: the least error of an fp32 sum of the samples' terms.

Threshold samples.  A sample some float64 pre-activation of H1 or G3 of which is below 1e-5 in magnitude may take the other side
of the ReLU in any finite arithmetic: it gets dout = 0 (its forward outputs are still compared).  Their share is at most 3 % per
case, and none of the planted live samples is among them (one that would be gets other inputs).  ``pick_seed`` takes the first
seed from SEEDS' on for which these float64 conditions hold.  SEEDS itself was chosen by hand where seed 1 left the fp32
yardstick less than its headroom; that headroom (e32_max < GATE_FLOOR / 4, tests/test_decoder_cpu.py) is a figure of the host's
fp32 sums and so depends on the host, the inputs do not."""
import functools
import math

import numpy as np
import torch

from mipsfusion_amd import ops
from mipsfusion_amd.model import MLP_reg
from oracle import tcnn_cpu

from . import step_cpu
from .render_cpu import CEIL_GRAD, CEIL_VALUE, FLT_MIN, GATE_FACTOR, GATE_FLOOR

N_FREQ, N_PE, N_FEAT, N_SDF_EMB, N_CLASS = 8, 48, 32, 64, 5
X_LO, X_HI = -1.5, 2.5                 # the range real rays reach
THRESHOLD = 1e-5                       # the margin of test_decoder_true_error_of_every_arithmetic_against_fp64
THRESHOLD_SHARE = 0.03
F16_TOL = 2e-3                         # plain f16, forward only: the tolerance the project states for it
EXTRA_FACTOR = 4.0
U = 2.0 ** -24                        # one fp32 rounding

# The largest error of the kernels' own sine / cosine (decoder_dev.h sin_reduced / cos_reduced: a two-piece reduction to
# revolutions, then v_sin_f32 / v_cos_f32) against the float64 sine / cosine of the fp32 argument, x in [-1.5, 2.5], all 48
# entries: TWICE the largest error measured on an MI355X (tests/test_gpu_decoder_fp64.py::test_encoding_* measure it again
# and assert it stays below these).  Measured: sine 2.44e-07 for f32 and bf16x6, 2.55e-07 for f16x3 (the largest: the constant
# is twice it; the f16x3 assertion has 2^-21 |e| more for its 22-bit operands), cosine 2.56e-07 (all three).  A correctly
# rounded fp32 sine is 3.0e-08 off.
E_SIN = 2 * 2.55e-07
E_COS = 2 * 2.56e-07

SMALL_MS = (1, 31, 32, 33, 127, 128, 129, 4096 + 17)
VARIANTS = ("base", "feat1e-4", "subnormal")
OUT_GROUPS = (("rgb", slice(0, 3)), ("sdf", slice(3, 4)), ("entropy", slice(4, 5)), ("prob", slice(5, 10)))
OUT_NAMES = tuple(n for n, _ in OUT_GROUPS)
ROW_NAMES = ("dfeat", "dx", "dembed_pos")


def large_ms(cu_count):
    """P - 32: the last size on the small-batch kernels; P: the first on the persistent ones (16 wave tiles of 32 samples for
    every CU); P + 33: a full tile and a ragged one more"""
    P = cu_count * 16 * 32
    return (P - 32, P, P + 33)


def tile_edge_ms(cu_count):
    """Both weight-gradient kernels launch min(tiles, T) workgroups, T = min(CU count, 256) (WG_MAX_BLOCKS / W16_MAX_BLOCKS).  The
    streaming kernel (wgrad16.hip) counts 32-sample tiles: 32 T - 31 gives T tiles, the last one ragged; 32 T + 1 gives T + 1,
    so one workgroup takes two.  The LDS kernel (decoder.hip) counts 128-sample block tiles: 128 T + 1 is the same edge for it
    (T + 1 block tiles, the last one a single sample)."""
    T = min(cu_count, 256)
    return (32 * T - 31, 32 * T + 1, 128 * T + 1)


def form_cases(cu_count):
    """[(M, variant)]: where the further weight-gradient forms of tests/test_gpu_decoder_fp64.py (BWD_FORMS2) run -- the smallest
    sizes at which they can go wrong: one tile and a sample, four tiles and a sample (also with subnormal rows), more tiles than
    the small-batch chain has waves, the workgroup-count edges, and the persistent chain with a ragged tile"""
    return ([(33, "base"), (129, "base"), (129, "subnormal"), (4096 + 17, "base")]
            + [(M, "base") for M in tile_edge_ms(cu_count)] + [(large_ms(cu_count)[2], "base")])


def live_tiles(dout):
    """the 32-sample tiles with a non-zero incoming gradient, ascending: what the backward chain appends to its live-tile lists
    (decoder16.hip tl_append: tile t goes to list (t >> 3) & 7)"""
    M = dout.shape[0]
    live = torch.cat([(dout != 0).any(1), torch.zeros((-M) % 32, dtype=torch.bool)])
    return live.view(-1, 32).any(1).nonzero()[:, 0]


# ------------------------------------------------------------------------------------------------------- encoding
def freq_scale(dtype):
    """[8] 2^k pi_f (exact in fp32)"""
    return (torch.exp2(torch.arange(N_FREQ, dtype=torch.float32)) * np.float32(tcnn_cpu.PI_F32)).to(dtype)


def signs(shape, seed):
    return (2.0 * torch.randint(0, 2, shape, generator=torch.Generator().manual_seed(seed)) - 1.0).double()


def encoding(x32, dtype, shift_sin=0.0, shift_cos=0.0):
    """-> pe [M,48] (entry d * 16 + 2 k + s), dpe_dx [M,3,8,2] = (2^k pi_f) cos(arg) in ``dtype``.  float64: sine and cosine of
    the fp32 argument in float64; float32: those rounded once.  shift_*: every sine / cosine moved by shift * (a fixed +-1)."""
    assert x32.dtype == torch.float32
    arg = step_cpu.freq_args(x32, N_FREQ).double()
    sin, cos = torch.sin(arg), torch.cos(arg)
    if shift_sin:
        sin = sin + shift_sin * signs(sin.shape, 4801)
    if shift_cos:
        cos = cos + shift_cos * signs(cos.shape, 4802)
    sin, cos = sin.to(dtype), cos.to(dtype)
    return sin.reshape(x32.shape[0], N_PE), freq_scale(dtype)[None, None, :, None] * cos


# -------------------------------------------------------------------------------------------------------- forward
def forward(weights, feat, x, pe):
    """MLP_reg.forward (model/decoder.py) in the dtype of its inputs -> out [M,10] = rgb(3) sdf entropy prob(5), and what the
    backward needs: e, the pre-activations H1, H2, G3 and prob"""
    w0, b0, w2, b2, wr, br, ws0, bs0, ws2, bs2 = weights
    e = torch.cat([x, pe], 1)                                     # [M,51]
    H1 = e @ w0.T + b0
    H2 = torch.relu(H1) @ w2.T + b2                               # sdf_emb = H2[:, :64], rgb_emb = H2[:, 64:]
    rgb = torch.cat([H2[:, N_SDF_EMB:], e], 1) @ wr.T + br
    G3 = torch.cat([H2[:, :N_SDF_EMB], feat], 1) @ ws0.T + bs0
    logits = torch.relu(G3) @ ws2.T + bs2
    z = logits - logits.max(1, keepdim=True).values
    p = torch.exp(z)
    p = p / p.sum(1, keepdim=True)
    entropy = -(p * torch.log2(p + 1e-5)).sum(1, keepdim=True)
    ids = torch.arange(N_CLASS, dtype=p.dtype)
    sdf = ((p * ids).sum(1, keepdim=True) / (N_CLASS - 1) - 0.5) * 2
    return dict(out=torch.cat([rgb, sdf, entropy, p], 1), e=e, H1=H1, H2=H2, G3=G3, prob=p)


# ------------------------------------------------------------------------------------------------------- backward
def backward(weights, feat, fwd, dpe_dx, dout, term_norms=False, cut=None):
    """by hand from dout [M,10] -> dfeat [M,32], dx_direct [M,3] (through e's first three columns), dembed_pos [M,48], dx (direct
    plus the path through the encoding) and the ten parameter gradients in ops.DECODER_PARAM_ORDER.  cut = (kind, pieces): the
    gradients CUTS[kind] names are formed from operands cut to ``pieces`` bf16 pieces (``cut_product``), still in float64"""
    w0, b0, w2, b2, wr, br, ws0, bs0, ws2, bs2 = weights
    e, H1, H2, G3, p = fwd["e"], fwd["H1"], fwd["H2"], fwd["G3"], fwd["prob"]
    M = e.shape[0]
    drgb, dsdf, dent, dp = dout[:, :3], dout[:, 3:4], dout[:, 4:5], dout[:, 5:]
    ids = torch.arange(N_CLASS, dtype=p.dtype)
    # sdf = sum(p ids) / 2 - 1;  entropy = -sum p log2(p + eps): d / dp = -(log2(p + eps) + p / ((p + eps) ln 2))
    dp = dp + dsdf * (ids * (2.0 / (N_CLASS - 1)))[None] - dent * (torch.log2(p + 1e-5) + p / ((p + 1e-5) * math.log(2.0)))
    dlogits = p * (dp - (dp * p).sum(1, keepdim=True))
    A3 = torch.relu(G3)
    g_ws2, g_bs2 = dlogits.T @ A3, dlogits.sum(0)
    dG3 = (dlogits @ ws2) * (G3 > 0).to(p.dtype)
    g_ws0, g_bs0 = dG3.T @ torch.cat([H2[:, :N_SDF_EMB], feat], 1), dG3.sum(0)
    dcat = dG3 @ ws0
    dfeat = dcat[:, N_SDF_EMB:]
    g_wr, g_br = drgb.T @ torch.cat([H2[:, N_SDF_EMB:], e], 1), drgb.sum(0)
    dcr = drgb @ wr
    dH2 = torch.cat([dcat[:, :N_SDF_EMB], dcr[:, :N_SDF_EMB]], 1)
    g_w2, g_b2 = dH2.T @ torch.relu(H1), dH2.sum(0)
    dH1 = (dH2 @ w2) * (H1 > 0).to(p.dtype)
    g_w0, g_b0 = dH1.T @ e, dH1.sum(0)
    de = dcr[:, N_SDF_EMB:] + dH1 @ w0
    dx_direct, dpe = de[:, :3], de[:, 3:]
    dx = dx_direct + (dpe.reshape(M, 3, N_FREQ, 2) * dpe_dx).sum((-1, -2))
    res = dict(dfeat=dfeat, dx_direct=dx_direct, dembed_pos=dpe, dx=dx,
               grads=[g_w0, g_b0, g_w2, g_b2, g_wr, g_br, g_ws0, g_bs0, g_ws2, g_bs2])
    # every parameter gradient is d^T a (a = None: a bias, the column sums of d), in ops.DECODER_PARAM_ORDER
    pairs = [(dH1, e), (dH1, None), (dH2, torch.relu(H1)), (dH2, None), (drgb, torch.cat([H2[:, N_SDF_EMB:], e], 1)), (drgb, None),
             (dG3, torch.cat([H2[:, :N_SDF_EMB], feat], 1)), (dG3, None), (dlogits, A3), (dlogits, None)]
    if cut is not None:
        kind, pieces = cut
        for i, n_cut in CUTS[kind].items():
            res["grads"][i] = cut_product(*pairs[i], pieces) if n_cut else res["grads"][i]
    if term_norms:
        # sqrt(sum_i t_i^2) of every entry's sum over the samples, t_i = d[i, j] a[i, k] (a = 1 for a bias): ``summation_floor``;
        # sum_i |t_i|, the magnitude a relative error of every term is applied to: ``two_plane_bound``
        sq = lambda d, a=None: ((d * d).T @ (a * a) if a is not None else (d * d).sum(0)).sqrt()      # noqa: E731
        ab = lambda d, a=None: (d.abs().T @ a.abs() if a is not None else d.abs().sum(0))              # noqa: E731
        res["term_norms"] = [sq(d, a) for d, a in pairs]
        res["term_abs"] = [ab(d, a) for d, a in pairs]
    return res


# ------------------------------------------------------------------------------------- the two-plane bf16 arithmetics
# Which parameter gradients (index in ops.DECODER_PARAM_ORDER) a two-plane arithmetic forms from cut operands, and how many of
# a term's factors are cut (2: both, the gradient and the activation; 1: the gradient alone -- a bias), read in the kernels:
#
#   "lds"     wgrad_precision="bf16x3", decoder.hip decoder_wgrad_kernel<.., BF16X3 = true>: wgrad_mma_bf16 runs the three LARGE
#             products -- sdf0: dG3^T [sdf_emb | grid], pts2: dH2^T relu(H1), pts0: dG1^T [e | ones] -- and split8_bf16 cuts BOTH
#             operands as they come out of LDS: hi = (__bf16)v, lo = (__bf16)(v - (float)hi), both conversions round to nearest
#             even; per k-step hi hi + hi lo + lo hi, the lo lo pair is dropped; fp32 accumulators.  The ones row of the pts0
#             phase makes column 51 of that product d pts_linears.0.bias: it IS a cut product, with 1.0 (exact in bf16, lo = 0)
#             as its second factor.  The two small heads (wgrad_mma_small, fp32-input MFMA) and the other four biases (row_sum in
#             fp32, the ones column of the small product) are not cut.
#   "stream"  wgrad_precision="stream_bf16x3", wgrad16.hip ArBF2 (P = 2), the streaming form w16_role_a / w16_role_b: next_plane
#             cuts EVERY block it transposes -- the five gradient blocks (dH2, dG3, dG1 and the small rows d logits | d rgb) in
#             transpose_block, the five activation blocks (H1, H3, sdf_emb | grid, rgb_emb, e) in transpose_mac -- into plane 0 =
#             bf16(r) (v_cvt_pk_bf16_f32, round to nearest even), r -= plane 0 (exact in fp32), plane 1 = bf16(r); the products
#             keep the plane pairs pa + pb <= 1, again hi hi + hi lo + lo hi.  All five bias gradients are the row sums of the
#             TRANSPOSED PLANES of their gradient block (transpose_block<A, SUM = true>): hi + lo, one cut factor.  So here the
#             small heads and every bias go through the cut as well.
CUTS = {"lds": {0: 2, 1: 1, 2: 2, 6: 2},
        "stream": {0: 2, 1: 1, 2: 2, 3: 1, 4: 2, 5: 1, 6: 2, 7: 1, 8: 2, 9: 1}}
U_BF16 = 2.0 ** -8                     # bf16 keeps 8 significant bits: round to nearest is within 2^-8 of the value
# two pieces: |v - hi| <= 2^-8 |v|, lo = bf16(v - hi) is within 2^-8 of THAT: v = (hi + lo)(1 + d), |d| <= 2^-16
CUT_ONE = U_BF16 ** 2
# both factors cut and the lo lo pair dropped: (a_hi + a_lo)(b_hi + b_lo) - a_lo b_lo; the first is a b (1 + d_a)(1 + d_b), and
# |a_lo| <= 2^-8 (1 + 2^-8) |a|: a term is within (2 * 2^-16 + 2^-32 + 2^-16 (1 + 2^-8)^2) |a b|, 3.008 * 2^-16
CUT_BOTH = 2 * CUT_ONE + CUT_ONE ** 2 + (U_BF16 * (1 + U_BF16)) ** 2


def bf16_pieces(v, pieces):
    """-> (hi, lo) float64: the fp32 value of ``v`` (what the records hold) as the kernels cut it: hi = bf16(v), lo = bf16(v - hi)
    (the difference is exact in fp32), both round to nearest even; pieces = 1: lo = 0"""
    v32 = v.float()
    hi = v32.to(torch.bfloat16).float()
    lo = (v32 - hi).to(torch.bfloat16).float() if pieces == 2 else torch.zeros_like(hi)
    return hi.double(), lo.double()


def cut_product(d, a, pieces):
    """d^T a (a None: the column sums of d) in float64 from operands cut to ``pieces`` bf16 pieces, the lo lo pair dropped"""
    dh, dl = bf16_pieces(d, pieces)
    if a is None:
        return (dh + dl).sum(0)
    ah, al = bf16_pieces(a, pieces)
    return dh.T @ ah + dh.T @ al + dl.T @ ah


def two_plane_bound(ref, kind):
    """{parameter name: (bound [like the gradient], bound on the rms)} for the gradients ``kind`` ("lds" / "stream", CUTS) forms
    from cut operands, on the error over the tensor's largest float64 magnitude (``errors``' normalisation); the other
    gradients keep ``gates``.

    Per element: a cut term is within c |t_i| of the float64 term (c = CUT_BOTH for a weight, CUT_ONE for a bias, derived
    above from the two roundings to nearest of the cut), so the sum of the cut terms is within c A of the float64 sum, A = sum_i
    |t_i| in float64 (``backward(term_norms=True)``: term_abs) -- a worst-case bound, as tests/hashgrid_cpu.py's gamma(k) A.
    What the kernel does besides -- the fp32 record it cuts, the fp32 accumulators, the reduce -- is the fp32 arithmetic the
    existing gate (a) allows for, and is added: bound = c A / max |r64| + gate (a).  The rms over the tensor: the two parts'
    rms add (the triangle inequality): rms(c A / max |r64|) + gate (b)."""
    out = {}
    for i, n_cut in CUTS[kind].items():
        name, g = ops.DECODER_PARAM_ORDER[i], ref["r64"]["grads"][i]
        top = float(g.abs().max())
        part = (CUT_BOTH if n_cut == 2 else CUT_ONE) * ref["term_abs"][i] / (top if top > 0 else 1.0)
        g_max, g_rms = gates(name, ref["e32"][name], ref["extra"][name])
        out[name] = (part + g_max, float(part.pow(2).mean().sqrt()) + g_rms)
    return out


def two_plane_errors(grads, ref, kind):
    """{name: dict(share: the largest error / bound over the elements, where, max: the error there, bound: the bound there,
    rms, rms_bound)} of the ten ``grads`` for the gradients ``kind`` cuts"""
    out = {}
    for name, (bound, rms_bound) in two_plane_bound(ref, kind).items():
        i = ops.DECODER_PARAM_ORDER.index(name)
        r = ref["r64"]["grads"][i]
        top = float(r.abs().max())
        err = (grads[i].double() - r).abs() / (top if top > 0 else 1.0)
        share = (err / bound).reshape(-1)
        w = int(torch.argmax(share))
        out[name] = dict(share=float(share[w]), where=w, max=float(err.reshape(-1)[w]), bound=float(bound.reshape(-1)[w]),
                         rms=float(err.pow(2).mean().sqrt()), rms_bound=rms_bound)
    return out


def evaluate(weights32, feat32, x32, dout32, dtype, *, external=False, shift_sin=0.0, shift_cos=0.0, term_norms=False, cut=None):
    """forward and backward in ``dtype`` from the fp32 inputs.  external: the encoding is an INPUT, the fp32 tensor
    ``embed_pos(x32)`` (MLP_reg's embed_pos argument), and dx is the direct path alone -- what the kernels return then."""
    if external:
        pe = embed_pos(x32).to(dtype)
        dpe_dx = torch.zeros(x32.shape[0], 3, N_FREQ, 2, dtype=dtype)
    else:
        pe, dpe_dx = encoding(x32, dtype, shift_sin, shift_cos)
    w = [t.to(dtype) for t in weights32]
    fwd = forward(w, feat32.to(dtype), x32.to(dtype), pe)
    res = dict(out=fwd["out"], H1=fwd["H1"], H2=fwd["H2"], G3=fwd["G3"])
    if dout32 is not None:
        res.update(backward(w, feat32.to(dtype), fwd, dpe_dx, dout32.to(dtype), term_norms, cut))
    return res


def embed_pos(x32):
    """the fp32 encoding a caller hands to the external-encoding form: the float64 sine rounded once"""
    return encoding(x32, torch.float32)[0]


# ---------------------------------------------------------------------------------------------------------- cases
def make_weights(seed):
    """MLP_reg's own initialisation, sdf_linear.2.weight times 4 (as the parity tests use) -> 10 fp32 tensors"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        dec = MLP_reg({}, input_ch=N_FEAT, input_ch_pos=N_PE)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    sd["sdf_linear.2.weight"] *= 4.0
    return [sd[k] for k in ops.DECODER_PARAM_ORDER]


X_SPECIAL = (0.0, -0.0, 0.5, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -20, -1.5, 2.5)
TOP_SCALE = math.exp(-6.0)


def planted_live(M):
    """the samples a kernel is likeliest to drop or misplace: those of the last, partial 32-sample tile, the first and the last
    of the batch, the first of every 128-sample block"""
    idx = {0, M - 1} | set(range(0, M, 128))
    if M % 32:
        idx |= set(range(M - M % 32, M))
    return torch.tensor(sorted(idx))


def on_threshold(H1, G3):
    return (H1.abs().min(1).values < THRESHOLD) | (G3.abs().min(1).values < THRESHOLD)


def _make_case(M, seed, variant):
    gen = torch.Generator().manual_seed(7919 * seed + M)
    weights = make_weights(seed)
    x = torch.rand(M, 3, generator=gen) * (X_HI - X_LO) + X_LO
    flat = x.reshape(-1)
    n = min(flat.numel(), len(X_SPECIAL))
    flat[:n] = torch.tensor(X_SPECIAL[:n])
    feat = torch.randn(M, N_FEAT, generator=gen) * (1e-4 if variant == "feat1e-4" else 0.3)     # 1e-4: tcnn's initial scale
    dout = torch.randn(M, 10, generator=gen) * torch.exp(torch.rand(M, 1, generator=gen) * 10.0 - 16.0)
    s = torch.arange(M)
    n_rays = (M + 63) // 64
    tail = torch.randint(10, 60, (n_rays,), generator=gen)
    tail[0] = 10 + int(tail[0]) % 23                             # the first ray's tail starts in its first tile: tile 1 is zero
    dout[::7] = 0.0                                              # single samples inside live tiles
    dout[(s % 64) >= tail.repeat_interleave(64)[:M]] = 0.0       # the tail of every 64-sample ray from a random position
    dout[(s // 64) % 5 == 3] = 0.0                               # one ray in five throughout
    live = planted_live(M)
    dout[live] = torch.randn(live.numel(), 10, generator=gen) * TOP_SCALE
    r64 = evaluate(weights, feat, x, None, torch.float64)
    thr = on_threshold(r64["H1"], r64["G3"])
    # a planted sample must be live, so it must not sit on a threshold: such a one gets other inputs (its features, and its point
    # unless it is one of the rows that hold X_SPECIAL).  1 % of the samples sit on one, and a large batch plants a thousand.
    for _ in range(8):
        bad = live[thr[live]]
        if bad.numel() == 0:
            break
        feat[bad] = torch.randn(bad.numel(), N_FEAT, generator=gen) * (1e-4 if variant == "feat1e-4" else 0.3)
        free = bad[bad >= 3]
        x[free] = torch.rand(free.numel(), 3, generator=gen) * (X_HI - X_LO) + X_LO
        rb = evaluate(weights, feat[bad], x[bad], None, torch.float64)
        thr[bad] = on_threshold(rb["H1"], rb["G3"])
    dout[thr] = 0.0
    subnormal = torch.zeros(0, dtype=torch.long)
    if variant == "subnormal":
        ok = (dout != 0).any(1)
        ok[live] = False
        subnormal = (ok & (s % 17 == 5)).nonzero()[:6, 0]
        dout[subnormal] = torch.randn(subnormal.numel(), 10, generator=gen) * 1e-41
    return dict(M=M, seed=seed, variant=variant, weights=weights, x=x, feat=feat, dout=dout, threshold=thr, planted=live,
                subnormal=subnormal)


def case_ok(c):
    return float(c["threshold"].double().mean()) <= THRESHOLD_SHARE and not bool(c["threshold"][c["planted"]].any())


def zero_tiles(dout):
    """(#full 32-sample tiles whose dout is zero throughout, #tiles with zero rows and live rows)"""
    M = dout.shape[0]
    dead = (dout == 0).all(1)
    pad = torch.cat([dead, torch.ones((-M) % 32, dtype=torch.bool)]).view(-1, 32)
    real = torch.cat([torch.ones(M, dtype=torch.bool), torch.zeros((-M) % 32, dtype=torch.bool)]).view(-1, 32)
    full = real.all(1)
    n_dead, n_real = (pad & real).sum(1), real.sum(1)
    return int(((n_dead == 32) & full).sum()), int(((n_dead > 0) & (n_dead < n_real)).sum())


# --------------------------------------------------------------------------------------------------------- errors
def _stat(err, rows=None):
    """largest, rms and the place of the largest of an error array (rows: the sample index of each of its rows)"""
    if err.numel() == 0:
        return dict(max=0.0, rms=0.0, where=-1)
    flat = int(torch.argmax(err))
    row = flat // (err.numel() // err.shape[0])
    return dict(max=float(err.reshape(-1)[flat]), rms=float(err.pow(2).mean().sqrt()), where=int(rows[row]) if rows is not None else flat)


def row_scale(dout):
    return dout.double().abs().max(1).values.clamp_min(FLT_MIN)


def errors(res, r64, dout, names=None, normal_rows_only=False):
    """{group: dict(max, rms, where)} of ``res`` (a kernel's results, the yardstick's or the perturbed answer's: tensors on the
    host, any float dtype) against the float64 answer, under this module's normalisations.  Groups: the four output groups,
    "dfeat", "dx", "dembed_pos" and the ten parameter names, as far as ``res`` has them (or ``names`` lists them).
    normal_rows_only: the rows whose incoming gradient is subnormal throughout are left out of the row groups."""
    out = {}
    have = lambda k: k in res and res[k] is not None and (names is None or k in names)      # noqa: E731
    if have("out"):
        a, r = res["out"].double(), r64["out"]
        for name, sl in OUT_GROUPS:
            scale = {"rgb": float(r[:, :3].abs().max()), "sdf": 1.0, "entropy": math.log2(N_CLASS), "prob": 1.0}[name]
            out[name] = _stat((a[:, sl] - r[:, sl]).abs() / scale, torch.arange(r.shape[0]))
    if dout is not None:
        top_dout = dout.abs().max(1).values
        live = (top_dout >= FLT_MIN if normal_rows_only else top_dout > 0).nonzero()[:, 0]
        rs = row_scale(dout)[live, None]
        for name in ROW_NAMES:
            if have(name):
                a, r = res[name].double()[live] / rs, r64[name][live] / rs
                top = float(r.abs().max()) if r.numel() else 1.0
                out[name] = _stat((a - r).abs() / top, live)
    if have("grads"):
        for name, a, r in zip(ops.DECODER_PARAM_ORDER, res["grads"], r64["grads"]):
            top = float(r.abs().max())
            out[name] = _stat((a.double() - r).abs() / (top if top > 0 else 1.0))
    return out


def gates(name, e32, extra=None):
    """-> (gate on the largest error, gate on the rms error) of a group"""
    ceiling = CEIL_VALUE if name in OUT_NAMES else CEIL_GRAD
    x_max, x_rms = (extra["max"], extra["rms"]) if extra is not None else (0.0, 0.0)
    return min(max(GATE_FACTOR * e32["max"], GATE_FLOOR, x_max), ceiling), max(GATE_FACTOR * e32["rms"], x_rms)


def summation_floor(r64):
    """{parameter name: dict(max, rms)}: what a sum over the samples costs in fp32 at the least, from float64 alone.

    Every parameter gradient is a sum over the M samples of terms t_i = d[i, j] a[i, k] whose signs differ, so the sum is far
    smaller than the terms' total magnitude -- for the biases (3 and 5 entries of a sum of up to 131 k terms) by two orders.  An
    arithmetic that does no more than round every TERM once to fp32 and then adds exactly is sqrt(sum_i (2^-24 t_i)^2) = 2^-24
    sqrt(sum_i t_i^2) off (independent roundings); every real fp32 sum also rounds its partial sums and is further off: the
    yardstick measures 2 - 5 times this.  The yardstick's own figure e32_rms, though, is ONE draw of that error, over 3 or 5
    numbers for the bias tensors, and the draw depends on the order in which the host's torch happens to add (a factor of 3
    between two builds on the same inputs).  Gate (b) is GATE_FACTOR times the error of an fp32-class arithmetic; this term keeps
    it from falling below GATE_FACTOR times the least such error when the draw is a lucky one:

        GATE_FACTOR * 2^-24 * sqrt(sum_i t_i^2) / max |r64|      per entry; its largest and its rms over the tensor.

    It never exceeds 8 times what the yardstick typically measures, and the largest-error gate (a) is not moved by it where the
    term is below GATE_FLOOR (everywhere in the cases of this module: tests/test_decoder_cpu.py asserts it)."""
    out = {}
    for name, g, n in zip(ops.DECODER_PARAM_ORDER, r64["grads"], r64["term_norms"]):
        top = float(g.abs().max())
        t = GATE_FACTOR * U * n / (top if top > 0 else 1.0)
        out[name] = dict(max=float(t.max()), rms=float(t.pow(2).mean().sqrt()))
    return out


@functools.lru_cache(maxsize=6)
def _reference(M, seed, variant, external):
    c = _make_case(M, seed, variant)
    args = (c["weights"], c["feat"], c["x"], c["dout"])
    r64 = evaluate(*args, torch.float64, external=external, term_norms=True)
    r32 = evaluate(*args, torch.float32, external=external)
    e32 = errors(r32, r64, c["dout"])
    e32_normal = errors(r32, r64, c["dout"], normal_rows_only=True) if c["subnormal"].numel() else e32
    if external:
        extra, flips = {k: dict(max=0.0, rms=0.0, where=-1) for k in e32}, 0
    else:
        rp = evaluate(*args, torch.float64, shift_sin=E_SIN, shift_cos=E_COS)
        extra = {k: dict(max=EXTRA_FACTOR * v["max"], rms=EXTRA_FACTOR * v["rms"], where=v["where"])
                 for k, v in errors(rp, r64, c["dout"]).items()}
        moved = ((rp["H1"] > 0) != (r64["H1"] > 0)).any(1) | ((rp["G3"] > 0) != (r64["G3"] > 0)).any(1)
        flips = int((moved & (c["dout"] != 0).any(1)).sum())
    # The result's own rounding: a kernel hands over fp32 numbers, so each entry r carries up to 2^-24 |r| whatever the arithmetic
    # in front of it.  The yardstick carries it too and 8 e32 covers it -- except where the yardstick is EXACT: the bias
    # gradients of a batch of one sample are that sample's dout, an input (e32 = 0, and gate (b) would be 0).  From float64
    # alone: the errors of r64 * (1 + 2^-24) under the same normalisations; the larger of it and the encoding's allowance.
    rounding = errors({k: ([g * (1.0 + U) for g in v] if k == "grads" else v * (1.0 + U)) for k, v in r64.items()
                       if k not in ("term_norms", "term_abs")},
                      r64, c["dout"])
    extra = {k: dict(max=max(v["max"], rounding[k]["max"]), rms=max(v["rms"], rounding[k]["rms"]), where=v["where"])
             for k, v in extra.items()}
    for k, v in summation_floor(r64).items():
        extra[k] = dict(max=max(extra[k]["max"], v["max"]), rms=max(extra[k]["rms"], v["rms"]), where=extra[k]["where"])
    # (the pre-activations of a large case are 400 MB: what a report needs of them is each sample's distance from a threshold)
    margin = torch.minimum(r64["H1"].abs().min(1).values, r64["G3"].abs().min(1).values)
    term_abs = r64["term_abs"]
    r64 = {k: v for k, v in r64.items() if k not in ("H1", "H2", "G3", "term_norms", "term_abs")}
    return dict(case=c, r64=r64, e32=e32, e32_normal=e32_normal, extra=extra, flips=flips, margin=margin, term_abs=term_abs)


# The seed of a size's cases, chosen by hand where seed 1 left the fp32 yardstick less than its headroom on the host this was
# written on (a cancelling bias gradient of a few samples).  A fixed table, so every machine builds the same inputs;
# tests/test_decoder_cpu.py asserts the headroom for every case, and that assertion is the host's fp32 figure.
# 32769 (128 * 256 + 1, tile_edge_ms): seed 1 puts the summation floor of pts_linear.2.weight at 4.25e-6, above GATE_FLOOR, and gate
# (a) is to stay at GATE_FLOOR in every case (a float64 figure; tests/test_decoder_cpu.py asserts it).
SEEDS = {31: 2, 32: 2, 33: 2, 32769: 2}


@functools.lru_cache(maxsize=None)
def pick_seed(M, variant="base"):
    """SEEDS' seed (1 for the other sizes), or the first after it whose case meets the float64 conditions on the inputs: the
    threshold share, the planted samples live.  Nothing measured in fp32 enters here."""
    first = SEEDS.get(M, 1)
    for seed in range(first, first + 16):
        if case_ok(_make_case(M, seed, variant)):
            return seed
    raise AssertionError(f"no seed gives a case M = {M} ({variant}) within the conditions on the inputs")


def case(M, variant="base"):
    """-> dict: fp32 ``weights`` (10, ops.DECODER_PARAM_ORDER), ``x`` [M,3], ``feat`` [M,32] (AoS), ``dout`` [M,10]; ``threshold``
    [M] bool, ``planted`` (indices), ``subnormal`` (indices of the rows that are subnormal throughout)"""
    return reference(M, variant)["case"]


def reference(M, variant="base", external=False):
    """-> dict: ``case``, ``r64`` (the answer), ``e32`` (the yardstick's errors; ``e32_normal``: without the subnormal rows),
    ``extra`` (the allowance for the hardware sine and cosine: EXTRA_FACTOR times the change of the answer under the shifted
    encoding, and at least the result's own rounding -- that alone for the external form, whose encoding is an input), ``flips`` (live samples whose ReLU pattern changes under
    the shift), ``margin`` [M] (each sample's smallest float64 |pre-activation| of H1 and G3), ``term_abs`` (per parameter gradient
    the float64 sum over the samples of its terms' magnitudes: ``two_plane_bound``)"""
    return _reference(M, pick_seed(M, variant), variant, external)
