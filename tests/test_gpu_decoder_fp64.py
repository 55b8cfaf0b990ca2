"""GPU (-m gpu): the decoder kernels (csrc/decoder.hip, csrc/decoder16.hip, csrc/wgrad16.hip, csrc/decoder_dev.h) against the
float64 restatement of tests/decoder_cpu.py (tests/test_decoder_cpu.py holds it, its inputs and its yardstick to their
conditions), through ops.* and so through ctypes and the C ABI, at ragged sizes:

  encoding    the kernels' own sine and cosine (sin_reduced / cos_reduced: a two-piece reduction to revolutions and the hardware
              sine) read out of the kernels: one-hot rows of rgb_linear.0.weight with zero bias make out[:, :3] three encoding
              entries, a dout of 1 in one rgb column makes dx the cosine times 2^k pi_f.  Against the float64 sine / cosine of
              the fp32 argument, under decoder_cpu.E_SIN / E_COS (twice the largest error measured).
  forward     f32 with the in-kernel and with the external encoding, bf16x6, f16x3, plain f16; AoS and level-major features;
              every size; every output group; the SDF-only entry against column 3 of the same answer.
  backward    f32 chain with f32 weight gradients (both encoding forms; the external one checks dembed_pos), bf16x6 and f16x3
              as JointEncoding runs them (lean records, recompute_h1, the ops switches at their defaults) and with the full
              records and every short cut off, the streaming kernels with deterministic=True, a frozen decoder (masks-only
              record, grads=None): dfeat, dx and all ten parameter gradients, each under both gates; exact zeros where
              float64 is zero; the rows that are subnormal throughout finite and under the same gates.
  further     every other weight-gradient form ops.decoder_bwd offers (BWD_FORMS2), each under the same check: the fp32 LDS kernel
  forms       behind either 16-bit chain (f16x3+f32w, bf16x6+f32w); the streaming kernels behind the fp32 chain and record
              (f32+stream_f16x3, f32+stream_bf16x6) and behind the other family's chain (f16x3+stream_bf16x6); the exchange form
              reading a FULL record with recompute_h1 (-full-rc); the lean activation record with the full gradient record
              (-lean-fulldact, LEAN_DACT off); the exchange form on the live-tile lists (-lists, COMPACT_LIVE off), with the
              ordered lists of deterministic=True (-det-lists: the only way into tile_lists_order_kernel; two calls give the same
              bytes in all ten gradients) and with a frozen decoder (f16x3-frozen-lists); the two-plane bf16 arithmetics
              (bf16x3 behind the f16x3 and the f32 chain, stream_bf16x3), whose cut gradients are held element by element to
              decoder_cpu.two_plane_bound (the operand cut's error on the float64 sum of the term magnitudes, plus the fp32 gate)
              and the others to the gates.  What ops.decoder_bwd refuses is asserted to be refused.

Sizes: 1, 31, 32, 33, 127, 128, 129, 4113 on the small-batch kernels; with P = CU count * 16 * 32: P - 32 (the last size on
them), P (the first on the persistent kernels) and P + 33 (a full tile and a ragged one more).  With T = min(CU count, 256), the
workgroups of both weight-gradient kernels: 32 T - 31 (T tiles, the last ragged) and 32 T + 1 (T + 1 tiles: one workgroup takes
two) on the three default forms and every further form; 128 T + 1 (the same edge in the 128-sample block tiles of the LDS kernel)
on the forms that run it.  The further forms run at 33, 129 (also with subnormal rows), 4113, these edges, and P + 33 behind a
16-bit chain.

Gates per group (decoder_cpu.gates): the largest error <= min(max(8 e32_max, 64 * 2^-24, extra_max), ceiling) and the rms error
<= max(8 e32_rms, extra_rms), extra holding the floors derived in decoder_cpu (the hardware sine, the result's rounding, the
least error of an fp32 sum over the samples); plain f16 (forward only): 2e-3 of the group's scale.  No outlier allowance.

Measured on an MI355X (worst group per form and size, kernel error | e32): see DESIGN.md, "The decoder kernels against
float64"."""
import math

import pytest
import torch

from mipsfusion_amd import _lib, ops

from . import decoder_cpu as D

pytestmark = pytest.mark.gpu

LAYOUTS = ("aos", "level_major")
LARGE_KEYS = ("P-32", "P", "P+33")
EDGE_KEYS = ("32T-31", "32T+1", "128T+1")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def size_of(key):
    if key in LARGE_KEYS:
        return D.large_ms(_lib.lib().mipsf_device_cu_count())[LARGE_KEYS.index(key)]
    if key in EDGE_KEYS:
        return D.tile_edge_ms(_lib.lib().mipsf_device_cu_count())[EDGE_KEYS.index(key)]
    return key


def report(form, tag, name, err, e32):
    print(f"\n  fp64 | {form} | {tag} | {name} | kernel {err:.2e} | e32 {e32:.2e}", end="")


def to_layout(feat_aos, layout):
    M = feat_aos.shape[0]
    return feat_aos.contiguous() if layout == "aos" else feat_aos.view(M, 16, 2).permute(1, 0, 2).contiguous()


def from_layout(t, layout, M):
    return t.reshape(M, 32) if layout == "aos" else t.view(16, M, 2).permute(1, 0, 2).reshape(M, 32)


def lay_id(layout):
    return _lib.FEAT_AOS if layout == "aos" else _lib.FEAT_LEVEL_MAJOR


class Held:
    """the inputs of a case on the device, with the operand images of the three arithmetics"""

    def __init__(self, dev, c, layout, weights=None):
        self.M, self.layout, self.lay = c["M"], layout, lay_id(layout)
        self.ws = [w.to(dev) for w in (weights if weights is not None else c["weights"])]
        self.x = c["x"].to(dev)
        self.feat = to_layout(c["feat"].to(dev), layout)
        self.dout = c["dout"].to(dev)
        self._packed = {}

    def packed(self, prec):
        fam = {"f32": "f32", "f16": "f16x3", "f16x3": "f16x3", "bf16x6": "bf16x6"}[prec]
        if fam not in self._packed:
            self._packed[fam] = ops.decoder_pack(self.ws) if fam == "f32" else ops.decoder_pack16(self.ws, precision=fam)
        return self._packed[fam]

    def fwd(self, prec, save=False, embed_pos=None):
        if prec == "f32":
            return ops.decoder_fwd(self.packed("f32"), self.feat, self.lay, self.x, embed_pos, self.M, save=save)
        return ops.decoder_fwd(None, self.feat, self.lay, self.x, None, self.M, save=save, precision=prec, packed16=self.packed(prec))


def check(form, tag, res, ref, f16=False, cut=None):
    """every group of ``res`` (host tensors) under both gates; exact zeros where float64 is zero; everything finite.  cut ("lds" /
    "stream"): the parameter gradients that two-plane arithmetic forms from cut operands are held, element by element and in
    the rms, to decoder_cpu.two_plane_bound instead"""
    c, r64 = ref["case"], ref["r64"]
    for name in ("out",) + D.ROW_NAMES:
        if res.get(name) is not None:
            a = res[name]
            assert bool(torch.isfinite(a).all()), f"{form} {tag}: {name} is not finite"
            if name != "out":
                zero = r64[name] == 0
                assert bool((a[zero] == 0).all()), \
                    f"{form} {tag}: {int((a[zero] != 0).sum())} entries of {name} are not 0.0 where the float64 answer is exactly 0"
    if res.get("grads") is not None:
        for name, a, r in zip(ops.DECODER_PARAM_ORDER, res["grads"], r64["grads"]):
            assert bool(torch.isfinite(a).all()), f"{form} {tag}: d {name} is not finite"
            assert bool((a[r == 0] == 0).all()), f"{form} {tag}: d {name} is not 0.0 where the float64 answer is exactly 0"
    err = D.errors(res, r64, c["dout"] if any(res.get(k) is not None for k in D.ROW_NAMES) else None)
    worst, failed = None, []
    two_plane = D.two_plane_errors(res["grads"], ref, cut) if cut is not None else {}
    for name, v in two_plane.items():
        ratio = max(v["share"], v["rms"] / v["rms_bound"])
        if worst is None or ratio > worst[0]:
            worst = (ratio, name + " (two-plane bound)", v["max"], ref["e32"][name]["max"])
        if v["share"] > 1.0 or v["rms"] > v["rms_bound"]:
            failed.append(f"{name}: element {v['where']} off by {v['max']:.3e}, {v['share']:.2f} of its two-plane bound {v['bound']:.2e}; "
                          f"rms {v['rms']:.3e} (bound {v['rms_bound']:.2e})")
    for name, v in err.items():
        if name in two_plane:
            continue
        e32, extra = ref["e32"][name], ref["extra"][name]
        g_max, g_rms = (D.F16_TOL, math.inf) if f16 else D.gates(name, e32, extra)
        ratio = max(v["max"] / g_max, (v["rms"] / g_rms) if g_rms > 0 else (0.0 if v["rms"] == 0 else math.inf))
        if worst is None or ratio > worst[0]:
            worst = (ratio, name, v["max"], e32["max"])
        if v["max"] > g_max or v["rms"] > g_rms:
            where = v["where"]
            place = (f"sample {where} (tile {where // 32}, |pre-activation| >= {float(ref['margin'][where]):.2e})"
                     if name in D.OUT_NAMES + D.ROW_NAMES else f"element {where}")
            failed.append(f"{name}: largest {v['max']:.3e} (gate {g_max:.2e}, e32 {e32['max']:.2e}, extra {extra['max']:.2e}) at {place}; "
                          f"rms {v['rms']:.3e} (gate {g_rms:.2e}, e32 {e32['rms']:.2e})")
    if two_plane:
        name, v = max(two_plane.items(), key=lambda kv: kv[1]["share"])
        print(f"\n  fp64 | {form} | {tag} | two-plane: {name} element {v['where']} error {v['max']:.2e} | bound {v['bound']:.2e} | "
              f"share {v['share']:.2f}", end="")
    report(form, tag, f"{worst[1]} at {worst[0]:.2f} of its gate", worst[2], worst[3])
    assert not failed, f"{form} {tag}:\n  " + "\n  ".join(failed)


# ============================================================================================================== encoding
ENC_PRECISIONS = ("f32", "bf16x6", "f16x3")


def encoding_points():
    """the x of the M = 129 case and a sweep of 4096 points over [-1.5, 2.5] in every coordinate (each in another order)"""
    sweep = torch.linspace(D.X_LO, D.X_HI, 4096)
    gen = torch.Generator().manual_seed(4096)
    cols = [sweep] + [sweep[torch.randperm(4096, generator=gen)] for _ in range(2)]
    return torch.cat([D.case(129)["x"], torch.stack(cols, 1)]).contiguous()


def encoding_case():
    x = encoding_points()
    M = x.shape[0]
    c = dict(D.case(129))
    gen = torch.Generator().manual_seed(M)
    c.update(M=M, x=x, feat=torch.randn(M, D.N_FEAT, generator=gen) * 0.3, dout=torch.zeros(M, 10))
    return c


def one_hot_rgb(weights, columns):
    """the case's weights with rgb_linear.0.weight = rows that select ``columns`` (one of e's 51 per rgb output) and zero bias"""
    ws = [w.clone() for w in weights]
    ws[4] = torch.zeros(3, 115)
    for j, col in enumerate(columns):
        ws[4][j, 64 + col] = 1.0
    ws[5] = torch.zeros(3)
    return ws


@pytest.mark.parametrize("prec", ENC_PRECISIONS)
def test_encoding_sine_of_the_kernels(dev, prec):
    c = encoding_case()
    M = c["M"]
    pe = torch.empty(M, D.N_PE, dtype=torch.float64)
    for i in range(16):
        h = Held(dev, c, "aos", one_hot_rgb(c["weights"], [3 + 3 * i + j for j in range(3)]))
        out, _ = h.fwd(prec)
        pe[:, 3 * i:3 * i + 3] = out[:, :3].cpu().double()
    want, _ = D.encoding(c["x"], torch.float64)
    err = (pe - want).abs()
    allow = D.E_SIN + (2.0 ** -21 * want.abs() if prec == "f16x3" else 0.0)
    i = int(torch.argmax(err))
    report("encoding", prec, f"sine, entry {i % D.N_PE} at x = {float(c['x'][i // D.N_PE, (i % D.N_PE) // 16])!r}", float(err.max()), 2.0 ** -25)
    assert bool((err <= allow).all()), f"{prec}: the kernels' sine is off by {float(err.max()):.3e} (E_SIN {D.E_SIN:.2e})"


@pytest.mark.parametrize("prec", ENC_PRECISIONS)
def test_encoding_cosine_of_the_kernels(dev, prec):
    c = encoding_case()
    M = c["M"]
    c["dout"][:, 0] = 1.0
    scale = D.freq_scale(torch.float64)
    cos = torch.empty(M, 3, D.N_FREQ, 2, dtype=torch.float64)
    for k in range(D.N_FREQ):
        for s in range(2):
            h = Held(dev, c, "aos", one_hot_rgb(c["weights"], []))
            h.ws[4][0, 64 + 3 + 2 * k + s::16] = 1.0                    # entry (d, k, s) of every coordinate d -> rgb column 0
            assert int(h.ws[4].count_nonzero()) == 3
            out, saved = h.fwd(prec, save=True if prec == "f32" else "masks")
            if prec == "f32":
                _, dx, _ = ops.decoder_bwd(h.packed("f32"), h.feat, h.lay, h.x, None, out, h.dout, saved, None, M)
            else:
                _, dx, _ = ops.decoder_bwd(None, h.feat, h.lay, h.x, None, out, h.dout, saved, None, M, precision=prec,
                                           packed16=h.packed(prec))
            cos[:, :, k, s] = dx.cpu().double() / scale[k]
    arg = D.step_cpu.freq_args(c["x"], D.N_FREQ).double()
    want = torch.cos(arg)
    err = (cos - want).abs()
    allow = D.E_COS + (2.0 ** -21 * want.abs() if prec == "f16x3" else 0.0)
    report("encoding", prec, "cosine (dx / (2^k pi_f))", float(err.max()), 2.0 ** -25)
    assert bool((err <= allow).all()), f"{prec}: the kernels' cosine is off by {float(err.max()):.3e} (E_COS {D.E_COS:.2e})"


# =============================================================================================================== forward
FWD_FORMS = ("f32", "f32-ext", "bf16x6", "f16x3", "f16")
FWD_RUNS = ([(M, v) for M in D.SMALL_MS for v in ("base", "feat1e-4")] + [(k, "base") for k in LARGE_KEYS])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", FWD_FORMS)
@pytest.mark.parametrize("key,variant", FWD_RUNS, ids=lambda v: str(v))
def test_forward(dev, key, variant, form, layout):
    M = size_of(key)
    external = form == "f32-ext"
    ref = D.reference(M, variant, external)
    c = ref["case"]
    h = Held(dev, c, layout)
    prec = "f32" if external else form
    pe = D.embed_pos(c["x"]).to(dev) if external else None
    tag = f"M{M}-{variant}-{layout}"
    out, none = h.fwd(prec, embed_pos=pe)
    assert none is None
    check(f"fwd {form}", tag, dict(out=out.cpu()), ref, f16=form == "f16")
    if prec == "f32":
        sdf = ops.decoder_fwd_sdf(h.packed("f32"), h.feat, h.lay, h.x, pe, M)
    else:
        sdf = ops.decoder_fwd_sdf(None, h.feat, h.lay, h.x, None, M, precision=prec, packed16=h.packed(prec))
    assert sdf.shape == (M,)
    err = D._stat((sdf.cpu().double() - ref["r64"]["out"][:, 3]).abs()[:, None], torch.arange(M))
    g_max, g_rms = (D.F16_TOL, math.inf) if form == "f16" else D.gates("sdf", ref["e32"]["sdf"], ref["extra"]["sdf"])
    assert err["max"] <= g_max and err["rms"] <= g_rms, \
        f"fwd_sdf {form} {tag}: sample {err['where']} off by {err['max']:.3e} (gate {g_max:.2e}), rms {err['rms']:.3e} (gate {g_rms:.2e})"


# ============================================================================================================== backward
# form -> (precision, record, switches on, deterministic, frozen)
BWD_FORMS = {
    "f32": ("f32", True, True, False, False),
    "f32-ext": ("f32", True, True, False, False),
    "bf16x6": ("bf16x6", "lean", True, False, False),
    "bf16x6-full": ("bf16x6", True, False, False, False),
    "bf16x6-det": ("bf16x6", "lean", True, True, False),
    "bf16x6-frozen": ("bf16x6", "masks", True, False, True),
    "f16x3": ("f16x3", "lean", True, False, False),
    "f16x3-full": ("f16x3", True, False, False, False),
    "f16x3-det": ("f16x3", "lean", True, True, False),
    "f16x3-frozen": ("f16x3", "masks", True, False, True),
}
BWD_RUNS = ([(M, "base", f) for M in D.SMALL_MS for f in BWD_FORMS]
            + [(M, "subnormal", f) for M in (33, 129, 4096 + 17) for f in BWD_FORMS]
            + [(M, "feat1e-4", f) for M in (129, 4096 + 17) for f in ("f32", "bf16x6", "f16x3")]
            + [(k, "base", f) for k in LARGE_KEYS for f in ("f32", "bf16x6", "f16x3")])


# the workgroup-count edges of the weight-gradient kernels on the default forms (128 T + 1: the LDS kernel's, which f32 runs)
EDGE_RUNS = [(k, "base", f) for k in EDGE_KEYS[:2] for f in ("f32", "bf16x6", "f16x3")] + [("128T+1", "base", "f32")]


def further(chain, record, wgrad, rc=False, det=False, frozen=False, off=(), cut=None):
    return dict(chain=chain, record=record, wgrad=wgrad, rc=rc, det=det, frozen=frozen, off=off, cut=cut)


# The further forms.  chain: the arithmetic of the forward and of the backward chain; record: what the forward keeps; wgrad:
# wgrad_precision; rc: recompute_h1; off: the ops switches turned off for the call (the others stay at their defaults); cut: the
# two-plane arithmetic's cut (decoder_cpu.CUTS)
BWD_FORMS2 = {
    "f16x3+f32w": further("f16x3", True, "f32"),
    "bf16x6+f32w": further("bf16x6", True, "f32"),
    "f32+stream_f16x3": further("f32", True, "stream_f16x3"),
    "f32+stream_bf16x6": further("f32", True, "stream_bf16x6"),
    "f16x3+stream_bf16x6": further("f16x3", True, "stream_bf16x6"),
    "f16x3-full-rc": further("f16x3", True, "stream_f16x3", rc=True),
    "bf16x6-full-rc": further("bf16x6", True, "stream_bf16x6", rc=True),
    "f16x3-lean-fulldact": further("f16x3", "lean", "stream_f16x3", rc=True, off=("LEAN_DACT",)),
    "bf16x6-lean-fulldact": further("bf16x6", "lean", "stream_bf16x6", rc=True, off=("LEAN_DACT",)),
    "f16x3-lists": further("f16x3", "lean", "stream_f16x3", rc=True, off=("COMPACT_LIVE",)),
    "bf16x6-lists": further("bf16x6", "lean", "stream_bf16x6", rc=True, off=("COMPACT_LIVE",)),
    "f16x3-det-lists": further("f16x3", "lean", "stream_f16x3", rc=True, det=True, off=("COMPACT_LIVE",)),
    "bf16x6-det-lists": further("bf16x6", "lean", "stream_bf16x6", rc=True, det=True, off=("COMPACT_LIVE",)),
    "f16x3-frozen-lists": further("f16x3", "masks", None, frozen=True, off=("COMPACT_LIVE",)),
    "bf16x3": further("f16x3", True, "bf16x3", cut="lds"),
    "f32+bf16x3": further("f32", True, "bf16x3", cut="lds"),
    "stream_bf16x3": further("f16x3", True, "stream_bf16x3", cut="stream"),
}


def further_runs():
    """(size key, variant, form): 33, 129 (also with subnormal rows), 4113, 32 T - 31 and 32 T + 1 for every further form; 128 T + 1
    where the LDS weight-gradient kernel runs (its workgroups count 128-sample block tiles); P + 33 behind a 16-bit chain
    (the fp32 chain has no persistent kernel)"""
    runs = []
    for form, f in BWD_FORMS2.items():
        runs += [(33, "base", form), (129, "base", form), (129, "subnormal", form), (4096 + 17, "base", form),
                 ("32T-31", "base", form), ("32T+1", "base", form)]
        if f["wgrad"] in ("f32", "bf16x3"):
            runs.append(("128T+1", "base", form))
        if f["chain"] != "f32":
            runs.append(("P+33", "base", form))
    # by size, so that the float64 answer of a size is formed once per layout
    order = {k: i for i, k in enumerate((33, 129, 4096 + 17) + EDGE_KEYS + LARGE_KEYS)}
    return sorted(runs, key=lambda r: (order[r[0]], r[1]))


def run_further(h, form):
    """a further form through ops.decoder_bwd -> dict of host tensors as run_backward's"""
    f = BWD_FORMS2[form]
    M, chain = h.M, f["chain"]
    grads = None if f["frozen"] else [torch.zeros_like(w) for w in h.ws]
    keep = (ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT)
    try:
        for name in f["off"]:
            setattr(ops, name, False)
        out, saved = h.fwd(chain, save=f["record"])
        kw = dict(wgrad_precision=f["wgrad"]) if f["wgrad"] is not None else {}
        if chain == "f32":
            dfeat, dx, dpe = ops.decoder_bwd(h.packed("f32"), h.feat, h.lay, h.x, None, out, h.dout, saved, grads, M, **kw)
        else:
            dfeat, dx, dpe = ops.decoder_bwd(None, h.feat, h.lay, h.x, None, out, h.dout, saved, grads, M, precision=chain,
                                             packed16=h.packed(chain), recompute_h1=f["rc"], deterministic=f["det"], **kw)
    finally:
        ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT = keep
    assert dpe is None
    return dict(out=out.cpu(), dfeat=from_layout(dfeat, h.layout, M).cpu(), dx=dx.cpu(), dembed_pos=None,
                grads=[g.cpu() for g in grads] if grads is not None else None)


def run_backward(h, form, ref):
    """-> dict of host tensors: dfeat [M,32] (AoS order), dx, dembed_pos (external form), grads (None: frozen)"""
    prec, record, switches, det, frozen = BWD_FORMS[form]
    M = h.M
    external = form == "f32-ext"
    pe = D.embed_pos(ref["case"]["x"]).to(h.x.device) if external else None
    grads = None if frozen else [torch.zeros_like(w) for w in h.ws]
    keep = (ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT)
    try:
        if not switches:
            ops.SKIP_ZERO_TILES = ops.COMPACT_LIVE = ops.LEAN_DACT = False
        out, saved = h.fwd(prec, save=record, embed_pos=pe)
        if prec == "f32":
            dfeat, dx, dpe = ops.decoder_bwd(h.packed("f32"), h.feat, h.lay, h.x, pe, out, h.dout, saved, grads, M)
        else:
            lean = record == "lean"
            dfeat, dx, dpe = ops.decoder_bwd(None, h.feat, h.lay, h.x, None, out, h.dout, saved, grads, M, precision=prec,
                                             packed16=h.packed(prec), wgrad_precision=("stream_" + prec) if lean else "auto",
                                             recompute_h1=lean, deterministic=det)
    finally:
        ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT = keep
    return dict(out=out.cpu(), dfeat=from_layout(dfeat, h.layout, M).cpu(), dx=dx.cpu(),
                dembed_pos=dpe.cpu() if dpe is not None else None, grads=[g.cpu() for g in grads] if grads is not None else None)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key,variant,form", BWD_RUNS + EDGE_RUNS, ids=lambda v: str(v))
def test_backward(dev, key, variant, form, layout):
    M = size_of(key)
    ref = D.reference(M, variant, form == "f32-ext")
    h = Held(dev, ref["case"], layout)
    assert (ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT) == (True, True, True), "the ops switches at their defaults"
    res = run_backward(h, form, ref)
    check(f"bwd {form}", f"M{M}-{variant}-{layout}", res, ref)
    if variant == "subnormal":
        rows = ref["case"]["subnormal"]
        assert bool(torch.isfinite(res["dfeat"][rows]).all()) and bool(torch.isfinite(res["dx"][rows]).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key,variant,form", further_runs(), ids=lambda v: str(v))
def test_backward_further_forms(dev, key, variant, form, layout):
    M = size_of(key)
    ref = D.reference(M, variant)
    h = Held(dev, ref["case"], layout)
    assert (ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT) == (True, True, True), "the ops switches at their defaults"
    res = run_further(h, form)
    assert (ops.SKIP_ZERO_TILES, ops.COMPACT_LIVE, ops.LEAN_DACT) == (True, True, True), "... and put back"
    check(f"bwd {form}", f"M{M}-{variant}-{layout}", res, ref, cut=BWD_FORMS2[form]["cut"])
    if variant == "subnormal":
        rows = ref["case"]["subnormal"]
        assert bool(torch.isfinite(res["dfeat"][rows]).all()) and bool(torch.isfinite(res["dx"][rows]).all())
    if BWD_FORMS2[form]["det"]:
        # the ordered lists and the ordered reduce: the same inputs, the same bytes (the chain fills its lists in another order)
        again = run_further(h, form)
        for name, a, b in zip(ops.DECODER_PARAM_ORDER, res["grads"], again["grads"]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{form} M{M}-{layout}: d {name} differs between two calls"
        assert torch.equal(res["dfeat"], again["dfeat"]) and torch.equal(res["dx"], again["dx"])


def test_refused_forms_are_refused(dev):
    """what ops.decoder_bwd does not offer raises instead of running something else: the fp32 weight-gradient kernels under
    deterministic=True, a kernel that reads H1 on a lean record (the LDS kernels, the streaming kernel of the other family, the
    two-plane one), weight gradients from a masks-only record, recompute_h1 with a kernel that cannot, the other family's packed16"""
    ref = D.reference(129)
    h = Held(dev, ref["case"], "aos")
    M = h.M
    grads = lambda: [torch.zeros_like(w) for w in h.ws]      # noqa: E731

    def bwd(chain, out, saved, g, **kw):
        return ops.decoder_bwd(None, h.feat, h.lay, h.x, None, out, h.dout, saved, g, M, precision=chain, packed16=h.packed(chain), **kw)

    for chain in ("f16x3", "bf16x6"):
        other = "bf16x6" if chain == "f16x3" else "f16x3"
        out, full = h.fwd(chain, save=True)
        for wp in ("f32", "bf16x3"):
            with pytest.raises(RuntimeError, match="deterministic"):
                bwd(chain, out, full, grads(), wgrad_precision=wp, deterministic=True)
            with pytest.raises(RuntimeError, match="recompute_h1"):
                bwd(chain, out, full, grads(), wgrad_precision=wp, recompute_h1=True)
        with pytest.raises(RuntimeError, match="recompute_h1"):
            bwd(chain, out, full, grads(), wgrad_precision="stream_bf16x3", recompute_h1=True)
        with pytest.raises(RuntimeError, match="packed for"):
            bwd(chain, out, full, grads(), wgrad_precision="stream_" + other, recompute_h1=True)
        with pytest.raises(RuntimeError, match="packed for"):
            ops.decoder_bwd(None, h.feat, h.lay, h.x, None, out, h.dout, full, grads(), M, precision=chain, packed16=h.packed(other))
        out_l, lean = h.fwd(chain, save="lean")
        for wp in ("f32", "bf16x3", "stream_bf16x3", "stream_" + other):
            with pytest.raises(RuntimeError, match="lean"):
                bwd(chain, out_l, lean, grads(), wgrad_precision=wp)
        out_m, masks = h.fwd(chain, save="masks")
        with pytest.raises(RuntimeError, match="masks only"):
            bwd(chain, out_m, masks, grads())
    out, saved = h.fwd("f32", save=True)
    with pytest.raises(RuntimeError, match="deterministic"):
        ops.decoder_bwd(h.packed("f32"), h.feat, h.lay, h.x, None, out, h.dout, saved, grads(), M, deterministic=True)
    with pytest.raises(RuntimeError, match="lean"):
        h.fwd("f32", save="lean")
