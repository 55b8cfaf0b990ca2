"""No GPU: the float64 restatement of the decoder (tests/decoder_cpu.py) held to its conditions, so that
tests/test_gpu_decoder_fp64.py compares the kernels with an answer that is itself checked:

  * in float64 the hand-written forward equals oracle/path_cpu.decoder_forward and the hand-written backward equals autograd
    through it, to 1e-12 of each tensor's maximum (a second, independent statement of the same network);
  * the derivative of the encoding equals a central difference of the float64 sine at the fp32 argument;
  * every case the GPU module uses meets the conditions on its inputs: the threshold share, the planted samples live, zero tiles
    and partially zero tiles present, the yardstick's headroom under GATE_FLOOR (a figure of the host's fp32 sums), the allowance
    for the hardware sine under GATE_FLOOR for the outputs, the summation floor of the parameter gradients under GATE_FLOOR.  The large cases depend on the device's CU count: checked with 256 and with 64;
  * the cases of the list forms hold zero tiles and mixed tiles, and those of the ordered lists give every list something to put
    in order;
  * the bound of the two-plane bf16 arithmetics (decoder_cpu.two_plane_bound) holds for the float64 backward with exactly those
    operands cut to two bf16 pieces, and is exceeded when they are cut to one."""
import math

import pytest
import torch

from mipsfusion_amd import ops
from oracle import path_cpu, tcnn_cpu

from . import decoder_cpu as D
from . import step_cpu

SMALL = [(M, v) for v in D.VARIANTS for M in D.SMALL_MS]
LARGE = [(M, "base") for cu in (256, 64) for M in D.large_ms(cu)]
EDGE = sorted({(M, "base") for cu in (256, 64) for M in D.tile_edge_ms(cu)})
FORM_CASES = sorted({mv for cu in (256, 64) for mv in D.form_cases(cu)})


def rel(a, b):
    top = float(b.abs().max())
    return float((a - b).abs().max()) / (top if top > 0 else 1.0)


@pytest.mark.parametrize("M,variant", [(1, "base"), (33, "base"), (129, "subnormal"), (4113, "feat1e-4")])
def test_forward_and_backward_equal_the_oracle_and_autograd_in_float64(M, variant):
    c = D.case(M, variant)
    w64 = {k: t.double().requires_grad_(True) for k, t in zip(ops.DECODER_PARAM_ORDER, c["weights"])}
    x, feat = c["x"].double().requires_grad_(True), c["feat"].double().requires_grad_(True)
    arg = step_cpu.freq_args(c["x"], D.N_FREQ).double()
    # the path through the encoding, by autograd: the fp32 argument's own derivative d arg / d x = 2^k pi_f, held as a constant
    k = D.freq_scale(torch.float64)[None, None, :, None]
    pe = torch.sin(arg + (x[:, :, None, None] - x.detach()[:, :, None, None]) * k).reshape(M, D.N_PE)
    pe.retain_grad()
    out = path_cpu.decoder_forward(w64, feat, pe, x)
    dout = c["dout"].double()
    out.backward(dout)
    r = D.evaluate(c["weights"], c["feat"], c["x"], c["dout"], torch.float64)
    assert rel(r["out"], out.detach()) <= 1e-12
    assert rel(r["dfeat"], feat.grad) <= 1e-12 and rel(r["dx"], x.grad) <= 1e-12 and rel(r["dembed_pos"], pe.grad) <= 1e-12
    for name, g in zip(ops.DECODER_PARAM_ORDER, r["grads"]):
        assert rel(g, w64[name].grad) <= 1e-12, name
    # the external-encoding form: the encoding is an input, dx is the direct path alone
    x2 = c["x"].double().requires_grad_(True)
    pe2 = D.embed_pos(c["x"]).double().requires_grad_(True)
    out2 = path_cpu.decoder_forward({n: t.detach() for n, t in w64.items()}, c["feat"].double(), pe2, x2)
    out2.backward(dout)
    e = D.evaluate(c["weights"], c["feat"], c["x"], c["dout"], torch.float64, external=True)
    assert rel(e["out"], out2.detach()) <= 1e-12 and rel(e["dx"], x2.grad) <= 1e-12 and rel(e["dembed_pos"], pe2.grad) <= 1e-12
    assert torch.equal(D.embed_pos(c["x"]), tcnn_cpu.frequency_forward(c["x"], D.N_FREQ)), "the oracle's fp32 encoding, bit for bit"


def test_encoding_derivative_against_a_central_difference():
    x = D.case(129)["x"]
    arg = step_cpu.freq_args(x, D.N_FREQ).double()
    _, dpe_dx = D.encoding(x, torch.float64)
    h = 2.0 ** -13
    k = D.freq_scale(torch.float64)[None, None, :, None]
    # d sin(arg(x)) / dx with d arg / dx = 2^k pi_f: the central difference in the argument, times that factor
    diff = (torch.sin(arg + h) - torch.sin(arg - h)) / (2 * h) * k
    # the difference's own error: h^2 / 6 of the third derivative, and the rounding of arg +- h (|arg| < 2^11) over 2 h
    assert float(((dpe_dx - diff).abs() / k).max()) <= h * h / 6 + 2.0 ** -42 / (2 * h)
    pe32, d32 = D.encoding(x, torch.float32)
    assert pe32.dtype == torch.float32 and float((pe32.double() - torch.sin(arg).reshape(129, -1)).abs().max()) <= 2.0 ** -24


@pytest.mark.parametrize("M,variant", SMALL + LARGE + EDGE, ids=lambda v: str(v))
def test_every_case_meets_the_conditions_on_its_inputs(M, variant):
    ref = D.reference(M, variant)
    c = ref["case"]
    x, dout = c["x"], c["dout"]
    assert float(x.min()) >= D.X_LO and float(x.max()) <= D.X_HI
    n = min(3 * M, len(D.X_SPECIAL))
    assert x.reshape(-1)[:n].tolist() == [float(torch.tensor(v, dtype=torch.float32)) for v in D.X_SPECIAL[:n]]
    assert M < 3 or math.copysign(1.0, float(x[0, 1])) == -1.0, "-0.0 keeps its sign"
    # thresholds
    assert float(c["threshold"].double().mean()) <= D.THRESHOLD_SHARE
    assert bool((dout[c["threshold"]] == 0).all())
    live = (dout != 0).any(1)
    assert bool(live[c["planted"]].all()) and not bool(c["threshold"][c["planted"]].any())
    top = dout[c["planted"]].abs().max(1).values
    assert float(top.min()) > 0.05 * D.TOP_SCALE, "the planted samples carry the top of the scale"
    for i in {0, M - 1} | set(range(0, M, 128)) | (set(range(M - M % 32, M)) if M % 32 else set()):
        assert bool(live[i]), i
    # zero patterns
    zero, partial = D.zero_tiles(dout)
    assert M < 64 or zero >= 1, "an all-zero 32-sample tile from M = 64 on (the tail of the first ray)"
    assert M < 32 or partial >= 1, "a partially zero tile from M = 32 on (M = 31 is one partial tile: planted live throughout)"
    assert M < 8 or M == 31 or bool((~live).any())
    if variant == "subnormal" and M >= 32:
        rows = dout[c["subnormal"]]
        assert rows.shape[0] >= 1 and bool((rows.abs() < D.FLT_MIN).all()) and bool((rows != 0).any(1).all())
    # the yardstick's headroom: gate (a) is a property of the arithmetic, not of one row's luck
    for name, v in ref["e32_normal"].items():
        assert v["max"] < D.GATE_FLOOR / 4, f"{name}: e32 {v['max']:.2e} (sample {v['where']})"
        assert v["rms"] <= v["max"]
    assert ref["flips"] == 0, "no live sample changes its ReLU pattern under the shifted encoding"
    # the allowance for the hardware sine and cosine, with the committed constants
    for name in D.OUT_NAMES:
        assert ref["extra"][name]["max"] < D.GATE_FLOOR, f"{name}: extra {ref['extra'][name]['max']:.2e}"
    # the least error of an fp32 sum over the samples (summation_floor): a floor of gate (b); it leaves gate (a) at GATE_FLOOR
    for name in ops.DECODER_PARAM_ORDER:
        assert 0 < ref["extra"][name]["max"] < D.GATE_FLOOR, f"{name}: extra {ref['extra'][name]['max']:.2e}"
        assert ref["extra"][name]["rms"] <= D.GATE_FACTOR * 5 * max(ref["e32"][name]["rms"], 2.0 ** -24), \
            f"{name}: the floor is above what 8 e32 typically is"
    ext = D.reference(M, variant, external=True)
    assert all(ext["extra"][n]["max"] <= 2.0 ** -23 for n in D.OUT_NAMES + D.ROW_NAMES), "an input encoding: the result's own rounding alone"
    for name, v in ext["e32_normal"].items():
        assert v["max"] < D.GATE_FLOOR / 4, f"external encoding, {name}: e32 {v['max']:.2e}"


def test_gates_and_errors():
    g = D.gates("dfeat", dict(max=1e-7, rms=1e-8))
    assert g == (D.GATE_FLOOR, 8e-8)
    assert D.gates("rgb", dict(max=1e-3, rms=1e-4))[0] == D.CEIL_VALUE and D.gates("dx", dict(max=1e-3, rms=1e-4))[0] == D.CEIL_GRAD
    assert D.gates("sdf", dict(max=1e-7, rms=1e-8), dict(max=5e-6, rms=2e-6)) == (5e-6, 2e-6)
    # a dropped sample of the partial tile, a misplaced row: far above the gates at the largest M
    ref = D.reference(D.large_ms(256)[2])
    c, r64 = ref["case"], ref["r64"]
    M = c["M"]
    for what in ("dropped", "misplaced"):
        dout = c["dout"].clone()
        if what == "dropped":
            dout[M - 1] = 0.0
        else:
            dout[[0, 1]] = dout[[1, 0]]
        bad = D.evaluate(c["weights"], c["feat"], c["x"], dout, torch.float64)
        err = D.errors(dict(grads=bad["grads"]), r64, c["dout"])
        worst = max(err[n]["max"] / D.gates(n, ref["e32"][n], ref["extra"][n])[0] for n in ops.DECODER_PARAM_ORDER)
        assert worst > 10.0, (what, worst)


@pytest.mark.parametrize("cu", (256, 64))
def test_cases_of_the_list_forms_have_zero_tiles_mixed_tiles_and_lists_to_order(cu):
    """The live-tile-list forms (COMPACT_LIVE off) are exercised only where the chain skips a tile and keeps a tile with dead rows
    in it; the ordered lists (deterministic=True) only where a list has several members, handed in by several workgroups."""
    T = min(cu, 256)
    for M, variant in D.form_cases(cu):
        if M >= 129:
            zero, mixed = D.zero_tiles(D.case(M, variant)["dout"])
            assert zero >= 1 and mixed >= 1, (M, variant, zero, mixed)
    t_minus, t_plus, _ = D.tile_edge_ms(cu)
    assert ((t_minus + 31) // 32, (t_plus + 31) // 32) == (T, T + 1) and t_minus % 32 == 1, "T tiles, the last ragged; T + 1 tiles"
    assert (D.tile_edge_ms(cu)[2] + 127) // 128 == T + 1
    # P + 33: more live tiles than the weight-gradient kernel has workgroups, so every workgroup walks several list positions
    big = D.live_tiles(D.case(D.large_ms(cu)[2])["dout"])
    assert big.numel() > T, (big.numel(), T)
    # 32 T + 1 has T + 1 tiles, one of them zero at the least (above): it cannot hold more than T live ones.  What the ordering
    # needs there: every one of the eight lists has several members (a list of one is in order whatever the schedule)
    for M in (t_plus, D.large_ms(cu)[2]):
        tiles = D.live_tiles(D.case(M)["dout"])
        for q in range(8):
            mine = tiles[((tiles >> 3) & 7) == q]
            assert mine.numel() >= 2, (M, q, mine.tolist())


@pytest.mark.parametrize("M,variant", FORM_CASES, ids=lambda v: str(v))
def test_two_plane_bound_holds_for_two_pieces_and_not_for_one(M, variant):
    """(a) the float64 backward with exactly the operands a two-plane arithmetic cuts (decoder_cpu.CUTS) rounded to two bf16
    pieces, the lo lo pair dropped, stays inside decoder_cpu.two_plane_bound, element by element and in the rms; (b) with one piece
    it does not, at any size.  Measured on the host this was written on: (a) 0.34 of the bound at M = 33, 0.25 at 129, 0.08 at
    4113, 0.02 - 0.12 at the larger sizes; (b) 110 x the bound at M = 33, 120 x at 129, 33 x at 4113, 12 x at 131105."""
    ref = D.reference(M, variant)
    c = ref["case"]
    want = ref["r64"]["grads"]
    # (the streaming form cuts all ten gradients, the lds form four of them in the same way: one evaluation per number of pieces)
    cut = {pieces: D.evaluate(c["weights"], c["feat"], c["x"], c["dout"], torch.float64, cut=("stream", pieces))["grads"] for pieces in (2, 1)}
    for kind in D.CUTS:
        shares = []
        for pieces in (2, 1):
            e = D.two_plane_errors([g if i in D.CUTS[kind] else r for i, (g, r) in enumerate(zip(cut[pieces], want))], ref, kind)
            assert set(e) == {ops.DECODER_PARAM_ORDER[i] for i in D.CUTS[kind]}
            shares.append(max(max(v["share"], v["rms"] / v["rms_bound"]) for v in e.values()))
            if pieces == 2:
                for name, v in e.items():
                    assert v["share"] <= 1.0 and v["rms"] <= v["rms_bound"], \
                        f"{kind} {name}: element {v['where']} {v['max']:.3e} over its bound {v['bound']:.3e}; rms {v['rms']:.3e} ({v['rms_bound']:.3e})"
        print(f"\n  two-plane bound | {kind} | M{M}-{variant} | two pieces {shares[0]:.3f} | one piece {shares[1]:.1f}", end="")
        assert shares[1] > 1.0, f"{kind}: one bf16 piece stays inside the two-plane bound ({shares[1]:.2f}): the bound has no teeth"


def test_two_plane_constants_and_cut():
    v = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23, -3.1415926, 1e-30, 0.0], dtype=torch.float64)
    hi, lo = D.bf16_pieces(v, 2)
    assert bool(((v.float().double() - hi - lo).abs() <= D.CUT_ONE * v.abs()).all()) and bool((lo.abs() <= D.U_BF16 * (1 + D.U_BF16) * v.abs()).all())
    assert float(hi[0]) == 1.0 + 2.0 ** -7 and float(lo[0]) == 2.0 ** -15, "round to nearest even of the exact residual 2^-15 + 2^-23"
    assert D.bf16_pieces(v, 1)[1].count_nonzero() == 0
    assert 3.0 * 2.0 ** -16 < D.CUT_BOTH < 3.01 * 2.0 ** -16 and D.CUT_ONE == 2.0 ** -16
    # the lds form leaves the small heads and four biases alone; the streaming form cuts all ten
    assert sorted(D.CUTS["lds"]) == [0, 1, 2, 6] and sorted(D.CUTS["stream"]) == list(range(10))
    assert all(n == (1 if ops.DECODER_PARAM_ORDER[i].endswith("bias") else 2) for k in D.CUTS for i, n in D.CUTS[k].items())
    c, want = D.case(33), D.reference(33)["r64"]["grads"]
    lds, stream = (D.evaluate(c["weights"], c["feat"], c["x"], c["dout"], torch.float64, cut=(k, 2))["grads"] for k in ("lds", "stream"))
    for i in range(10):
        assert torch.equal(lds[i], stream[i] if i in D.CUTS["lds"] else want[i]), "only the listed gradients are cut, alike in both forms"
        assert not torch.equal(stream[i], want[i])
