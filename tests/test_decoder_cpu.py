"""No GPU: the float64 restatement of the decoder (tests/decoder_cpu.py) held to its conditions, so that
tests/test_gpu_decoder_fp64.py compares the kernels with an answer that is itself checked:

  * in float64 the hand-written forward equals oracle/path_cpu.decoder_forward and the hand-written backward equals autograd
    through it, to 1e-12 of each tensor's maximum (a second, independent statement of the same network);
  * the derivative of the encoding equals a central difference of the float64 sine at the fp32 argument;
  * every case the GPU module uses meets the conditions on its inputs: the threshold share, the planted samples live, zero tiles
    and partially zero tiles present, the yardstick's headroom under GATE_FLOOR (a figure of the host's fp32 sums), the allowance
    for the hardware sine under GATE_FLOOR for the outputs, the summation floor of the parameter gradients under GATE_FLOOR.  The large cases depend on the device's CU count: checked with 256 and with 64."""
import math

import pytest
import torch

from mipsfusion_amd import ops
from oracle import path_cpu, tcnn_cpu

from . import decoder_cpu as D
from . import step_cpu

SMALL = [(M, v) for v in D.VARIANTS for M in D.SMALL_MS]
LARGE = [(M, "base") for cu in (256, 64) for M in D.large_ms(cu)]


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


@pytest.mark.parametrize("M,variant", SMALL + LARGE, ids=lambda v: str(v))
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
