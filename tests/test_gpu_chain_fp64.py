"""GPU (-m gpu): the training step AS JointEncoding.forward_from_table AND forward COMPOSE IT against the float64 chain of
tests/chain_cpu.py -- the seams between the kernels, which the unit files (test_gpu_step_fp64, test_gpu_hashgrid_fp64,
test_gpu_decoder_fp64, test_gpu_render_fp64) cannot see: there the TEST supplies counts, the wants_dx mask, dout, the live-sample
list and the tile lists; here the kernels hand them to each other.

Cases (chain_cpu.SPECS): ragged shapes from 1 x 16 to 16 x 129, rays kept by per-ray rejection so that every discrete decision holds
with a margin in float64 (tests/test_chain_cpu.py): no allowance for flipped decisions, no outliers, no skipped rays.

Compared, per run: rgb and depth per ray; the eight loss entries (NaN places must coincide); z_vals and counts for equality; the table
gradient element by element over the tensor's largest float64 magnitude, exactly 0.0 where the chain's is zero or no corner lands;
the ten decoder gradients per tensor; rot.grad and trans.grad per pose over the row's largest magnitude, exactly 0.0 for a pose without a
ray; through the two-launch entry the per-ray d rays_o and d rays_d.  Gates: the project's, unchanged -- the largest error <=
min(max(GATE_FACTOR * e32, GATE_FLOOR), ceiling), CEIL_VALUE for values and CEIL_GRAD for gradients (tests/render_cpu.py), e32 the fp32
oracle's distance from the chain on the same case.

Forms: (1) default -- forward_from_table, bf16x6, mask on, live-sample list, lean record -- on every case; on chain_cpu.FORM_CASES also
(2) decoder_precision f16x3 and f32, (3) deterministic (two calls, the same bytes), (4) in-place accumulation onto a non-zero base, then
grid_grad_is_zero_at_backward on zeroed gradients, (5) mask_fixed_rays = False, (6) ops.pose_rays + forward, (7) tracking (frozen map
inside frozen_weights), and (8) wgrad_precision f32 and lean_record = False on N17-S75.

The worst group (largest error / gate) per case and form on an MI355X, kernel error | e32 ("The composed step against
float64", has the same table):

  default              N1-S16 table 4.8e-6 | 4.6e-6; N5-S33 sdf_loss 1.3e-6 | 6.5e-8; N17-S64 d rgb_linear.0.weight 5.5e-6 | 2.2e-6;
                       N17-S75 rgb 5.5e-7 | 4.8e-7; N33-S64 d translation 1.7e-5 | 9.3e-6; N16-S129 d rgb_linear.0.weight 5.1e-6 | 3.3e-6;
                       N8-S64-fixed table 1.0e-5 | 6.7e-6; N17-S64-nodepth d pts_linear.0.bias 5.9e-7 | 3.6e-7
  Python objective, deterministic (both calls), in place (both), no mask, pose_rays + forward, wgrad f32, full record
                       the default form's group and figures on every case they run (N16-S129 in place onto a base: 5.2e-6)
  f16x3                N5-S33 sdf_loss 9.6e-7 | 6.5e-8; N17-S64 d rgb_linear.0.weight 5.6e-6 | 2.2e-6; N17-S75 d quaternion 1.4e-5 | 1.3e-5;
                       N16-S129 d rgb_linear.0.weight 5.2e-6 | 3.3e-6
  f32                  N5-S33 sdf_loss 9.6e-7 | 6.5e-8; N17-S64 5.5e-6 | 2.2e-6; N17-S75 rgb 5.5e-7 | 4.8e-7; N16-S129 5.2e-6 | 3.3e-6
  tracking (both)      N5-S33 sdf_loss 1.3e-6 | 6.5e-8; N17-S64 depth 8.7e-7 | 6.6e-7; N17-S75 rgb 5.5e-7 | 4.8e-7;
                       N16-S129 d quaternion 5.8e-5 | 5.0e-5

No case or form missed a gate, and none came nearer to one than a third of it."""
import contextlib

import numpy as np
import pytest
import torch

from mipsfusion_amd import ops
from mipsfusion_amd.model import JointEncoding, scene_rep
from oracle import path_cpu

from . import chain_cpu as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ the model of a case
_MODELS = {}


def model_of(name, dev):
    """the module built from the case's weights and its inputs on the device, once a process"""
    if name in _MODELS:
        return _MODELS[name]
    case = C.build_case(name)
    cfg = case["cfg"]
    bb = torch.from_numpy(np.array(cfg["mapping"]["bound"]))
    nf = torch.from_numpy(np.array(cfg["mapping"]["localMLP_max_len"]))
    with torch.random.fork_rng(devices=[]):
        m = JointEncoding(cfg, bb, nf).to(dev).train()
    with torch.no_grad():
        assert m.embed_fn.params.numel() == case["params"].size
        m.embed_fn.params.copy_(torch.from_numpy(case["params"]).to(dev))
        for p, w in zip(m.decoder.ordered_parameters(), case["weights"]):
            p.copy_(w.to(dev))
    rays = C.rays_of(case)
    inp = dict(table=case["table"].to(dev), rows=case["rows"].to(dev), owner=case["owner"].to(dev), noise=case["noise"].to(dev),
               fixed=case["fixed"].to(dev), d_cam=rays[:, :3].contiguous().to(dev), rgb=rays[:, 3:6].contiguous().to(dev),
               d=rays[:, 6:7].contiguous().to(dev))
    _MODELS[name] = (m, inp)
    return _MODELS[name]


def map_parameters(m):
    return [m.embed_fn.params] + m.decoder.ordered_parameters()


@contextlib.contextmanager
def settings(m, **attrs):
    keep = {k: getattr(m, k) for k in attrs}
    for k, v in attrs.items():
        setattr(m, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(m, k, v)


@contextlib.contextmanager
def render_inputs(seen):
    """what the placement handed to the render and loss launch: z_vals and counts, as the composed step passed them on"""
    cls = scene_rep._RenderFn
    own = "apply" in vars(cls)
    orig = cls.apply

    def spy(*a):
        seen["z_vals"], seen["counts"] = a[1].detach().clone(), a[4].detach().clone()
        return orig(*a)

    cls.apply = spy
    try:
        yield
    finally:
        if own:
            cls.apply = orig
        else:
            del cls.apply


def run(name, dev, *, entry="table", loss="kernel", in_place=False, base=None, tracking=False):
    """one training step of the case -> the results on the host.  entry: "table" (forward_from_table) | "rays" (ops.pose_rays +
    forward); loss: "kernel" (ret["_loss_total"]) | "python" (path_cpu.total_loss of the returned entries); base: {tensor name: the
    non-zero value its .grad holds on entry} (in-place accumulation); tracking: the map takes no gradient"""
    m, inp = model_of(name, dev)
    case = C.build_case(name)
    rot = case["rot"].to(dev).clone().requires_grad_(True)
    trans = case["trans"].to(dev).clone().requires_grad_(True)
    params = map_parameters(m)
    if base is None:
        m.zero_grad(set_to_none=True)
    else:
        for p, b in zip(params + [rot, trans], base):
            p.grad = b.to(dev).clone()
    seen, ro, rd = {}, None, None
    with render_inputs(seen):
        if entry == "table":
            ret = m.forward_from_table(inp["table"], inp["rows"], rot, trans, inp["fixed"], inp["owner"], inp["noise"], EMD_w=case["emd_w"],
                                       accumulate_in_place=in_place)
        else:
            ro, rd = ops.pose_rays(rot, trans, inp["fixed"], inp["owner"], inp["d_cam"])
            ro.retain_grad(), rd.retain_grad()
            ret = m.forward(ro, rd, inp["rgb"], inp["d"], EMD_w=case["emd_w"], noise=inp["noise"])
    total = ret["_loss_total"] if loss == "kernel" else path_cpu.total_loss(ret, case["cfg"]["training"])
    total.backward()
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.detach().cpu()      # noqa: E731
    res = dict(rgb=host(ret["rgb"]), depth=host(ret["depth"]), losses=host(ret["_loss_vec"]), z_vals=host(seen["z_vals"]),
               counts=host(seen["counts"]), d_rot=host(rot.grad), d_trans=host(trans.grad), param_grads=[host(p.grad) for p in params])
    if not tracking:
        res["table"] = res["param_grads"][0].reshape(-1, 2)
        res["grads"] = res["param_grads"][1:]
    if ro is not None:
        res["d_rays_o"], res["d_rays_d"] = host(ro.grad), host(rd.grad)
    return res


# ------------------------------------------------------------------------------------------------------------- the comparison
def report(form, name, group, err, e32):
    print(f"\n  fp64 | {form} | {name} | {group} | kernel {err:.2e} | e32 {e32:.2e}", end="")


def held(form, name, res, *, minus=None):
    """every compared group of a run under its gate; minus: the base the in-place forms started from (subtracted in float64)"""
    case, c64, e32 = C.build_case(name), C.answer(name), C.e32(name)
    lv = case["levels"]
    K, Fn = case["spec"]["K"], case["spec"]["F"]
    assert torch.equal(res["z_vals"], c64["z_vals"]), f"{form} {name}: z_vals are not the placement's, bit for bit"
    assert torch.equal(res["counts"], c64["counts"]), f"{form} {name}: counts {res['counts'].tolist()} != {c64['counts'].tolist()}"
    res = dict(res)
    for k in ("d_rot", "d_trans"):
        if res[k] is None:                                       # no ray of an optimised pose: no pose gradient at all
            assert not bool(c64[k].any()), f"{form} {name}: no {k} although optimised poses own rays"
            res[k] = torch.zeros_like(c64[k])
    if minus is not None:
        res["table"] = res["table"].double() - minus[0].reshape(-1, 2).double()
        res["grads"] = [g.double() - b.double() for g, b in zip(res["grads"], minus[1:11])]
        res["d_rot"], res["d_trans"] = res["d_rot"].double() - minus[11].double(), res["d_trans"].double() - minus[12].double()
    if "table" in res:
        dense, hit = C.table_grad(c64, lv)
        got = C._np64(res["table"])
        quiet = ~hit[:, None] | (dense == 0.0)
        assert not got[quiet].any(), \
            f"{form} {name}: {np.count_nonzero(got[quiet])} table entries are not 0.0 where the chain's are zero or no corner lands"
    for k in range(K):
        if not bool(((case["owner"] % (Fn + K)) == Fn + k).any()):
            assert not bool(res["d_rot"][k].any()) and not bool(res["d_trans"][k].any()), f"{form} {name}: pose {k} owns no ray: exactly 0.0"
    err = C.errors(res, c64, lv)
    worst = None
    for group, (e, where) in err.items():
        gate = C.gate(group, e32[group])
        report(form, name, group, e, e32[group])
        if worst is None or e / gate > worst[1] / worst[2]:
            worst = (group, e, gate, where)
    print(f"\n  fp64 | {form} | {name} | WORST {worst[0]} | kernel {worst[1]:.2e} | e32 {e32[worst[0]]:.2e}", end="")
    for group, (e, where) in err.items():
        gate = C.gate(group, e32[group])
        assert e <= gate, (f"{form} {name}: {group} off by {e:.3e} (gate {gate:.2e}, e32 {e32[group]:.2e}) at "
                           f"{C.place(case, c64, group, where)}")
    return err


# ----------------------------------------------------------------------------------------------------------------- the forms
@pytest.mark.parametrize("name", C.CASES)
def test_default_step(dev, name):
    """forward_from_table, bf16x6, mask on, live-sample list, lean record; ret["_loss_total"].backward()"""
    m, _ = model_of(name, dev)
    assert m.decoder_precision == "bf16x6" and m.mask_fixed_rays and m.lean_record and ops.COMPACT_LIVE and m.wgrad_precision == "auto"
    held("default", name, run(name, dev))


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_python_objective(dev, name):
    """path_cpu.total_loss of the returned entries: the objective's gradient comes from render_bwd at every S"""
    held("python objective", name, run(name, dev, loss="python"))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", C.FORM_CASES)
def test_decoder_precision(dev, name, precision):
    m, _ = model_of(name, dev)
    with settings(m, decoder_precision=precision):
        held(precision, name, run(name, dev))


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_deterministic(dev, name):
    m, _ = model_of(name, dev)
    with settings(m, deterministic=True):
        a, b = run(name, dev), run(name, dev)
    for k in ("rgb", "depth", "losses", "d_rot", "d_trans"):
        assert torch.equal(a[k], b[k]) or (k == "losses" and torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k]))), k
    for i, (x, y) in enumerate(zip(a["param_grads"], b["param_grads"])):
        assert torch.equal(x, y), f"parameter gradient {i} differs between two deterministic calls"
    held("deterministic", name, a)
    held("deterministic, second call", name, b)


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_in_place_accumulation(dev, name):
    """.grad tensors pre-filled with a non-zero base: the result is base + answer; then grid_grad_is_zero_at_backward on zeroed
    gradients: the result is the answer.  The base is half the answer's scale and below: adding it costs one rounding of the sum,
    2^-24 * 1.5 of the scale, under GATE_FLOOR."""
    m, _ = model_of(name, dev)
    case, c64 = C.build_case(name), C.answer(name)
    gen = torch.Generator().manual_seed(11)
    shapes = [(m.embed_fn.params.shape, float(np.abs(c64["dp"]).max()))]
    shapes += [(p.shape, float(g.abs().max())) for p, g in zip(m.decoder.ordered_parameters(), c64["grads"])]
    shapes += [(case["rot"].shape, float(c64["d_rot"].abs().max())), (case["trans"].shape, float(c64["d_trans"].abs().max()))]
    base = [((0.25 + 0.25 * torch.rand(s, generator=gen)) * (2.0 * torch.randint(0, 2, s, generator=gen) - 1.0) * top).float() for s, top in shapes]
    with settings(m, accumulate_param_grads_in_place=True):
        res = run(name, dev, in_place=True, base=base)
        held("in place, onto a base", name, res, minus=base)
        # the zeroed gradients: the same tensors, filled with zeros (as FusedAdam.step(zero_grad=True) leaves them)
        zeros = [torch.zeros_like(b) for b in base]
        with settings(m, grid_grad_is_zero_at_backward=True):
            res = run(name, dev, in_place=True, base=zeros)
        held("in place, zeroed gradients", name, res)


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_without_the_fixed_ray_mask(dev, name):
    m, _ = model_of(name, dev)
    with settings(m, mask_fixed_rays=False):
        held("no mask", name, run(name, dev, loss="python"))


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_two_launch_entry(dev, name):
    """ops.pose_rays followed by forward: the per-ray d rays_o and d rays_d are compared here"""
    res = run(name, dev, entry="rays")
    assert res["d_rays_o"] is not None and res["d_rays_d"] is not None
    err = held("pose_rays + forward", name, res)
    assert "d_rays_o" in err and "d_rays_d" in err


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_tracking(dev, name):
    """every map parameter frozen, inside frozen_weights: the pose gradients under the gates, no parameter gradient appears"""
    m, _ = model_of(name, dev)
    params = map_parameters(m)
    for p in params:
        p.requires_grad_(False)
    m.frozen_weights(True)
    try:
        first = run(name, dev, tracking=True)
        second = run(name, dev, tracking=True)                   # (the operand images packed by the first call are reused)
    finally:
        m.frozen_weights(False)
        for p in params:
            p.requires_grad_(True)
    for res, form in ((first, "tracking"), (second, "tracking, packed weights reused")):
        assert all(g is None for g in res["param_grads"]), "a frozen parameter got a gradient"
        held(form, name, res)


@pytest.mark.parametrize("attrs", [dict(wgrad_precision="f32"), dict(lean_record=False)], ids=["wgrad-f32", "full-record"])
def test_weight_gradient_forms(dev, attrs):
    name = "N17-S75"
    m, _ = model_of(name, dev)
    with settings(m, **attrs):
        held(", ".join(f"{k}={v}" for k, v in attrs.items()), name, run(name, dev))
