"""GPU tests of the sub-map pose graph (mipsfusion_amd/pose_graph.py, csrc/posegraph.hip) against the float64 restatement of
tests/posegraph_cpu.py.  Both sides compute in float64 from the same inputs, so the float32 anchors may differ by one rounding
and the float64 anchors by rounding noise only; tests/test_posegraph_cpu.py bounds what the order of the sums can contribute
(measured there: at most 1.8e-15 between LAPACK and a fixed-order Cholesky with reversed edge sums).

The 16 graphs are posegraph_cpu.GPU_FIXTURES; the smallest, n2_e1, is N = 2 with the lone key edge (E = 1; 2.1e-16 there).
Measured on an MI355X: float32 anchors equal on all 16 graphs; float64 deviation relative to max(1, |t|_inf) 1.7e-16 .. 9.4e-15
(largest: reject6, lever arms of 40 m), against the gate of 1e-9; steps, solves, rejections, radius and status equal on all."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, pose_graph as pg, synth

from . import posegraph_cpu as R

pytestmark = pytest.mark.gpu

# largest |float64 anchor - restatement| / max(1, |t|_inf) over the fixtures, from a run on an MI355X (gate: 1e-9)
MEASURED = 9.42e-15
FIXTURES = sorted(R.GPU_FIXTURES)
DECREASING = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


_cache = {}


def _case(name):
    """-> (graph, the restatement's result), computed once"""
    if name not in _cache:
        g = R.GPU_FIXTURES[name]()
        _cache[name] = (g, R.optimize(*g, decreasing=DECREASING))
    return _cache[name]


def _upload(graph, dev):
    X, e, o, w = graph
    return (torch.from_numpy(np.ascontiguousarray(X)).to(dev), torch.from_numpy(np.ascontiguousarray(e, np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(o.astype(X.dtype))).to(dev), torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev))


def _run(graph, dev, **kw):
    o64, o32, res, _ = pg.pose_graph_enqueue(*_upload(graph, dev), **kw)
    return o64.cpu().numpy(), o32.cpu().numpy(), res.cpu().numpy()


def _scale(X):
    """max(1, |t|_inf) per anchor, shaped for a [N,4,4] comparison"""
    return np.maximum(1.0, np.abs(X[:, :3, 3]).max(1))[:, None, None]


# ------------------------------------------------------------------------------------------------------------- the graphs
@pytest.mark.parametrize("name", FIXTURES)
def test_graph_matches_the_restatement(dev, name):
    """float32 anchors within 2^-23 * max(1, |t|_inf) (one float32 ulp at the block's magnitude: both sides round a float64 value
    that is far closer than half such an ulp), float64 anchors within 1e-9 * max(1, |t|_inf) (the float32 inputs define the result
    to 6e-8 only; 1e-9 is 60 times inside that and 1e6 above float64 rounding: only another algorithm trips it); steps and status
    equal; solves and rejections equal where every accept/reject decision of the restatement holds with a margin above 1e-9."""
    graph, want = _case(name)
    if name == "n2_e1":
        assert (len(graph[0]), len(graph[1])) == (2, 1), "the smallest accepted graph: one 6x6 block, one edge"
    # on the restatement alone: the fixture decides nothing on a coin toss
    assert R.plateau_margin(want, DECREASING) > 1e-6, f"{name}: a step's decrease sits on the plateau threshold; replace the fixture"
    o64, o32, res = _run(graph, dev, decreasing=DECREASING)
    scale = _scale(want["anchors"])
    d64 = float((np.abs(o64 - want["anchors"]) / scale).max())
    d32 = float((np.abs(o32.astype(np.float64) - want["anchors32"].astype(np.float64)) / scale).max())
    print(f"{name}: N {len(graph[0])} E {len(graph[1])} float64 deviation {d64:.2e} float32 {d32:.2e} | steps {int(res[2])}/{want['steps']} "
          f"solves {int(res[3])}/{want['solves']} rejections {int(res[4])}/{want['rejections']} status {int(res[6])}/{want['status']} "
          f"loss {res[0]:.6e} -> {res[1]:.6e} (restatement {want['first_loss']:.6e} -> {want['loss']:.6e}) radius {res[5]:g}")
    assert np.all(np.abs(o32.astype(np.float64) - want["anchors32"].astype(np.float64)) <= 2.0 ** -23 * scale)
    assert np.all(np.abs(o64 - want["anchors"]) <= 1e-9 * scale)
    assert int(res[2]) == want["steps"] and int(res[6]) == want["status"]
    if R.decision_margin(want) > 1e-9:
        assert int(res[3]) == want["solves"] and int(res[4]) == want["rejections"] and res[5] == want["radius"]
    assert np.array_equal(o64[:, 3], np.tile([0.0, 0, 0, 1], (len(o64), 1))) and np.abs(o64[0] - R.project(graph[0])[0]).max() < 1e-15
    if name.startswith("reject"):
        assert int(res[4]) >= 1


def test_zero_drift_and_unconnected_nodes_come_back_as_projected(dev):
    graph, want = _case("zero_drift")
    projected = _run(graph, dev, steps=0)[0]
    o64, o32, res = _run(graph, dev)
    assert np.array_equal(projected, R.project(graph[0])), "half turns and dyadic translations project exactly"
    assert o64.tobytes() == projected.tobytes() and np.array_equal(o32, graph[0])
    assert res[0] == 0.0 and res[1] == 0.0 and int(res[2]) == 3 and int(res[4]) == 0
    assert int(res[6]) == _lib.POSEGRAPH_NAN_QUALITY == R.STATUS_NAN_QUALITY and res[5] == want["radius"]
    graph, want = _case("lonely_node")
    last = len(graph[0]) - 1
    assert int(np.max(graph[1])) < last
    projected = _run(graph, dev, steps=0)[0]
    o64 = _run(graph, dev)[0]
    assert o64[last].tobytes() == projected[last].tobytes() and o64[0].tobytes() == projected[0].tobytes()
    assert not np.array_equal(o64[1], projected[1])


def test_float64_inputs_are_read_as_float64(dev):
    graph, want = _case("chain12_64")
    assert graph[0].dtype == np.float64 and not np.array_equal(graph[0], graph[0].astype(np.float32))
    o64 = _run(graph, dev)[0]
    assert np.all(np.abs(o64 - want["anchors"]) <= 1e-9 * _scale(want["anchors"]))
    rounded = R.optimize(graph[0].astype(np.float32), graph[1], graph[2].astype(np.float32), graph[3])
    assert np.abs(o64 - rounded["anchors"]).max() > 1e-9


# ------------------------------------------------------------------------------------------------------------- determinism
def test_two_calls_give_the_same_bytes(dev):
    for name in ("chain8_loop0", "ws21", "reject3"):
        a, b = _run(_case(name)[0], dev), _run(_case(name)[0], dev)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


def test_captured_call_replays_on_new_inputs(dev):
    """one capture of the 8-node launch, replayed after the inputs were overwritten in place: equal to the eager results"""
    g1 = _case("chain8_loop0")[0]
    g2 = R.chain_graph(8, drift=0.35, seed=33, weight=1.0)
    assert g1[1].shape == g2[1].shape
    eager = [_run(g, dev) for g in (g1, g2)]
    bufs = _upload(g1, dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        out = pg.pose_graph_enqueue(*bufs)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        pg.pose_graph_enqueue(*bufs, out=out)
    for g, want in ((g2, eager[1]), (g1, eager[0]), (g2, eager[1])):
        for dst, src in zip(bufs, _upload(g, dev)):
            dst.copy_(src)
        for o in out[:3]:
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in out[:3]]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw_call(dev, n_nodes, n_edges):
    """mipsf_posegraph_optimize with sizes of the caller's choice over buffers that are large enough for any accepted size"""
    X = torch.eye(4, device=dev).repeat(80, 1, 1).contiguous()
    e = torch.tensor([[0, 1]], dtype=torch.int32, device=dev).repeat(1100, 1).contiguous()
    o = torch.eye(4, device=dev).repeat(1100, 1, 1).contiguous()
    w = torch.ones(1100, dtype=torch.float64, device=dev)
    o64, o32 = torch.zeros(80, 4, 4, dtype=torch.float64, device=dev), torch.zeros(80, 4, 4, device=dev)
    res = torch.zeros(8, dtype=torch.float64, device=dev)
    ws = torch.zeros(int(_lib.lib().mipsf_posegraph_workspace_bytes(64, 1024)) // 8, dtype=torch.float64, device=dev)
    a = _lib.PosegraphArgs.new(n_nodes=n_nodes, n_edges=n_edges, input_f64=0, anchors=X.data_ptr(), edges=e.data_ptr(),
                               observations=o.data_ptr(), weights=w.data_ptr(), steps=10, patience=3, max_rejects=16, decreasing=1e-3,
                               radius=1e4, min_diag=1e-6, anchors_out=o64.data_ptr(), anchors_out32=o32.data_ptr(),
                               result=res.data_ptr(), workspace=ws.data_ptr())
    rc = _lib.lib().mipsf_posegraph_optimize(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, (_lib.lib().mipsf_last_error() or b"").decode(), res.cpu()


def test_refusals(dev):
    assert _lib.lib().mipsf_posegraph_workspace_bytes(65, 10) == 0 and _lib.lib().mipsf_posegraph_workspace_bytes(10, 1025) == 0
    assert _lib.lib().mipsf_posegraph_workspace_bytes(1, 1) == 0 and _lib.lib().mipsf_posegraph_workspace_bytes(64, 1024) > 0
    for n, e, word in ((65, 10, "65 nodes"), (10, 1025, "1025 edges"), (1, 1, "1 nodes"), (2, 0, "0 edges")):
        rc, msg, res = _raw_call(dev, n, e)
        assert rc != 0 and word in msg and not res.any(), (n, e, msg)
    assert _raw_call(dev, 64, 1024)[0] == 0
    X, e, o, w = _case("chain8_loop0")[0]
    for bad in ([3, 3], [2, 8], [-1, 2]):
        e2 = e.copy()
        e2[4] = bad
        o64, o32, res = _run((X, e2, o, w), dev)
        assert int(res[6]) == _lib.POSEGRAPH_BAD_EDGE and int(res[2]) == 0 and np.array_equal(o64, _run((X, e, o, w), dev, steps=0)[0])
    Xt = torch.from_numpy(X)
    eye = torch.eye(4)
    with pytest.raises(ValueError, match="itself"):
        pg.pose_graph_optimize(Xt, [[0, 1], [2, 2]], eye, eye, 7, 0)
    with pytest.raises(ValueError, match="outside"):
        pg.pose_graph_optimize(Xt, [[0, 1], [1, 8]], eye, eye, 7, 0)
    with pytest.raises(ValueError, match="nodes"):
        pg.pose_graph_optimize(torch.eye(4).repeat(65, 1, 1), [[0, 1]], eye, eye, 1, 0)
    with pytest.raises(ValueError, match="edges"):
        pg.pose_graph_optimize(Xt, [[0, 1]] * 1024, eye, eye, 7, 0)
    mirrored = Xt.clone()
    mirrored[3, :3, 0] *= -1.0                                              # determinant -1
    with pytest.raises(ValueError, match="determinant"):
        pg.pose_graph_optimize(mirrored, [[0, 1]], eye, eye, 7, 0)


def test_out_of_another_size_is_refused(dev):
    """`out` of a call with a smaller N or E, or a short workspace, would be written past its end: refused on the host"""
    small = pg.pose_graph_enqueue(*_upload(_case("chain3")[0], dev))
    with pytest.raises(ValueError, match="`out` holds"):
        pg.pose_graph_enqueue(*_upload(_case("chain8_loop0")[0], dev), out=small)
    bufs = _upload(_case("ws21")[0], dev)
    out = pg.pose_graph_enqueue(*bufs)
    with pytest.raises(ValueError, match="workspace"):
        pg.pose_graph_enqueue(*bufs, out=out[:3] + (out[3][:-1],))
    again = pg.pose_graph_enqueue(*bufs, out=tuple(o.clone() for o in out))
    assert all(torch.equal(a, b) for a, b in zip(again[:3], out[:3]))


def test_pose_graph_optimize_is_the_reference_call(dev):
    """pairs + the two local poses -> edges as PoseCorrector.py:186-201 builds them -> the restatement on those edges"""
    rng = np.random.default_rng(4)
    X = R.chain_graph(6, seed=17)[0]
    pairs, part = pg.adjacent_pairs([[0, -1], [1, 0], [2, 1], [3, 2], [4, 3], [5, 4], [0, 5]])
    assert pg.global_ba_gate(part, 6)
    prev = R.random_pose(rng, 0.4, 1.0)
    aft = R.rigid_inverse(R.project(X)[0]) @ R.project(X)[5] @ prev @ R.random_pose(rng, 0.08, 0.1)
    got = pg.pose_graph_optimize(torch.from_numpy(X), pairs, torch.from_numpy(prev), torch.from_numpy(aft), id_prev=5, id_aft=0)
    e, o, w = pg.build_edges(torch.from_numpy(X), pairs, torch.from_numpy(prev), torch.from_numpy(aft), 5, 0, 0.1)
    want = R.optimize(X.astype(np.float64), e.numpy(), o.numpy(), w.numpy())
    assert e[-1].tolist() == [0, 5] and R.plateau_margin(want) > 1e-6
    assert np.all(np.abs(got.anchors.numpy() - want["anchors"]) <= 1e-9 * _scale(want["anchors"]))
    assert (got.steps, got.rejections, got.status) == (want["steps"], want["rejections"], want["status"])
    assert abs(got.first_loss - want["first_loss"]) <= 1e-9 * want["first_loss"] and got.loss < got.first_loss
    moved = pg.rebase(torch.from_numpy(R.project(X)), torch.arange(6), torch.from_numpy(R.project(X)), got.anchors)
    assert float((moved - got.anchors).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------------------- the runner
def _walk(dev, flag):
    from mipsfusion_amd import sequence
    from mipsfusion_amd.graph import work_stream

    from .test_gpu_sequence import _small_two_room_cfg
    cfg = _small_two_room_cfg()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    gt, frames, _ = synth.two_room_sequence(cfg, 40, kf_every=5)
    gt, frames = gt[:26], frames[:26]                                       # the shortest walk that holds the back switch
    schedule = {10: ("new",), 25: ("back", 0)}
    prev = torch.cuda.current_stream(dev)
    try:
        seq = sequence.GraphedSequence(cfg, dev, frames, kf_every=5, sampler="device", stream=work_stream(dev), schedule=schedule,
                                       deterministic=True, **({"pose_graph": True} if flag else {}))
        res = seq.run(gt)
    finally:
        torch.cuda.set_stream(prev)
    return seq, res


def test_runner_records_the_pose_graph_of_a_back_switch(dev):
    seq, res = _walk(dev, True)
    _, plain = _walk(dev, False)
    assert len(res["est"]) == len(plain["est"]) == 26
    assert all(torch.equal(a, b) for a, b in zip(res["est"], plain["est"])), "the pose graph moved the runner's state"
    assert plain["pose_graph"] == [] and len(res["pose_graph"]) == 1 and res["pose_graph"] == seq.pose_graphs
    rec = res["pose_graph"][0]
    assert rec["pairs"].tolist() == [[0, 1]] and (rec["id_prev"], rec["id_aft"]) == (1, 0) and rec["anchors"].shape == (2, 4, 4)
    for anchor, frame in zip(rec["anchors"], (0, 10)):                      # through the keyframe table's quaternions
        assert float((anchor - res["est"][frame].float()).abs().max()) < 1e-5
    want = pg.pose_graph_optimize(rec["anchors"], rec["pairs"], rec["local_pose_prev"], rec["local_pose_after"], rec["id_prev"],
                                  rec["id_aft"], rec["key_edge_weight"])
    got = rec["result"]
    print("pose graph of the back switch:", got.first_loss, "->", got.loss, "steps", got.steps, "rejections", got.rejections)
    assert torch.equal(got.anchors, want.anchors) and got[1:] == want[1:]
    assert got.status == 0 and got.loss <= got.first_loss and float((got.anchors[0] - rec["anchors"][0].double()).abs().max()) < 1e-6
