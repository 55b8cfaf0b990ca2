"""Closing a loop: the pose graph over the first-keyframe ("anchor") poses of all sub-maps (upstream: InactiveMap.global_BA ->
PoseCorrector.pose_graph_optimize -> model/poseGraph.py, a Levenberg-Marquardt optimisation run through pypose on the host).
Here the whole optimisation -- projection of the rotations, every step, every rejection, the stop -- is ONE launch of
``csrc/posegraph.hip`` (C ABI: include/mipsf_posegraph.h; DESIGN.md 4.15 states what it computes):

    adjacent_pairs       keyframeSet.find_adjacent_localMLP_pair from the keyframe -> sub-map binding table
    global_ba_gate       InactiveMap.py:484-488
    build_edges          PoseCorrector.py:186-201
    pose_graph_enqueue   the launch: device tensors in, device tensors out, no check, no synchronisation, capturable
    pose_graph_optimize  PoseCorrector.pose_graph_optimize on top of them; one read-back when it has finished
    rebase               anchors_new anchors_old^-1 applied to world poses (trajectories, SubMap poses before extract_scene_mesh)

No pypose version is pinned upstream and none is installed here; tests/posegraph_cpu.py is the float64 restatement the kernel is
held to.  The same call gives the same bytes.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib

MIN_DIAG, MAX_REJECTS = 1e-6, 16        # pypose LM(min=1e-6, reject=16)


class PoseGraphResult(NamedTuple):
    anchors: torch.Tensor               # float64 [N,4,4], CPU
    first_loss: float
    loss: float
    steps: int
    rejections: int
    status: int                         # _lib.POSEGRAPH_FACTORISATION_FAILED | POSEGRAPH_NAN_QUALITY; POSEGRAPH_BAD_EDGE from
                                        # pose_graph_enqueue alone: pose_graph_optimize raises on it


# --------------------------------------------------------------------------------------------------------------- host helpers
def adjacent_pairs(keyframe_submaps):
    """keyframe_submaps: [n_kf,2] the sub-maps each keyframe is bound to, -1 for none (keyframeSet.keyframe_localMLP).  A keyframe
    bound to two sub-maps makes them adjacent (Manager.py:546,595 -> add_adjcent_pair).  -> (pairs int32 [k,2], every row (i, j)
    with i < j, rows in ascending (i, j); participants int64 [m] ascending), as find_adjacent_localMLP_pair returns them."""
    t = torch.as_tensor(keyframe_submaps, dtype=torch.int64).reshape(-1, 2)
    both = t[(t[:, 0] >= 0) & (t[:, 1] >= 0) & (t[:, 0] != t[:, 1])]
    found = sorted({(int(min(a, b)), int(max(a, b))) for a, b in both.tolist()})
    pairs = torch.tensor(found, dtype=torch.int32).reshape(-1, 2)
    return pairs, torch.unique(pairs.to(torch.int64))


def global_ba_gate(participants, n_submaps: int) -> bool:
    """InactiveMap.py:484-488: at least two sub-maps take part in some pair, and all sub-maps take part"""
    m = int(torch.as_tensor(participants).numel())
    return m >= 2 and m == int(n_submaps)


def build_edges(anchors, pairs, local_pose_prev, local_pose_after, id_prev, id_aft, key_edge_weight):
    """PoseCorrector.py:186-201 in float64 -> (edges int32 [k+1,2], observations float64 [k+1,4,4], weights float64 [k+1]).
    Every adjacent pair (i, j): edge (i, j) observed as X_j^-1 X_i of the current anchors, weight 1; last the key edge
    (id_aft, id_prev) observed as local_pose_prev @ local_pose_after^-1, weight key_edge_weight."""
    X = torch.as_tensor(anchors).detach().to("cpu", torch.float64)
    pairs = torch.as_tensor(pairs).to("cpu", torch.int64).reshape(-1, 2)
    prev = torch.as_tensor(local_pose_prev).detach().to("cpu", torch.float64)
    aft = torch.as_tensor(local_pose_after).detach().to("cpu", torch.float64)
    obs = [torch.linalg.inv(X[j]) @ X[i] for i, j in pairs.tolist()]
    obs.append(prev @ torch.linalg.inv(aft))
    edges = torch.cat([pairs, torch.tensor([[int(id_aft), int(id_prev)]], dtype=torch.int64)]).to(torch.int32)
    weights = torch.cat([torch.ones(len(pairs), dtype=torch.float64), torch.tensor([float(key_edge_weight)], dtype=torch.float64)])
    return edges, torch.stack(obs), weights


def check_rotations(poses, what: str, tol: float = 1e-5) -> None:
    """mat2SE3(check=True): R R^T = I and det R = 1 to rtol = atol = 1e-5, else ValueError"""
    R = torch.as_tensor(poses).detach().to("cpu", torch.float64)[..., :3, :3]
    eye = torch.eye(3, dtype=torch.float64).expand_as(R)
    if not torch.allclose(R @ R.transpose(-1, -2), eye, rtol=tol, atol=tol):
        raise ValueError(f"{what}: rotation matrices are not all orthogonal")
    if not torch.allclose(torch.linalg.det(R), torch.ones(R.shape[:-2], dtype=torch.float64), rtol=tol, atol=tol):
        raise ValueError(f"{what}: rotation matrices' determinants are not all 1")


def check_graph(n_nodes: int, edges) -> None:
    """what mipsf_posegraph_optimize refuses, before anything is uploaded"""
    e = torch.as_tensor(edges).to("cpu", torch.int64).reshape(-1, 2)
    if not 2 <= n_nodes <= _lib.POSEGRAPH_MAX_NODES:
        raise ValueError(f"pose graph: {n_nodes} nodes, accepted are 2 .. {_lib.POSEGRAPH_MAX_NODES}")
    if not 1 <= len(e) <= _lib.POSEGRAPH_MAX_EDGES:
        raise ValueError(f"pose graph: {len(e)} edges, accepted are 1 .. {_lib.POSEGRAPH_MAX_EDGES}")
    if bool((e[:, 0] == e[:, 1]).any()):
        raise ValueError("pose graph: an edge joins a node to itself")
    if int(e.min()) < 0 or int(e.max()) >= n_nodes:
        raise ValueError(f"pose graph: an edge names a node outside 0 .. {n_nodes - 1}")


def rebase(poses_world, submap_of_pose, anchors_old, anchors_new):
    """World poses after the anchors moved: pose k of sub-map s becomes X_new[s] X_old[s]^-1 W_k (its pose relative to the anchor
    is kept).  For trajectories, and for ``SubMap(first_kf_c2w=..., kf_c2w=...)`` before ``extract_scene_mesh``.  float64."""
    W = torch.as_tensor(poses_world).detach().to(torch.float64)
    s = torch.as_tensor(submap_of_pose).to(torch.int64).reshape(-1).to(W.device)
    old = torch.as_tensor(anchors_old).detach().to(W.device, torch.float64)
    new = torch.as_tensor(anchors_new).detach().to(W.device, torch.float64)
    return (new @ torch.linalg.inv(old))[s] @ W


# --------------------------------------------------------------------------------------------------------------- the launch
def pose_graph_enqueue(anchors, edges, observations, weights, steps=10, patience=3, decreasing=1e-3, radius=1e4,
                       min_diag=MIN_DIAG, max_rejects=MAX_REJECTS, out=None):
    """-> (anchors float64 [N,4,4], anchors float32 [N,4,4], result float64 [8] = first loss | last loss | steps done | solves |
    rejections | final radius | status bits | 0), all on the device.  anchors [N,4,4] and observations [E,4,4]: both float32 or
    both float64; edges int32 [E,2]; weights float64 [E]; contiguous device tensors.  Nothing is checked beyond shapes and sizes,
    nothing is read back and nothing synchronises: the call can be recorded into a graph and replayed on new values (pass the
    tuple a first call returned as ``out`` to keep the outputs in place; the workspace travels with it)."""
    N, E = anchors.shape[0], edges.shape[0]
    if tuple(anchors.shape[1:]) != (4, 4) or tuple(observations.shape) != (E, 4, 4) or tuple(edges.shape) != (E, 2) or tuple(weights.shape) != (E,):
        raise ValueError("pose graph: anchors [N,4,4], edges [E,2], observations [E,4,4], weights [E]")
    if anchors.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"pose graph: anchors are {anchors.dtype}, expected float32 or float64")
    dev = anchors.device
    need = int(_lib.lib().mipsf_posegraph_workspace_bytes(N, E))
    if need == 0:
        raise RuntimeError(f"pose graph: {N} nodes / {E} edges, accepted are 2 .. {_lib.POSEGRAPH_MAX_NODES} nodes and "
                           f"1 .. {_lib.POSEGRAPH_MAX_EDGES} edges")
    if out is None:
        out = (torch.empty(N, 4, 4, dtype=torch.float64, device=dev), torch.empty(N, 4, 4, dtype=torch.float32, device=dev),
               torch.empty(_lib.POSEGRAPH_RESULT_DOUBLES, dtype=torch.float64, device=dev),
               torch.empty((need + 7) // 8, dtype=torch.float64, device=dev))
    out64, out32, result, ws = out
    # a tuple from a call with another N or E would be written past its end: sizes only, nothing here reads the device
    for t, shape, dtype in ((out64, (N, 4, 4), torch.float64), (out32, (N, 4, 4), torch.float32),
                            (result, (_lib.POSEGRAPH_RESULT_DOUBLES,), torch.float64)):
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise ValueError(f"pose graph: `out` holds {tuple(t.shape)} {t.dtype} on {t.device}, this call writes {shape} {dtype} on {dev}")
    if ws.dtype != torch.float64 or ws.device != dev or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise ValueError(f"pose graph: the workspace of `out` has {ws.numel() * ws.element_size()} bytes on {ws.device}, "
                         f"{N} nodes / {E} edges need {need} of float64 on {dev}")
    a =_lib.PosegraphArgs.new(n_nodes=N, n_edges=E, input_f64=int(anchors.dtype == torch.float64),
                               anchors=_lib.dptr(anchors, anchors.dtype), edges=_lib.dptr(edges, torch.int32),
                               observations=_lib.dptr(observations, anchors.dtype), weights=_lib.dptr(weights, torch.float64),
                               steps=int(steps), patience=int(patience), max_rejects=int(max_rejects), decreasing=float(decreasing),
                               radius=float(radius), min_diag=float(min_diag), anchors_out=_lib.dptr(out64, torch.float64),
                               anchors_out32=_lib.dptr(out32), result=_lib.dptr(result, torch.float64), workspace=ws.data_ptr())
    _lib.check(_lib.lib().mipsf_posegraph_optimize(C.byref(a), _lib.stream_ptr()), "posegraph_optimize")
    return out


def pose_graph_optimize(anchors, pairs, local_pose_prev, local_pose_after, id_prev, id_aft, key_edge_weight=0.1, steps=10, patience=3,
                        decreasing=1e-3, radius=1e4, device=None) -> PoseGraphResult:
    """PoseCorrector.pose_graph_optimize: anchors [N,4,4] (float32 or float64, camera -> world, anchor 0 stays), pairs [k,2] from
    ``adjacent_pairs``, the overlapping keyframe's pose in the sub-map left (``local_pose_prev``, sub-map id_prev) and in the
    sub-map re-entered (``local_pose_after``, sub-map id_aft).  Rotations must be orthonormal with determinant 1 to 1e-5
    (ValueError otherwise, as mat2SE3(check=True)).  Edges are built and uploaded in float64 whatever the anchors' type.
    The defaults are the reference's: key_edge_weight of its configurations,
    StopOnPlateau(steps=10, patience=3, decreasing=1e-3), TrustRegion(radius=1e4)."""
    anchors = torch.as_tensor(anchors)
    check_graph(anchors.shape[0], torch.cat([torch.as_tensor(pairs).to("cpu", torch.int64).reshape(-1, 2),
                                             torch.tensor([[int(id_aft), int(id_prev)]], dtype=torch.int64)]))
    edges, obs, w = build_edges(anchors, pairs, local_pose_prev, local_pose_after, id_prev, id_aft, key_edge_weight)
    check_rotations(anchors, "anchors")
    check_rotations(obs, "observations")
    dev = torch.device(device) if device is not None else (anchors.device if anchors.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(dev):
        out64, _, result, _ = pose_graph_enqueue(anchors.detach().to(dev, torch.float64).contiguous(), edges.to(dev), obs.to(dev).contiguous(),
                                                 w.to(dev), steps, patience, decreasing, radius)
        r = result.cpu()                                            # the one read-back
        X = out64.cpu()
    status = int(r[6])
    if status & _lib.POSEGRAPH_BAD_EDGE:
        raise RuntimeError("pose graph: the kernel refused an edge")
    return PoseGraphResult(X, float(r[0]), float(r[1]), int(r[2]), int(r[4]), status)
