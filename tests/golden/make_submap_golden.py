#!/usr/bin/env python3
"""Records the sub-map manager's fixtures tests/golden/submap/*.npz from the upstream's own ``Manager`` and ``KeyframeSet``.

usage (from the repository root, where the upstream tree is present): python tests/golden/make_submap_golden.py

The upstream classes are imported behind ``oracle.ref_import.load()`` and run on the CPU against a stand-in for the SLAM object
(``dataset.H/W/fx/fy/cx/cy``, ``kf_c2w``, ``est_c2w_data``, ``keyframe_ref``, ``active_localMLP_Id``, ``prev_active_localMLP_Id``,
``overlap_kf_flag``, ``rectified_local_pose``, ``current_pose_switch_submap``) and for ``poseCorrector.switch_pose_rectifying``
(accepts or rejects, hands the initial pose back).  Frames are NOT written: the tests render them again with ``synth``
(tests/submap_fixtures.py).  Written are the settings, the constructed state before the call, and what upstream did.

branch_*   one frame + a state constructed relative to the frame's own points, one ``process_keyframe`` call, one branch.
           Anchors of sub-maps are pure translations, so upstream's float32 ``first_kf_pose @ pose_local`` is exact whatever the
           order of its sums (its 4x4 product goes through a BLAS whose fused multiply-adds differ from a plain restatement).
walk_*     the 300-frame two-room walk; upstream's ``convert_pose_to_world`` is handed the walk's world pose for the same reason
           (``derive_schedule`` has the world poses too and passes them on).
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import                                   # noqa: E402
import submap_fixtures as sf                                      # noqa: E402
from mipsfusion_amd import submap_cpu as sc, synth               # noqa: E402

F32 = np.float32
N_KF, N_FRAMES = 32, 512


class Reference:
    """upstream's Manager over a stand-in SLAM object"""

    def __init__(self, cfg, accept=True, world_of_frame=None):
        ref_import.load()
        import Manager as manager_module
        from model.keyframeSet import KeyframeSet
        from helper_functions.geometry_helper import extract_first_kf_pose
        self.cfg, self.every = cfg, cfg["mapping"]["keyframe_every"]
        fx, fy, cx, cy = sf.INTRINSICS
        slam = types.SimpleNamespace(device="cpu", dataset=types.SimpleNamespace(H=sf.H, W=sf.W, fx=fx, fy=fy, cx=cx, cy=cy))
        slam.kfSet = KeyframeSet(cfg, sf.H, sf.W, N_KF, "cpu")
        slam.kf_c2w = torch.zeros(N_KF, 4, 4)
        slam.est_c2w_data = torch.zeros(N_FRAMES, 4, 4)
        slam.keyframe_ref = torch.full((N_KF,), -3, dtype=torch.int32)
        slam.overlap_kf_flag = torch.zeros(N_KF)
        slam.active_localMLP_Id = torch.zeros(1, dtype=torch.int64)
        slam.prev_active_localMLP_Id = torch.full((1,), -1, dtype=torch.int64)
        slam.rectified_local_pose = torch.eye(4).unsqueeze(0)
        self.rectify_calls = []

        def current_pose_switch_submap(frame_Id, keyframe_Id, prev_id=None, active_id=None):   # mipsfusion.py:589-603
            first_prev = extract_first_kf_pose(prev_id, slam.kfSet.localMLP_first_kf, slam.kf_c2w)
            first_aft = extract_first_kf_pose(active_id, slam.kfSet.localMLP_first_kf, slam.kf_c2w)
            return first_aft.inverse() @ (first_prev @ slam.est_c2w_data[frame_Id]), slam.est_c2w_data[frame_Id].clone()
        slam.current_pose_switch_submap = current_pose_switch_submap

        def switch_pose_rectifying(batch, pose_ini, pose_bf, id_aft, id_prev, kf_ids, masks):
            self.rectify_calls.append((pose_ini.clone(), kf_ids.clone(), masks.clone()))
            return accept, 1234, pose_ini.clone()
        slam.poseCorrector = types.SimpleNamespace(switch_pose_rectifying=switch_pose_rectifying)
        self.slam = slam
        self.m = manager_module.Manager(cfg, slam)
        self.ratios, self.overlap, self.surface = [], None, None
        inner_cr, inner_ovlp = self.m.compute_containing_ratio, self.m.find_overlapping_region

        def compute_containing_ratio(*a, **k):
            r = inner_cr(*a, **k)
            self.ratios.append(("cr_active_new" if k.get("localMLP_center") is not None else None, r.numpy().copy()))
            return r

        def find_overlapping_region(*a, **k):
            self.overlap_target = int(a[3])
            self.overlap = inner_ovlp(*a, **k)
            return self.overlap
        self.m.compute_containing_ratio, self.m.find_overlapping_region = compute_containing_ratio, find_overlapping_region
        if world_of_frame is not None:
            self.m.convert_pose_to_world = lambda pose_local, submap: world_of_frame[self.frame_id].clone()

    def load_state(self, st):
        k, s, n_sub, n_kf = self.slam.kfSet, self.slam, len(st["boxes"]), len(st["keyframe_ref"])
        size = max(self.cfg["mapping"]["localMLP_num"], n_sub)
        k.localMLP_info = torch.zeros(size, 7)
        k.localMLP_info[:n_sub, 0] = 1
        k.localMLP_info[:n_sub, 1:] = torch.from_numpy(st["boxes"])
        k.localMLP_max_len = torch.tensor(self.cfg["mapping"]["localMLP_max_len"])[None].repeat(size, 1)
        k.localMLP_max_len[:n_sub] = torch.from_numpy(st["max_len"])
        k.localMLP_adjacent = torch.zeros(size, size)
        for a, b in st["adjacent"]:
            k.localMLP_adjacent[a, b] = k.localMLP_adjacent[b, a] = 1
        k.localMLP_first_kf = torch.full((size,), -1)
        k.localMLP_first_kf[:n_sub] = torch.from_numpy(st["first_kf"])
        k.keyframe_localMLP[:] = -1
        k.keyframe_localMLP[:n_kf] = torch.from_numpy(st["keyframe_submaps"])
        k.collected_kf_num[0] = n_kf
        k.rays[:n_kf] = torch.from_numpy(st["table"])
        k.frame_ids = torch.arange(n_kf).float() * self.every
        s.keyframe_ref[:] = -3
        s.keyframe_ref[:n_kf] = torch.from_numpy(st["keyframe_ref"])
        s.kf_c2w[:n_kf] = torch.from_numpy(st["kf_world"])
        for kf in range(n_kf):
            s.est_c2w_data[kf * self.every] = torch.from_numpy(st["kf_local"][kf])
        sca = [int(v) for v in st["scalars"]]
        s.active_localMLP_Id[0], s.prev_active_localMLP_Id[0] = sca[0], sca[1]
        m = self.m
        m.double_binding_counter, m.db_active_localMLP_Id, m.db_mo_localMLP_Id = sca[2], sca[3], sca[4]
        m.wait_loop, m.localMLP_Id_wait, m.localMLP_Id_actual = bool(sca[5]), sca[6], sca[7]

    def dump_state(self):
        k, s, m = self.slam.kfSet, self.slam, self.m
        n_sub, n_kf = int(torch.count_nonzero(k.localMLP_info[:, 0])), int(k.collected_kf_num[0])
        adj = sorted((i, j) for i in range(n_sub) for j in range(i + 1, n_sub) if k.localMLP_adjacent[i, j] > 0)
        return {"boxes": k.localMLP_info[:n_sub, 1:].numpy().copy(), "max_len": k.localMLP_max_len[:n_sub].numpy().copy(),
                "first_kf": k.localMLP_first_kf[:n_sub].numpy().astype(np.int64), "adjacent": np.asarray(adj, np.int64).reshape(-1, 2),
                "keyframe_submaps": k.keyframe_localMLP[:n_kf].numpy().astype(np.int64), "keyframe_ref": s.keyframe_ref[:n_kf].numpy().copy(),
                "kf_world": s.kf_c2w[:n_kf].numpy().copy(),
                "kf_local": np.stack([s.est_c2w_data[kf * self.every].numpy() for kf in range(n_kf)]),
                "scalars": np.asarray([int(s.active_localMLP_Id[0]), int(s.prev_active_localMLP_Id[0]), int(m.double_binding_counter),
                                       int(m.db_active_localMLP_Id), int(m.db_mo_localMLP_Id), int(m.wait_loop), int(m.localMLP_Id_wait),
                                       int(m.localMLP_Id_actual)], np.int64),
                "table": k.rays[:n_kf].numpy().copy()}

    def process(self, frame, pose_local, frame_id, force):
        """mipsfusion.py:686-709 around one keyframe -> (flag, label)"""
        s, self.frame_id = self.slam, frame_id
        kf = frame_id // self.every
        batch = {"frame_id": frame_id, "depth": frame["depth"][None], "direction": frame["direction"][None], "rgb": frame["rgb"][None]}
        s.kfSet.add_keyframe(batch)
        s.est_c2w_data[frame_id] = torch.as_tensor(pose_local, dtype=torch.float32)
        self.ratios, self.overlap, waited = [], None, bool(self.m.wait_loop)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            flag = self.m.process_keyframe(batch, s.active_localMLP_Id[0].clone(), s.est_c2w_data[frame_id].clone(), frame_id, kf, force=force)
        if flag == 1:
            s.est_c2w_data[frame_id] = s.rectified_local_pose[0].clone()
        s.kfSet.collected_kf_num[0] = s.kfSet.collected_kf_num[0] + 1
        text = out.getvalue()
        label = text[text.rindex("-- (") + 4:text.rindex(")")]
        names, named = (["cr_wait"] if waited else []) + ["cr_mo", "cr_active"], {}
        for tag, value in self.ratios:
            named[tag or names.pop(0)] = value
        return int(flag), label, named, kf


def translation(x, y, z):
    m = np.eye(4, dtype=F32)
    m[:3, 3] = (x, y, z)
    return m


def local_pose(yaw, pitch, t):
    m = np.eye(4, dtype=F32)
    m[:3, :3] = synth.look_rotation(yaw, pitch).numpy()
    m[:3, 3] = t
    return m


A = [translation(0.25, 0.0, 0.5), translation(-0.5, 0.25, -0.25), translation(0.5, -0.25, 0.75)]


def product(a, b):
    return (torch.from_numpy(a) @ torch.from_numpy(b)).numpy()


def cloud(frame, pose_world, far):
    rows = sf.rows_of(frame).numpy()
    return sc.world_points(rows[(rows[:, 6] > 0) & (rows[:, 6] < far)], pose_world)


def span_box(pts, x_range=None, scale=1.2, axis=0):
    """a box around the points, scaled about their centre; the range along ``axis`` replaced by (lo, hi) where given"""
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    c, l = (lo + hi) / 2, (hi - lo) * scale
    if x_range is not None:
        c[axis], l[axis] = (x_range[0] + x_range[1]) / 2, x_range[1] - x_range[0]
    return np.concatenate([c, l]).astype(F32)


def keyframe_entry(bind, ref, anchor, local, seed):
    world = product(anchor, local)
    rows = sf.rows_of(sf.box_frame(world, seed, 0)).numpy()
    return {"bind": bind, "ref": ref, "world": world if ref == -1 else np.zeros((4, 4), F32), "local": local,
            "rows": rows[sc.lattice_pixels(sf.H, sf.W, 12, 16)]}


def make_state(boxes, max_len, first_kf, adjacent, kfs, active, prev, counter=0, db=(-1, -1), wait=(0, -1, -1)):
    return {"boxes": np.asarray(boxes, F32).reshape(-1, 6), "max_len": np.asarray(max_len, F32).reshape(-1, 3),
            "first_kf": np.asarray(first_kf, np.int64), "adjacent": np.asarray(adjacent, np.int64).reshape(-1, 2),
            "keyframe_submaps": np.asarray([k["bind"] for k in kfs], np.int64), "keyframe_ref": np.asarray([k["ref"] for k in kfs], np.int32),
            "kf_world": np.stack([k["world"] for k in kfs]), "kf_local": np.stack([k["local"] for k in kfs]),
            "scalars": np.asarray([active, prev, counter, db[0], db[1], wait[0], wait[1], wait[2]], np.int64),
            "table": np.stack([k["rows"] for k in kfs])}


def margins(cfg, state, fx_pose_world, frame, overlap, active, target):
    """float64 margins of an overlap fixture: no projected point within 1e-3 px of an edge bound, no camera depth within 1e-6 of
    0, consecutive ranking distances differ by more than 1e-4 where more than ten keyframes are related"""
    m = sf.SubmapManager(cfg, sf.H, sf.W, sf.INTRINSICS, rectify=lambda *a: (False, 0, None), backend="cpu", max_keyframes=N_KF)
    m.load_state(state)
    kf_ids = overlap[4].numpy()
    if len(kf_ids) == 0:                                  # no related keyframe: nothing is projected
        return
    kfs = m.keyframe_submaps[:m.n_keyframes]
    related = np.nonzero((kfs == target).any(1) & ~(kfs == active).any(1))[0]
    lat = (cfg["mapping"]["overlapping"]["n_rays_h"], cfg["mapping"]["overlapping"]["n_rays_w"])
    pts = sc.world_points(sf.rows_of(frame).numpy()[sc.lattice_pixels(sf.H, sf.W, *lat)], fx_pose_world)
    if len(related) > 10:
        dist = np.sort(sc.overlap_distances(sf.rows_of(frame).numpy(), fx_pose_world, sf.H, sf.W, lat, m.table, related,
                                            m.keyframe_world_poses(related)))
        assert np.diff(dist).min() > 1e-4, "two ranking distances differ by less than 1e-4"
    cam = sc.overlap_camera_points(pts, m.keyframe_world_poses(kf_ids))
    u, v = sc.overlap_project(cam, *[float(x) for x in sf.INTRINSICS])
    for value, bounds in ((u, (20.0, cfg["cam"]["W"] - 20.0)), (v, (20.0, cfg["cam"]["H"] - 20.0))):
        for b in bounds:
            assert np.abs(value - b).min() > 1e-3, "a projected point lies within 1e-3 px of an edge bound"
    assert np.abs(cam[..., 2]).min() > 1e-6, "a camera depth lies within 1e-6 of 0"


def record_branch(name, cfg_over, state, pose_local, frame_id, seed, force=False, accept=True, x_case=None, axis=0):
    cfg = sf.config(cfg_over)
    ref = Reference(cfg, accept)
    ref.load_state(state)
    active = int(state["scalars"][0])
    pose_world = product(state["kf_world"][state["first_kf"][active]], pose_local)
    frame = sf.box_frame(pose_world, seed, frame_id)
    gh = ref_import.load().geometry_helper
    c, l = gh.get_frame_surface_bbox(torch.from_numpy(pose_world), frame["depth"], frame["direction"], cfg["cam"]["near"], cfg["cam"]["far"])
    if x_case is not None:                                # the expand rule's case on one axis of the active sub-map
        got = sc.case_of(sc.expand_rule(state["boxes"][active], np.concatenate([c.numpy(), l.numpy()]), state["max_len"][active])[1], axis)
        assert got == x_case, (name, got, x_case)
    flag, label, ratios, kf = ref.process(frame, pose_local, frame_id, force)
    after = ref.dump_state()
    out = {"spec": json.dumps({"cfg": cfg_over, "frame_id": frame_id, "seed": seed, "force": force, "accept": accept, "flag": flag,
                               "label": label}),
           "pose_local": pose_local, "pose_world": pose_world, "e_surface": np.concatenate([c.numpy(), l.numpy()]),
           "e_bindings": after["keyframe_submaps"][kf]}
    out.update({"s_" + k: v for k, v in state.items()})
    out.update({"e_" + k: v for k, v in after.items() if k != "table"})
    out.update({"e_" + k: v for k, v in ratios.items()})
    if ref.overlap is not None:
        switch, target_d, rays_d, mask_final, kf_ids, masks = ref.overlap
        margins(cfg, state, pose_world, frame, ref.overlap, active, ref.overlap_target)
        out.update(e_mask_final=mask_final.numpy(), e_top_kf_masks=masks.numpy(), e_kf_ids=kf_ids.numpy().astype(np.int64),
                   e_target_d=target_d.numpy(), e_rays_d_cam=rays_d.numpy(), e_rectify_calls=np.int64(len(ref.rectify_calls)),
                   e_rectified=ref.slam.rectified_local_pose[0].numpy().copy())
    np.savez_compressed(os.path.join(sf.GOLDEN, f"branch_{name}.npz"), **out)
    print(f"branch_{name}: flag {flag} ({label}); ratios { {k: float(v) for k, v in ratios.items()} }")
    return label, after


def branches():
    far = 5.0
    cur = local_pose(0.35, -0.08, [0.15, 0.0, -0.1])
    labels, cases = [], set()

    def points(anchor, local, seed, frame_id):
        world = product(anchor, local)
        return cloud(sf.box_frame(world, seed, frame_id), world, far)

    def quantile(pts, q, axis=0):
        return float(np.quantile(pts[:, axis].astype(np.float64), q))

    def note(box, pts, max_len):
        s_lo, s_hi = pts.min(0), pts.max(0)
        s_len = s_hi - s_lo
        cases.update(sc.case_of(sc.expand_rule(box, np.concatenate([s_lo + sc.HALF * s_len, s_len]), max_len)[1], a) for a in range(3))

    kf0 = keyframe_entry((0, -1), -1, A[0], np.eye(4, dtype=F32), 100)       # an anchor is its first keyframe's world pose
    big = [10.0, 10.0, 10.0]

    # one sub-map, the frame is keyframe 1
    p = points(A[0], cur, 1, 15)
    lo, hi = float(p[:, 0].min()) - 0.1, float(p[:, 0].max()) + 0.1

    def one(box, max_len):
        note(box, p, np.asarray(max_len, F32))
        return make_state([box], [max_len], [0], [], [kf0], 0, -1)
    labels.append(record_branch("unchanged", {}, one(span_box(p), big), cur, 15, 1)[0])
    labels.append(record_branch("expanded_free", {}, one(span_box(p, (lo, quantile(p, 0.5))), big), cur, 15, 1, x_case=2)[0])
    # the clamped cases cut the frame's points at the new face: the side that grows must not end on a wall (its points lie ON the
    # surface box's face), so the camera looks to the side whose far end is not a wall
    mirrored = local_pose(-0.35, -0.08, [0.15, 0.0, -0.1])
    views = [(cur, p), (mirrored, points(A[0], mirrored, 1, 15))]
    on_hi = [float(np.mean(q[:, 0] > q[:, 0].max() - 1e-3)) for _, q in views]
    pos_view, neg_view = (views[0], views[1]) if on_hi[0] < on_hi[1] else (views[1], views[0])
    for name, (pose, q), x_range, reach, case in (
            ("expanded_positive", pos_view, lambda q: (float(q[:, 0].min()) - 0.1, quantile(q, 0.5)), lambda q, r: quantile(q, 0.9) - r[0], 3),
            ("expanded_negative", neg_view, lambda q: (quantile(q, 0.5), float(q[:, 0].max()) + 0.1), lambda q, r: r[1] - quantile(q, 0.1), 4)):
        r = x_range(q)
        box, max_len = span_box(q, r), [reach(q, r), 10.0, 10.0]
        note(box, q, np.asarray(max_len, F32))
        label = record_branch(name, {}, make_state([box], [max_len], [0], [], [kf0], 0, -1), pose, 15, 1, x_case=case)[0]
        assert label == "expanded", (name, label)
        labels.append(label)
    # both sides at once, along y: the clamped faces fall short of floor and ceiling, whose points (a third of the frame) stay
    # outside, so this fixture asks for 0.6 of the frame
    labels.append(record_branch("expanded_both", {"mapping": {"min_containing_ratio": 0.6}}, one(span_box(p, (quantile(p, 0.3, 1), quantile(p, 0.7, 1)), axis=1),
                                                         [10.0, 0.97 * float(p[:, 1].max() - p[:, 1].min()), 10.0]), cur, 15, 1, x_case=5, axis=1)[0])
    assert labels[-1] == "expanded"
    small = span_box(p, (lo, quantile(p, 0.3)))
    tight = [float(small[3]) + 0.05, 10.0, 10.0]
    labels.append(record_branch("new_one_submap", {}, one(small, tight), cur, 15, 1)[0])
    labels.append(record_branch("force", {}, one(small, tight), cur, 15, 1, force=True)[0])

    # two sub-maps, active 0 again after a visit to 1; keyframe 2 is bound to sub-map 1 alone
    kf1 = keyframe_entry((1, 0), -1, A[1], np.eye(4, dtype=F32), 101)
    kf2 = keyframe_entry((1, -1), -3, A[1], local_pose(0.32, -0.09, [0.9, -0.2, 0.6]), 102)
    p = points(A[0], cur, 3, 45)
    lo = float(p[:, 0].min()) - 0.1
    small = span_box(p, (lo, quantile(p, 0.3)))
    tight = [float(small[3]) + 0.05, 10.0, 10.0]
    poor = span_box(p, (quantile(p, 0.6), float(p[:, 0].max()) + 0.1))
    note(small, p, np.asarray(tight, F32))
    labels.append(record_branch("new_poor_second", {}, make_state([small, poor], [tight, big], [0, 1], [(0, 1)], [kf0, kf1, kf2], 0, 1), cur, 45, 3)[0])
    both = make_state([span_box(p), span_box(p, scale=1.1)], [big, big], [0, 1], [(0, 1)], [kf0, kf1, kf2], 0, 1)
    labels.append(record_branch("double_binding_first", {}, both, cur, 45, 3)[0])
    both["scalars"][2:5] = (4, 0, 1)
    labels.append(record_branch("double_binding_switch", {}, both, cur, 45, 3, accept=True)[0])
    labels.append(record_branch("double_binding_rejected", {}, both, cur, 45, 3, accept=False)[0])

    # two sub-maps, active 1, the camera is back in the range of sub-map 0 (keyframes 0 and 1 belong to it alone)
    kf1 = keyframe_entry((0, -1), -3, A[0], local_pose(0.28, -0.1, [0.12, 0.02, -0.15]), 103)
    kf2 = keyframe_entry((1, 0), -1, A[1], np.eye(4, dtype=F32), 104)
    cur1 = product(translation(0.75, -0.25, 0.75), cur)                       # A[1]^-1 A[0] is the translation (0.75, -0.25, 0.75)
    p = points(A[1], cur1, 5, 45)
    lo = float(p[:, 0].min()) - 0.1
    small = span_box(p, (lo, quantile(p, 0.3)))
    tight = [float(small[3]) + 0.05, 10.0, 10.0]
    back = make_state([span_box(p), small], [big, tight], [0, 2], [(0, 1)], [kf0, kf1, kf2], 1, 0)
    labels.append(record_branch("switch_to_prev", {}, back, cur1, 45, 5, accept=True)[0])
    label, after = record_branch("wait_loop", {}, back, cur1, 45, 5, accept=False)
    labels.append(label)
    # the next keyframe, seen from the sub-map the wait loop opened (its anchor is the pose of keyframe 3, a rotation: the local
    # pose is the identity plus a translation along exact binary fractions, so the product stays exact)
    labels.append(record_branch("wait_loop_resolved", {}, after, np.eye(4, dtype=F32), 60, 6, accept=True)[0])

    assert set(labels) == set(sf.LABELS), (sorted(set(labels)), sorted(sf.LABELS))
    assert {3, 4, 5} <= cases, cases


def record_walk(name, cfg_over):
    cfg = sf.config(cfg_over)
    poses, frames = sf.walk(cfg)
    every = cfg["mapping"]["keyframe_every"]
    ref = Reference(cfg, True, world_of_frame=poses)
    # mipsfusion.first_frame_mapping
    gh = ref_import.load().geometry_helper
    c, l = gh.get_frame_surface_bbox(poses[0], frames[0]["depth"], frames[0]["direction"], cfg["cam"]["near"], cfg["cam"]["far"])
    first = keyframe_entry((0, -1), -1, np.eye(4, dtype=F32), np.eye(4, dtype=F32), 0)
    first["world"] = poses[0].numpy()
    first["rows"] = sf.rows_of(frames[0]).numpy()[sc.lattice_pixels(sf.H, sf.W, 12, 16)]
    ref.load_state(make_state([np.concatenate([c.numpy(), l.numpy()])], [cfg["mapping"]["localMLP_max_len"]], [0], [], [first], 0, -1))
    flags, labels, bindings, boxes, active, last_switch = [], [], [], [], [], 0
    for k in range(every, len(frames), every):
        s = ref.slam
        anchor = s.kf_c2w[s.kfSet.localMLP_first_kf[s.active_localMLP_Id[0]]]
        before = ref.dump_state()
        flag, label, _, kf = ref.process(frames[k], (anchor.inverse() @ poses[k]).numpy(), k,
                                         (k - last_switch) <= cfg["tracking"]["switch_interval"])
        if ref.overlap is not None:
            margins(cfg, before, poses[k].numpy(), frames[k], ref.overlap, int(before["scalars"][0]), ref.overlap_target)
        if flag in (1, 3):
            last_switch = k
        st = ref.dump_state()
        pad = np.zeros((sc.MAX_BOXES, 6), F32)
        pad[:len(st["boxes"])] = st["boxes"]
        flags.append(flag), labels.append(label), bindings.append(st["keyframe_submaps"][kf]), boxes.append(pad), active.append(st["scalars"][0])
    n = max(len(ref.dump_state()["boxes"]), 1)
    np.savez_compressed(os.path.join(sf.GOLDEN, f"walk_{name}.npz"), spec=json.dumps({"cfg": cfg_over, "labels": labels}),
                        e_flags=np.asarray(flags, np.int64), e_bindings=np.asarray(bindings, np.int64), e_boxes=np.stack(boxes)[:, :n],
                        e_active=np.asarray(active, np.int64), e_scalars=ref.dump_state()["scalars"])
    print(f"walk_{name}: {labels}")
    return set(labels)


def main():
    if not ref_import.available():
        sys.exit("the upstream tree is not present")
    os.makedirs(sf.GOLDEN, exist_ok=True)
    branches()
    got = record_walk("a", {"mapping": {"min_cr_localMLP_len": [2.0, 2.0, 2.0], "localMLP_max_len": [7.0, 7.0, 4.2],
                                        "localMLP_max_len_back": [7.0, 7.0, 4.2]}, "cam": {"far": 6}})
    assert {"unchanged", "new localMLP", "double binding, unchanged"} <= got, got
    # far 3.5 with max_len [7, 7, 3.6] never expands at this image size (most of the frame lies beyond far and counts against every
    # box); far 5.5, max_len [7, 7, 7] and no forced keyframes after a switch does (far 6 puts a projected point within 1e-3 px
    # of an edge bound at one switch, which the margin conditions refuse)
    got = record_walk("b", {"mapping": {"min_cr_localMLP_len": [1.0, 1.0, 1.0], "localMLP_max_len": [7.0, 7.0, 7.0],
                                        "localMLP_max_len_back": [7.0, 7.0, 7.0]}, "cam": {"far": 5.5}, "tracking": {"switch_interval": 0}})
    assert {"unchanged", "new localMLP", "expanded"} <= got, got
    for path in sf.fixtures("branch") + sf.fixtures("walk"):
        assert os.path.getsize(path) < 1000 * 1000, path


if __name__ == "__main__":
    main()
