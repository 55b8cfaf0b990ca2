"""What tests/test_submap_cpu.py, tests/test_gpu_submap.py and tests/golden/make_submap_golden.py share: the small configuration,
the frames (regenerated with ``synth`` -- no image is committed), and running a SubmapManager over a recorded fixture.

A branch fixture (tests/golden/submap/branch_*.npz) is one frame plus a constructed state that sends a single
``process_keyframe`` down one branch; a walk fixture (walk_*.npz) is the reference's trace over the keyframes of the two-room
walk.  ``spec`` (JSON) holds the settings, ``s_*`` the state before, ``e_*`` what the reference's Manager did.
"""
import copy
import glob
import json
import os

import numpy as np
import torch

from mipsfusion_amd import synth
from mipsfusion_amd.submap_manager import SubmapManager, derive_schedule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "submap")
H, W = 154, 203                         # the smallest image that holds the reference's 150 x 200 lattice
INTRINSICS = (104.8, 104.8, 101.0, 76.5)
ROOM = [[-2.0, 2.0], [-1.5, 1.5], [-3.0, 3.0]]
LABELS = ("unchanged", "expanded", "new localMLP", "switch to prev", "wait loop, new localMLP", "double binding, unchanged",
          "double binding, active submap switch")

BASE_CFG = {
    "cam": {"H": H, "W": W, "fx": INTRINSICS[0], "fy": INTRINSICS[1], "cx": INTRINSICS[2], "cy": INTRINSICS[3], "crop_edge": 0,
            "near": 0, "far": 5},
    "sampling": {"kf_n_rays_h": 12, "kf_n_rays_w": 16},
    "mapping": {"min_containing_ratio": 0.75, "min_containing_ratio_mo": 0.8, "min_containing_ratio_back": 0.7,
                "min_cr_localMLP_len": [0.1, 0.1, 0.1], "localMLP_max_len": [10.0, 10.0, 10.0],
                "localMLP_max_len_back": [10.0, 10.0, 10.0], "localMLP_num": 10, "keyframe_every": 15,
                "overlapping": {"n_rays_h": 24, "n_rays_w": 32, "min_pts": 200}},
    "tracking": {"switch_interval": 30},
}


def config(overrides=None):
    cfg = copy.deepcopy(BASE_CFG)
    for section, values in (overrides or {}).items():
        for k, v in values.items():
            if isinstance(v, dict):
                cfg[section].setdefault(k, {}).update(v)
            else:
                cfg[section][k] = v
    return cfg


def rows_of(frame):
    return torch.cat([frame["direction"], frame["rgb"], frame["depth"][..., None]], -1).reshape(-1, 7).contiguous()


def box_frame(pose_world, seed, frame_id):
    return synth.render_box_frame(ROOM, torch.as_tensor(pose_world, dtype=torch.float32), H, W, *INTRINSICS, shrink=0.0, seed=seed,
                                  frame_id=frame_id)


_WALK = {}


def walk(cfg):
    """the 300-frame two-room walk at the fixtures' size -> (world poses, frames); rendered once per process"""
    if "walk" not in _WALK:
        poses, frames, _ = synth.two_room_sequence(cfg)
        _WALK["walk"] = (poses, frames)
    return _WALK["walk"]


def fixtures(kind):
    return sorted(glob.glob(os.path.join(GOLDEN, f"{kind}_*.npz")))


def load(path):
    z = np.load(path)
    d = {k: z[k] for k in z.files}
    d["spec"] = json.loads(str(d["spec"]))
    return d


class StubRectify:
    """stands where upstream calls poseCorrector.switch_pose_rectifying: accepts or rejects, hands the initial pose back"""

    def __init__(self, accept):
        self.accept, self.calls = bool(accept), []

    def __call__(self, rows, pose_ini, pose_before, sub_after, sub_before, kf_ids, masks):
        self.calls.append((np.array(pose_ini), np.array(pose_before), int(sub_after), int(sub_before), np.array(kf_ids), np.array(masks)))
        return self.accept, 1234, np.array(pose_ini)


def state_of(fx):
    return {k[2:]: fx[k] for k in fx if k.startswith("s_")}


def manager_for(fx, backend, device="cuda"):
    spec = fx["spec"]
    stub = StubRectify(spec.get("accept", True))
    m = SubmapManager(config(spec["cfg"]), H, W, INTRINSICS, device=device, rectify=stub, backend=backend, max_keyframes=32)
    return m, stub


def run_branch(fx, backend, device="cuda"):
    """-> (manager after the call, Decision, the stub)"""
    spec = fx["spec"]
    m, stub = manager_for(fx, backend, device)
    m.load_state(state_of(fx))
    rows = rows_of(box_frame(fx["pose_world"], spec["seed"], spec["frame_id"]))
    if backend == "hip":
        rows = rows.to(device)
    d = m.process_keyframe(rows, fx["pose_local"], spec["frame_id"], force=spec["force"])
    return m, d, stub


def check_branch(fx, m, d, stub):
    """the manager against what the reference's Manager did: flag, label, bindings, boxes bit for bit, counters, wait-loop state,
    the ratios it looked at and the overlap record"""
    spec = fx["spec"]
    assert (d.flag, d.label) == (spec["flag"], spec["label"])
    assert list(d.bindings) == fx["e_bindings"].tolist()
    st = m.dump_state()
    for key in ("boxes", "max_len"):
        assert np.array_equal(st[key].view(np.uint32), fx["e_" + key].view(np.uint32)), key
    assert np.array_equal(st["scalars"], fx["e_scalars"]), (st["scalars"], fx["e_scalars"])
    assert np.array_equal(st["adjacent"], fx["e_adjacent"])
    assert np.array_equal(st["first_kf"], fx["e_first_kf"])
    assert np.array_equal(st["keyframe_ref"], fx["e_keyframe_ref"])
    assert np.array_equal(st["keyframe_submaps"], fx["e_keyframe_submaps"])
    centre, length = d.stats.surface
    assert np.array_equal(np.concatenate([centre, length]).view(np.uint32), fx["e_surface"].view(np.uint32))
    for name, value in d.ratios.items():                  # float32 count / count, as upstream forms them
        assert np.array_equal(np.float32(value).view(np.uint32), fx["e_" + name].view(np.uint32)) or \
            (np.isnan(value) and np.isnan(fx["e_" + name])), name
    if "e_mask_final" in fx:                              # find_overlapping_region ran
        assert len(stub.calls) == int(fx["e_rectify_calls"])
        rec = d.overlap if d.flag == 1 else None
        if rec is not None:
            assert np.array_equal(rec["mask_final"], fx["e_mask_final"])
            assert np.array_equal(rec["top_kf_masks"], fx["e_top_kf_masks"])
            assert np.array_equal(rec["kf_ids"], fx["e_kf_ids"])
            assert np.array_equal(rec["target_d"].view(np.uint32), fx["e_target_d"].view(np.uint32))
            assert np.array_equal(rec["rays_d_cam"].view(np.uint32), fx["e_rays_d_cam"].view(np.uint32))
            assert np.allclose(d.rectified_pose, fx["e_rectified"], rtol=0, atol=1e-5)     # through a float32 inverse on either side
    else:
        assert not stub.calls


def run_walk(fx, backend, device="cuda"):
    spec = fx["spec"]
    cfg = config(spec["cfg"])
    poses, frames = walk(cfg)
    stub = StubRectify(True)
    schedule, trace, m = derive_schedule(frames, poses, cfg, INTRINSICS, device=device, rectify=stub, backend=backend,
                                         return_manager=True, max_keyframes=32)
    return schedule, trace, m


def check_walk(fx, schedule, trace, m):
    assert [d.label for d in trace] == fx["spec"]["labels"]
    assert [d.flag for d in trace] == fx["e_flags"].tolist()
    assert np.array_equal(np.asarray([d.bindings for d in trace]), fx["e_bindings"])
    for i, d in enumerate(trace):
        n = len(d.boxes)
        assert np.array_equal(d.boxes.view(np.uint32), fx["e_boxes"][i, :n].view(np.uint32)), f"keyframe {d.keyframe}"
        assert d.active == fx["e_active"][i]
    every = config(fx["spec"]["cfg"])["mapping"]["keyframe_every"]
    implied = {}
    for d, flag in zip(trace, fx["e_flags"].tolist()):
        if flag == 3:
            implied[d.keyframe * every] = ("new",)
        elif flag == 1:
            implied[d.keyframe * every] = ("back", int(fx["e_active"][d.keyframe - 1]))
    assert schedule == implied
    assert np.array_equal(m.dump_state()["scalars"], fx["e_scalars"])
