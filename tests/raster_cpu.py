"""Float64 restatement of the mesh renderer (mipsfusion_amd/mesh_render.py, csrc/raster.hip, include/mipsf_raster.h) in numpy,
following the header's rules literally: every floating-point operation below is one IEEE float64 operation (numpy contracts
nothing), EVERY pixel is tested against EVERY face (no screen box, no tiles), and the winner of a pixel is the integer minimum of
(depth bits, face index).  The device's depth words, face indices and `seen` flags must EQUAL what this file gives.  It is a
checker, not the product.
"""
import math

import numpy as np

KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
TINY = np.float32(2.0 ** -126)


def intrinsics(K):
    K = np.asarray(K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.ndim == 2 else tuple(float(x) for x in K)


def _poses(poses):
    p = np.asarray([np.asarray(q, np.float32) for q in poses] if isinstance(poses, (list, tuple)) else poses, np.float32)
    return (p[None] if p.ndim == 2 else p).astype(np.float64)


def _dot(d, n):
    return (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]


def _cross(P, Q):
    return (P[1] * Q[2] - P[2] * Q[1], P[2] * Q[0] - P[0] * Q[2], P[0] * Q[1] - P[1] * Q[0])


def pixel_rays(pose, K, H, W):
    """dw [3] of arrays [H*W]: the header's world-frame direction of every pixel, row-major"""
    fx, fy, cx, cy = intrinsics(K)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx = ((i - cx) / fx).reshape(-1)
    dy = (-((j - cy) / fy)).reshape(-1)
    R = pose[:3, :3]
    return [(R[k, 0] * dx + R[k, 1] * dy) + R[k, 2] * (-1.0) for k in range(3)]


def render_depth(vertices32, faces, poses, K, H, W, near=0.0, far=math.inf, chunk=256, return_tt=False):
    """-> (depth fp32 [n,H,W], face int32 [n,H,W]) (, tt float64 [n,H,W]: the winner's unrounded depth, nan for a miss)"""
    v = np.asarray(vertices32, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = _poses(poses)
    ok = np.all((f >= 0) & (f < len(v)), axis=1)
    index = np.nonzero(ok)[0]
    depth = np.zeros((len(P), H, W), np.float32)
    face = np.full((len(P), H, W), -1, np.int32)
    tts = np.full((len(P), H, W), np.nan)
    with np.errstate(all="ignore"):
        for n, pose in enumerate(P):
            t = pose[:3, 3]
            dw = [d[None, :] for d in pixel_rays(pose, K, H, W)]
            best = np.full(H * W, KEY_EMPTY, np.uint64)
            best_tt = np.full(H * W, np.nan)
            for s in range(0, len(index), chunk):
                ids = index[s:s + chunk]
                A, B, C = (v[f[ids, k]] - t for k in range(3))
                A, B, C = ([X[:, d, None] for d in range(3)] for X in (A, B, C))
                nAB, nBC, nCA = _cross(A, B), _cross(B, C), _cross(C, A)
                e0, e1, e2 = _dot(dw, nAB), _dot(dw, nBC), _dot(dw, nCA)
                inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                den = (e0 + e1) + e2
                num = _dot(A, nBC)
                tt = num / den
                d32 = tt.astype(np.float32)
                hit = inside & (den != 0) & (tt > near) & (tt < far) & (d32 >= TINY) & (d32 < np.float32(np.inf))
                key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[:, None].astype(np.uint64)
                key = np.where(hit, key, KEY_EMPTY)
                row = np.argmin(key, axis=0)
                k = key[row, np.arange(H * W)]
                better = k < best
                best = np.where(better, k, best)
                best_tt = np.where(better, tt[row, np.arange(H * W)], best_tt)
            got = best != KEY_EMPTY
            depth[n] = np.where(got, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).reshape(H, W)
            face[n] = np.where(got, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(H, W)
            tts[n] = np.where(got, best_tt, np.nan).reshape(H, W)
    return (depth, face, tts) if return_tt else (depth, face)


# ------------------------------------------------------------------------------------------------------------ depth L1
def l1_records(a, b):
    """two depth stacks fp32 [n,H,W] -> per view dict(sum_all, sum_both, both, rec_only, gt_only, neither); the sums by math.fsum"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = []
    for x, y in zip(a, b):
        d = np.abs(x.astype(np.float64) - y.astype(np.float64)).reshape(-1)
        hx, hy = (x != 0).reshape(-1), (y != 0).reshape(-1)
        out.append({"sum_all": math.fsum(d), "sum_both": math.fsum(d[hx & hy]), "both": int((hx & hy).sum()),
                    "rec_only": int((hx & ~hy).sum()), "gt_only": int((~hx & hy).sum()), "neither": int((~hx & ~hy).sum())})
    return out


def depth_metrics(recs, H, W):
    """the fields of mipsfusion_amd.mesh_render.DepthMetrics as a dict"""
    n, hw = len(recs), H * W
    both = sum(r["both"] for r in recs)
    per_view = tuple(r["sum_all"] / hw for r in recs)
    return {"l1": math.fsum(per_view) / n, "l1_both": math.fsum(r["sum_both"] for r in recs) / both if both else math.nan,
            "both": both / (n * hw), "rec_only": sum(r["rec_only"] for r in recs) / (n * hw),
            "gt_only": sum(r["gt_only"] for r in recs) / (n * hw), "neither": sum(r["neither"] for r in recs) / (n * hw),
            "l1_per_view": per_view, "l1_both_per_view": tuple(r["sum_both"] / r["both"] if r["both"] else math.nan for r in recs),
            "n_views": n, "pixels": hw}


def depth_l1(mesh_rec, mesh_gt, poses, K, H, W, near=0.0, far=math.inf):
    d_rec = render_depth(np.asarray(mesh_rec[0], np.float32), mesh_rec[1], poses, K, H, W, near, far)[0]
    d_gt = render_depth(np.asarray(mesh_gt[0], np.float32), mesh_gt[1], poses, K, H, W, near, far)[0]
    return depth_metrics(l1_records(d_rec, d_gt), H, W)


# ------------------------------------------------------------------------------------------------------------ visibility
def visible(points32, depth, poses, max_depth, K, edge, eps):
    """-> bool [m]: the header's rule of mipsf_raster_visible, the OR over the views"""
    p = np.asarray(points32, np.float32).astype(np.float64).reshape(-1, 3)
    D = np.asarray(depth, np.float32)
    P = _poses(poses)
    md = np.asarray(max_depth, np.float32).astype(np.float64).reshape(-1)
    fx, fy, cx, cy = intrinsics(K)
    _, H, W = D.shape
    seen = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            R, t = pose[:3, :3], pose[:3, 3]
            q = [p[:, d] - t[d] for d in range(3)]
            cam = [(R[0, c] * q[0] + R[1, c] * q[1]) + R[2, c] * q[2] for c in range(3)]
            z = -cam[2]
            u = cx + fx * (cam[0] / z)
            v = cy - fy * (cam[1] / z)
            ok = (z > 0) & (z < md[k]) & (edge < u) & (u < float(W) - edge) & (edge < v) & (v < float(H) - edge)
            col, row = np.floor(u + 0.5), np.floor(v + 0.5)
            ok &= (col >= 0) & (col < W) & (row >= 0) & (row < H)
            ci, ri = np.where(ok, col, 0).astype(np.int64), np.where(ok, row, 0).astype(np.int64)
            d = D[k, ri, ci]
            seen |= ok & ((d == 0) | (z <= d.astype(np.float64) + eps))
    return seen


def cull_faces(mesh, occluder, poses, max_depth, K, W, H, edge, eps):
    """the face list evaluate.cull_to_views(occlusion=True) keeps: all three vertices seen in front of the occluder's depth"""
    v32, f = np.asarray(mesh[0], np.float32), np.asarray(mesh[1], np.int64)
    occ = mesh if occluder is None else occluder
    depth = render_depth(np.asarray(occ[0], np.float32), occ[1], poses, K, H, W)[0]
    seen = visible(v32, depth, poses, max_depth, K, edge, eps)
    ok = np.all((f >= 0) & (f < len(v32)), axis=1)
    keep = np.zeros(len(f), bool)
    keep[ok] = seen[f[ok]].all(1)
    return f[keep]


# ------------------------------------------------------------------------------------------------------------ known answers
def box_exit_depth(lo, hi, pose32, K, H, W):
    """The closed form of synth.render_box_frame in float64: the z-depth at which every pixel's ray leaves the box lo..hi from a
    camera inside it -> float64 [H,W].  The ray is the header's R d of the fp32 pose, widened."""
    pose = np.asarray(pose32, np.float32).astype(np.float64)
    dw = np.stack(pixel_rays(pose, K, H, W), -1)
    t = pose[:3, 3]
    with np.errstate(all="ignore"):
        tt = np.where(dw > 0, (np.asarray(hi) - t) / dw, np.where(dw < 0, (np.asarray(lo) - t) / dw, np.inf))
    return tt.min(-1).reshape(H, W)


# ------------------------------------------------------------------------------------------------------------ cases
SIZES = {"40x56": (40, 56, (40.0, 40.0, 27.5, 19.5)), "33x47": (33, 47, (35.0, 37.0, 23.2, 16.4))}      # name -> H, W, (fx, fy, cx, cy)

# (yaw, pitch) of the ten box-room views: the four walls, floor and ceiling, corners, and two oblique ones
BOX_VIEWS = ((0.3, -0.1), (2.1, 0.25), (0.0, 0.0), (math.pi / 2, 0.0), (math.pi, 0.1), (-math.pi / 2, -0.2), (0.7, 1.3), (-2.5, -1.4),
             (math.pi / 4, 0.6), (3.9, -0.7))

# (position, yaw, pitch) in the two rooms of synth.TWO_ROOMS; yaw pi looks along +z, room A is z < 2.75
ROOMS_VIEWS = (((1.2, 3.8, 0.9), math.pi, -0.08),             # room A, through the door into room B
               ((1.2, 3.8, 4.4), 0.0, 0.05),                  # room B, through the door into room A
               ((0.2, 3.0, 1.5), math.pi + 0.5, 0.1),         # room A, onto its copy of the shared wall at an angle
               ((2.0, 4.5, 5.5), 0.4, 0.1),                   # room B, onto its copy of the shared wall and part of the door
               ((1.0, 2.0, 1.0), 0.3, -0.2),                  # room A, away from the door
               ((1.2, 3.8, 2.5), math.pi - 0.8, 0.2))         # room A, 25 cm from the shared wall


def pose_of(position, yaw, pitch):
    import torch
    from mipsfusion_amd import synth
    c2w = torch.eye(4)
    c2w[:3, :3] = synth.look_rotation(yaw, pitch)
    c2w[:3, 3] = torch.tensor(position, dtype=torch.float32)
    return c2w


def box_room():
    """-> (vertices float64, faces int64, lo, hi): the 12 triangles of the reference configuration's room"""
    from mipsfusion_amd import synth
    v, f = synth.box_room_mesh(synth.config_reference_defaults()["mapping"]["bound"])
    return v, f, v.min(0), v.max(0)


def box_poses(views=BOX_VIEWS, offset=(0.21, -0.4, 0.33)):
    import torch
    _, _, lo, hi = box_room()
    centre = 0.5 * (lo + hi) + np.asarray(offset)
    return torch.stack([pose_of(centre, yaw, pitch) for yaw, pitch in views])


def rooms_poses():
    import torch
    return torch.stack([pose_of(*view) for view in ROOMS_VIEWS])


_marched = {}


def marched_room(res=24, pad=0.25):
    """tests/mcubes_cpu.marching_cubes of the box room's SDF on res^3 voxels, in world coordinates -> (vertices float64, faces int64)"""
    if res not in _marched:
        from . import mcubes_cpu
        _, _, lo, hi = box_room()
        ticks = [np.linspace(lo[d] - pad, hi[d] + pad, res) for d in range(3)]
        p = np.stack(np.meshgrid(*ticks, indexing="ij"), -1)
        sdf = np.minimum(p - lo, hi - p).min(-1).astype(np.float32)                  # positive inside the room
        mv, mf = mcubes_cpu.marching_cubes(sdf, 0.0, 3.0)
        step = np.array([(t[-1] - t[0]) / (res - 1) for t in ticks])
        _marched[res] = (np.array([t[0] for t in ticks]) + mv * step, mf)
    return _marched[res]


def split_square():
    """E.mesh_square(0.25), its camera and intrinsics: 17 x 17 pixels whose rays meet the unit square on a lattice of pitch 1/16,
    the border pixels on its border, the 17 diagonal pixels on the edge the two faces share"""
    import torch
    from . import eval_cpu as E
    v, f = E.mesh_square(0.25)
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.5, 0.5, 1.25])
    return v, f, pose[None], (16.0, 16.0, 8.0, 8.0), 17, 17


def random_view():
    """the camera the issue's numbers for E.mesh_random() belong to -> (poses, K, H, W)"""
    import torch
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, 0.0, 4.0])
    return pose[None], (40.0, 40.0, 31.5, 23.5), 48, 64


ONE_FACE = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.7], [0.4, 1.5, -0.2]]), np.array([[0, 1, 2]]))
DEPTH_CASES = ("box_room/40x56", "box_room/33x47", "two_rooms/40x56", "two_rooms/33x47", "marched_24/33x47", "marched_24/40x56",
               "random_5000/48x64", "random_5000/33x47", "one_face/40x56", "one_face/33x47", "square/17x17", "square/33x47",
               "outside_looking_away/40x56", "near_far_cut/33x47", "camera_in_a_wall/40x56", "camera_in_a_wall/33x47")
_depth_cases = {}


def depth_case(name):
    """name -> dict(vertices fp32, faces int64, poses fp32 tensor [n,4,4], K, H, W, near, far, depth, face): the inputs of one
    render call and the restatement's answer, computed once.  Every case but the 17 x 17 square has 3 views or more in one call."""
    if name in _depth_cases:
        return _depth_cases[name]
    import torch
    from mipsfusion_amd import synth
    from . import eval_cpu as E
    mesh, size = name.split("/")
    near, far = 0.0, math.inf
    if size in SIZES:
        H, W, K = SIZES[size]
    v, f, lo, hi = box_room()
    centre = 0.5 * (lo + hi)
    if mesh == "box_room":
        poses = box_poses()
    elif mesh == "two_rooms":
        v, f = synth.two_rooms_mesh()
        poses = rooms_poses()
    elif mesh == "marched_24":
        v, f = marched_room()
        poses = box_poses(BOX_VIEWS[:3] if size == "33x47" else BOX_VIEWS[5:6])
    elif mesh == "random_5000":
        v, f = E.mesh_random()
        if size == "48x64":
            poses, K, H, W = random_view()
        else:                                                   # from 4 m away, from inside the cloud, and from inside looking up
            poses = torch.stack([pose_of((0.0, 0.0, 4.0), 0.0, 0.0), pose_of((0.1, -0.2, 0.3), 0.5, 0.2), pose_of((0.0, 0.0, 0.0), 2.0, 1.2)])
    elif mesh == "one_face":                                    # seen whole, cut by the camera plane, and from behind
        v, f = ONE_FACE
        poses = torch.stack([pose_of((0.6, 0.6, 2.0), 0.0, 0.0), pose_of((0.5, 0.5, 0.3), 1.2, 0.1), pose_of((0.6, 0.6, -2.0), math.pi, 0.0)])
    elif mesh == "square":
        v, f, poses, K17, H17, W17 = split_square()
        if size == "17x17":
            K, H, W = K17, H17, W17
        else:                                                   # the lattice view, an oblique one, and one from below the square
            poses = torch.stack([poses[0], pose_of((0.2, 0.1, 0.9), 0.4, -0.3), pose_of((0.5, 0.5, -0.5), math.pi, 0.0)])
    elif mesh == "outside_looking_away":                        # 1 m beyond the wall z = hi[2], looking along +z: everything is behind
        poses = torch.stack([pose_of((centre[0], centre[1], hi[2] + 1.0), math.pi, p) for p in (0.0, 0.3, -0.3)])
    elif mesh == "near_far_cut":                                # both lie inside the depth range of the first two views
        poses = box_poses(BOX_VIEWS[:3])
        near, far = 1.68, 2.35
    elif mesh == "camera_in_a_wall":                            # z = lo[2] exactly: looking along the wall, into the room, out of it
        poses = torch.stack([pose_of((centre[0], centre[1] + 0.3, lo[2]), yaw, pitch) for yaw, pitch in ((math.pi / 2, 0.0), (math.pi, 0.2), (0.0, 0.1), (0.7, -0.4))])
    else:
        raise KeyError(name)
    v32 = np.asarray(v, np.float32)
    depth, face = render_depth(v32, f, poses, K, H, W, near, far)
    _depth_cases[name] = {"vertices": v32, "faces": np.asarray(f, np.int64), "poses": poses, "K": K, "H": H, "W": W, "near": near, "far": far,
                          "depth": depth, "face": face}
    return _depth_cases[name]
