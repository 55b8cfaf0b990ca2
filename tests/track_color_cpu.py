"""Float64 restatement of the TSDF tracker's colour registration (mipsf_track_register_color: include/mipsf_track_color.h,
csrc/track_color.hip, TSDFVolume.track(rgb=...)) in numpy, following the header's rule literally and built the way
tests/track_cpu.py builds `evaluate` and `register`: every floating-point operation below is one IEEE float64 operation.  The
device's geometric pair sets, photometric row sets, both counts and the iteration count must EQUAL what this file gives, its pose
to the rounding of the sums' order and of sin and cos.  It is a checker, not the product.  It also holds the cases the tests share,
each computed once, all on the colour fusion of box/40x56/v0.15/t4 (20 x 40 x 24 voxels).
"""
import math

import numpy as np

from . import icp_cpu
from . import raster_cpu as R
from . import track_cpu as TC
from . import tsdf_cpu as T

RESULT_DOUBLES = 22                   # MIPSF_TRACK_COLOR_RESULT_DOUBLES
WEIGHTS = (0.01, 0.1, 1.0, 10.0)      # the sweep of tests/test_track_color_cpu.py; the package's default is its best


def box_color(lo, hi, pose32, K, H, W):
    """The closed form of synth.render_box_frame's texture in float64, next to raster_cpu.box_exit_depth: the colour
    0.5 + 0.5 sin(4 x) of the point at which every pixel's ray leaves the box -> float64 [H,W,3]"""
    pose = np.asarray(pose32, np.float32).astype(np.float64)
    dw = np.stack(R.pixel_rays(pose, K, H, W), -1)
    depth = R.box_exit_depth(lo, hi, pose32, K, H, W).reshape(-1)
    hit = pose[:3, 3] + dw * depth[:, None]
    return (0.5 + 0.5 * np.sin(4.0 * hit)).reshape(H, W, 3)


def intensity(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / 3.0


# ------------------------------------------------------------------------------------------------------------ registration
def evaluate_color(Tm, model_depth, model_normals, model_color, pose_ref, live, live_color, K, depth_max, max_dist, color_weight,
                   max_color_diff):
    """one evaluation of the header's rule -> dict(partner int64 [H*W], color_row bool [H*W], n, usable, sum_d2, n_color, sum_ri2,
    A, b, ambiguous, abs_ri: |rI| of every pair with a whole patch, patch: its u, v, fu, fv, Im, Iu, Iv)"""
    fx, fy, cx, cy = R.intrinsics(K)
    H, W = live.shape
    Q = np.asarray(pose_ref, np.float32).astype(np.float64)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    row, col = row.reshape(-1), col.reshape(-1)
    MD = np.asarray(model_depth, np.float32).reshape(H, W)
    with np.errstate(all="ignore"):
        d = np.asarray(live, np.float32).astype(np.float64).reshape(-1)
        usable = (d > 0) & (d < np.inf) & (d <= depth_max)
        p = TC._apply(Tm, d * ((col - cx) / fx), -(d * ((row - cy) / fy)), -d)
        q = [p[r] - Q[r, 3] for r in range(3)]
        cam = [(Q[0, c] * q[0] + Q[1, c] * q[1]) + Q[2, c] * q[2] for c in range(3)]
        z = -cam[2]
        u, v = cx + fx * (cam[0] / z), cy - fy * (cam[1] / z)
        col2, row2 = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = usable & (z > 0) & (col2 >= 0) & (col2 < W) & (row2 >= 0) & (row2 < H)
        ci, ri = np.where(inside, col2, 0).astype(np.int64), np.where(inside, row2, 0).astype(np.int64)
        dm = MD[ri, ci].astype(np.float64)
        nrm = np.asarray(model_normals, np.float32).reshape(H, W, 3)[ri, ci].astype(np.float64)
        n2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        cand = inside & (dm > 0) & (dm < np.inf) & (n2 > 0)
        c2, r2 = ci.astype(np.float64), ri.astype(np.float64)
        vm = TC._apply(Q, dm * ((c2 - cx) / fx), -(dm * ((r2 - cy) / fy)), -dm)
        e = [p[r] - vm[r] for r in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        md2 = max_dist * max_dist
        pair = cand & (d2 <= md2)
        res = (e[0] * nrm[:, 0] + e[1] * nrm[:, 1]) + e[2] * nrm[:, 2]
        # the photometric row
        c0, r0 = np.floor(u), np.floor(v)
        patch = pair & (c0 >= 0) & (c0 + 1.0 < W) & (r0 >= 0) & (r0 + 1.0 < H)
        c0i, r0i = np.where(patch, c0, 0).astype(np.int64), np.where(patch, r0, 0).astype(np.int64)
        c1i, r1i = np.minimum(c0i + 1, W - 1), np.minimum(r0i + 1, H - 1)
        corners = [MD[a, b].astype(np.float64) for a, b in ((r0i, c0i), (r0i, c1i), (r1i, c0i), (r1i, c1i))]
        deep = patch.copy()
        for dc in corners:
            deep &= (dc > 0) & (dc < np.inf)
        IM = intensity(np.asarray(model_color, np.float32).reshape(H, W, 3))
        I00, I01, I10, I11 = IM[r0i, c0i], IM[r0i, c1i], IM[r1i, c0i], IM[r1i, c1i]
        Il = intensity(np.asarray(live_color, np.float32).reshape(H * W, 3))
        fu, fv = u - c0, v - r0
        Im = (I00 * (1.0 - fu) + I01 * fu) * (1.0 - fv) + (I10 * (1.0 - fu) + I11 * fu) * fv
        Iu = (I01 - I00) * (1.0 - fv) + (I11 - I10) * fv
        Iv = (I10 - I00) * (1.0 - fu) + (I11 - I01) * fu
        rI = Im - Il
        crow = deep & (np.abs(rI) <= max_color_diff) & (np.abs(rI) < np.inf)
        zz = z * z
        gx, gy = Iu * (fx / z), -(Iv * (fy / z))
        gz = Iu * (fx * (cam[0] / zz)) - Iv * (fy * (cam[1] / zz))
        g = [(Q[r, 0] * gx + Q[r, 1] * gy) + Q[r, 2] * gz for r in range(3)]
        # what a last-bit difference could flip
        near_int = lambda x: np.abs(x - np.round(x)) < 1e-9      # noqa: E731
        amb = usable & (np.abs(z) < 1e-12)
        amb |= usable & (z > 0) & (near_int(u + 0.5) | near_int(v + 0.5))
        amb |= inside & ((np.abs(dm) < 1e-12) & (dm != 0) | (n2 < 1e-12) & (n2 != 0))
        amb |= cand & (np.abs(d2 - md2) <= 1e-12 * md2)
        amb |= pair & (near_int(u) | near_int(v))
        for dc in corners:
            amb |= patch & (np.abs(dc) < 1e-12) & (dc != 0)
        if max_color_diff < np.inf:
            amb |= deep & (np.abs(np.abs(rI) - max_color_diff) <= 1e-12 * max(1.0, max_color_diff))
    P3 = np.stack(p, 1)
    J = np.concatenate([np.cross(P3[pair], nrm[pair]), nrm[pair]], 1)
    G3 = np.stack(g, 1)[crow]
    Jc = np.concatenate([np.cross(P3[crow], G3), G3], 1)
    return {"partner": np.where(pair, ri * W + ci, -1), "color_row": crow, "n": int(pair.sum()), "usable": int(usable.sum()),
            "sum_d2": float(d2[pair].sum()), "n_color": int(crow.sum()), "sum_ri2": float((rI[crow] * rI[crow]).sum()),
            "A": J.T @ J + color_weight * (Jc.T @ Jc), "b": J.T @ res[pair] + color_weight * (Jc.T @ rI[crow]), "ambiguous": int(amb.sum()),
            "abs_ri": np.abs(rI[deep]), "patch": {"u": u[deep], "v": v[deep], "fu": fu[deep], "fv": fv[deep], "Im": Im[deep], "Iu": Iu[deep], "Iv": Iv[deep]}}


def register_color(model_depth, model_normals, model_color, pose_ref, live, live_color, pose_init, K, depth_max=math.inf, max_dist=0.5,
                   max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, color_weight=1.0, max_color_diff=math.inf,
                   relative_color_rmse=1e-6):
    """the loop of mipsf_track_register_color -> dict(transformation, pose fp32, n, fitness, rmse, n_color, color_rmse, iterations,
    partner, color_row, pairs_per_eval, rows_per_eval, ambiguous_per_eval)"""
    Tm = np.asarray(pose_init, np.float32).astype(np.float64).copy()
    it, prev, pairs, rows, ambiguous = 0, None, [], [], []
    while True:
        ev = evaluate_color(Tm, model_depth, model_normals, model_color, pose_ref, live, live_color, K, float(depth_max), float(max_dist),
                            float(color_weight), float(max_color_diff))
        fitness = ev["n"] / ev["usable"] if ev["usable"] else 0.0
        rmse = math.sqrt(ev["sum_d2"] / ev["n"]) if ev["n"] else 0.0
        crmse = math.sqrt(ev["sum_ri2"] / ev["n_color"]) if ev["n_color"] else 0.0
        pairs.append(ev["n"]), rows.append(ev["n_color"]), ambiguous.append(ev["ambiguous"])
        stop = it >= max_iteration or (it > 0 and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse
                                       and abs(prev[2] - crmse) < relative_color_rmse)
        if stop:
            break
        x = icp_cpu.solve_psd(ev["A"], -ev["b"]) if ev["n"] else None
        if x is not None:
            U = icp_cpu.rotation_zyx(x)
            Tm[:3] = U @ Tm[:3]
            Tm[:3, 3] += x[3:]
        prev = (fitness, rmse, crmse)
        it += 1
    return {"transformation": Tm, "pose": Tm.astype(np.float32), "n": ev["n"], "fitness": fitness, "rmse": rmse, "n_color": ev["n_color"],
            "color_rmse": crmse, "iterations": it, "partner": ev["partner"], "color_row": ev["color_row"], "pairs_per_eval": pairs,
            "rows_per_eval": rows, "ambiguous_per_eval": ambiguous}


def odometry_color(depth, rgb, K, first_pose, origin, voxel, dims, trunc, color_weight=None, min_correspondences=0, **kw):
    """tsdf_odometry(rgb=..., color_weight=...) on the host -> (poses fp32 [n,4,4], records, state): the colour is always fused,
    and registered against only when color_weight is given"""
    D, C3 = np.asarray(depth, np.float32), np.asarray(rgb, np.float32)
    n, H, W = D.shape
    ticks = T.make_ticks(origin, voxel, dims)
    state = T.new_state(dims, True)
    poses = np.zeros((n, 4, 4), np.float32)
    poses[0] = np.asarray(first_pose, np.float32)
    T.integrate(state, ticks, D[:1], poses[:1], K, trunc, rgb=C3[:1])
    records = [None]
    for k in range(1, n):
        m = TC.raycast(state, origin, voxel, poses[k - 1:k], K, H, W, 0.5 * trunc, color=color_weight is not None)
        if color_weight is None:
            r = TC.register(m["depth"][0], m["normals"][0], poses[k - 1], D[k], poses[k - 1], K, max_dist=trunc, **kw)
        else:
            r = register_color(m["depth"][0], m["normals"][0], m["color"][0], poses[k - 1], D[k], C3[k], poses[k - 1], K, max_dist=trunc,
                               color_weight=color_weight, **kw)
        r["lost"] = r["n"] < min_correspondences
        poses[k] = poses[k - 1] if r["lost"] else r["pose"]
        if not r["lost"]:
            T.integrate(state, ticks, D[k:k + 1], poses[k:k + 1], K, trunc, rgb=C3[k:k + 1])
        records.append(r)
    return poses, records, state


# ------------------------------------------------------------------------------------------------------------ cases
VOLUME = TC.REG_VOLUME                # box/40x56/v0.15/t4
K_ONE_WALL, K_TWO_WALLS = (120.0, 120.0, 27.5, 19.5), (90.0, 90.0, 27.5, 19.5)
CASES = ("one_wall", "two_walls", "corner", "bad_pixels", "color_cut", "image_17x33", "image_1x1", "no_model", "weight_0")
GEOMETRIC = ("one_wall", "two_walls", "corner")
# Every registration starts a millimetre beside the pose its model was cast from: started ON it, u and v of the first evaluation
# are the live pixel's own column and row to a few ulps, and floor(u) is then a matter of the last bit.
NUDGE = (0.0011, 0.0007, 0.0005)
_memo = {}


def color_volume():
    """the CPU fusion of the volume's 20 views with rgb = the texture -> dict(state, origin, voxel, dims, trunc)"""
    if "volume" not in _memo:
        c = T.case(VOLUME)
        _, _, lo, hi = R.box_room()
        rgb = np.stack([box_color(lo, hi, p.numpy(), c["K"], c["H"], c["W"]) for p in c["poses"]]).astype(np.float32)
        state = T.new_state(c["dims"], True)
        T.integrate(state, c["ticks"], c["depth"], c["poses"], c["K"], c["trunc"], rgb=rgb)
        _memo["volume"] = {"state": state, "origin": c["origin"], "voxel": c["voxel"], "dims": c["dims"], "trunc": c["trunc"], "depth": c["depth"],
                           "rgb": rgb, "poses": c["poses"], "K": c["K"]}
    return _memo["volume"]


def model(pose_ref, K, H, W):
    """the ray cast of the colour volume with color=True -> (depth [H,W], normals [H,W,3], color [H,W,3])"""
    key = ("model", np.asarray(pose_ref, np.float32).tobytes(), tuple(K), H, W)
    if key not in _memo:
        v = color_volume()
        m = TC.raycast(v["state"], v["origin"], v["voxel"], np.asarray(pose_ref, np.float32)[None], K, H, W, 0.5 * v["trunc"], color=True)
        _memo[key] = (m["depth"][0], m["normals"][0], m["color"][0])
    return _memo[key]


def _moved(ref, t_cam=(0.0, 0.0, 0.0), t_world=(0.0, 0.0, 0.0)):
    out = np.asarray(ref, np.float64).copy()
    out[:3, 3] += out[:3, :3] @ np.asarray(t_cam, np.float64) + np.asarray(t_world, np.float64)
    return out.astype(np.float32)


def _frame(truth, K, H, W):
    _, _, lo, hi = R.box_room()
    return R.box_exit_depth(lo, hi, truth, K, H, W).astype(np.float32), box_color(lo, hi, truth, K, H, W).astype(np.float32)


def _bad(a, shift=0):
    """track_cpu's pattern over the top left quarter of an image (0 / NaN / inf / negative), moved right and down by `shift`"""
    H, W = a.shape[:2]
    q = a[shift:shift + H // 2, shift:shift + W // 2]
    q[::2, ::2] = 0.0
    q[1::2, ::2] = np.nan
    q[::2, 1::2] = np.inf
    q[1::2, 1::2] = -1.5


def case(name):
    """name -> dict(model_depth, model_normals, model_color, pose_ref, live, live_color, pose_init, truth, K, H, W, depth_max, max_dist,
    kw: color_weight is left to the caller unless the case is about it)"""
    if name in _memo:
        return _memo[name]
    v = color_volume()
    _, _, lo, hi = R.box_room()
    centre = 0.5 * (lo + hi) + np.asarray(T.BOX_OFFSETS[0])
    H, W, K = R.SIZES["40x56"]
    kw = {}
    if name in ("one_wall", "color_cut"):
        K = K_ONE_WALL
        ref = R.pose_of(tuple(centre), 0.0, 0.0).numpy()
        truth = _moved(ref, t_cam=(0.06, 0.04, 0.0))
    elif name == "two_walls":
        K = K_TWO_WALLS
        ref = R.pose_of(tuple(centre), math.pi / 4, 0.0).numpy()
        truth = _moved(ref, t_world=(0.0, 0.07, 0.0))            # the walls' common edge is the y axis
    elif name in ("corner", "bad_pixels", "no_model", "weight_0"):
        ref = v["poses"][TC.REG_VIEW].numpy()
        truth = TC.perturbed(ref, *TC.REG_OFFSETS["1.9deg_5.8cm"])
    elif name == "image_17x33":
        H, W, K = 17, 33, (25.0, 26.0, 16.3, 8.1)
        ref = v["poses"][2].numpy()                              # yaw 0, pitch 0: a wall, and at this focal length its neighbours
        truth = TC.perturbed(ref, 0.64, 2.3, 1)
    elif name == "image_1x1":
        H, W, K = 1, 1, (30.0, 30.0, 0.0, 0.0)
        ref = v["poses"][2].numpy()
        truth = _moved(ref, t_cam=(0.0, 0.0, 0.02))
    else:
        raise KeyError(name)
    md, mn, mc = model(ref, K, H, W)
    live, live_color = _frame(truth, K, H, W)
    if name == "bad_pixels":
        md, mn, mc = md.copy(), mn.copy(), mc.copy()
        _bad(live), _bad(live_color, 1), _bad(mc, 1)
    if name == "no_model":
        md, mn, mc = np.zeros_like(md), np.zeros_like(mn), np.zeros_like(mc)
    if name == "weight_0":
        kw["color_weight"] = 0.0
    out = {"model_depth": md, "model_normals": mn, "model_color": mc, "pose_ref": ref, "live": live, "live_color": live_color, "pose_init": _moved(ref, NUDGE),
           "truth": truth, "K": K, "H": H, "W": W, "depth_max": math.inf, "max_dist": v["trunc"], "kw": kw}
    if name == "color_cut":                                      # the median |rI| of the first evaluation: half the rows go
        ev = evaluate_color(out["pose_init"].astype(np.float64), md, mn, mc, ref, live, live_color, K, math.inf, v["trunc"], 1.0, math.inf)
        s = np.sort(ev["abs_ri"])
        kw["max_color_diff"] = float(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))              # between two rows, never on one
    _memo[name] = out
    return out


def want(name, **kw):
    """the restatement's answer to a case; color_weight must be among the keywords unless the case sets it"""
    c = case(name)
    kw = dict(kw, **c["kw"])
    key = (name, tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = register_color(c["model_depth"], c["model_normals"], c["model_color"], c["pose_ref"], c["live"], c["live_color"], c["pose_init"],
                                    c["K"], c["depth_max"], c["max_dist"], **kw)
    return _memo[key]


def depth_only(name, **kw):
    c = case(name)
    key = ("depth_only", name, tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = TC.register(c["model_depth"], c["model_normals"], c["pose_ref"], c["live"], c["pose_init"], c["K"], c["depth_max"], c["max_dist"], **kw)
    return _memo[key]


def reg_colors(name):
    """colour images to go with track_cpu.reg_case(name): the colour of this file's view-7 model and the texture at the case's truth"""
    c = TC.reg_case(name)
    _, _, lo, hi = R.box_room()
    v = color_volume()
    mc = model(v["poses"][TC.REG_VIEW].numpy(), c["K"], c["H"], c["W"])[2]
    return mc, box_color(lo, hi, c["truth"], c["K"], c["H"], c["W"]).astype(np.float32)


# the odometry: 8 frames at 33 x 47 facing one wall through a narrow lens, sliding 1.5 cm a frame along it; voxels of 10 cm
ODO_FRAMES, K_ODO = 8, (100.0, 100.0, 23.2, 16.4)


def odo_case():
    """-> dict(depth fp32 [8,H,W], rgb fp32 [8,H,W,3], truth fp32 [8,4,4], K, H, W, origin, voxel, dims, trunc, bounds [3,2])"""
    if "odo" not in _memo:
        H, W, _ = R.SIZES["33x47"]
        _, _, lo, hi = R.box_room()
        centre = 0.5 * (lo + hi) + np.asarray(T.BOX_OFFSETS[0])
        ref = R.pose_of(tuple(centre), 0.0, 0.0).numpy()
        truth = np.stack([_moved(ref, t_cam=(0.012 * k, 0.009 * k, 0.0)) for k in range(ODO_FRAMES)])
        frames = [_frame(p, K_ODO, H, W) for p in truth]
        voxel = 0.1
        origin, dims = T.box_grid(voxel)
        bounds = np.stack([origin, origin + voxel * (np.asarray(dims) - 1.5)], 1)
        _memo["odo"] = dict(depth=np.stack([f[0] for f in frames]), rgb=np.stack([f[1] for f in frames]), truth=truth, K=K_ODO, H=H, W=W,
                            origin=np.asarray(origin, np.float64), voxel=voxel, dims=tuple(dims), trunc=4 * voxel, bounds=bounds)
    return _memo["odo"]
