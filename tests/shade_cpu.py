"""Float64 restatement of the mesh shader (mipsfusion_amd/mesh_render.py, csrc/shade.hip, include/mipsf_shade.h) in numpy,
following the header's rules literally: every floating-point operation below is one IEEE float64 operation (numpy contracts
nothing), the vertex normals add their faces one by one in ascending face index, and the attribute pass recomputes the rasteriser's
edge values from the face image.  The device's colour, normal and shaded words, its vertex-normal words and its record must EQUAL
what this file gives.  It is a checker, not the product.  The cases, poses and depth renderer are tests/raster_cpu.py's, unchanged.
"""
import numpy as np

from . import raster_cpu as R

FLAT, SMOOTH = 1, 2                           # MIPSF_SHADE_FLAT, MIPSF_SHADE_SMOOTH
SHADE_CASES = ("box_room/33x47", "marched_24/33x47", "one_face/40x56", "square/17x17", "camera_in_a_wall/40x56", "random_5000/33x47")
BACKGROUND = (0.25, 0.5, 0.75)


def _unit(P):
    """the header's unit(P) on three arrays -> (three arrays, ok)"""
    L = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
    ok = (L > 0) & (L < np.inf)
    return [P[k] / L for k in range(3)], ok


def valid_faces(vertices32, faces):
    """-> bool [F]: three indices in [0, V) and nine finite coordinates"""
    v = np.asarray(vertices32, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = np.all((f >= 0) & (f < len(v)), axis=1)
    if len(v):
        ok &= np.isfinite(v[np.where(ok[:, None], f, 0)]).all((1, 2))
    return ok


def face_normals(vertices32, faces, ids):
    """N_f = cross(v[b] - v[a], v[c] - v[a]) of the faces `ids` (valid ones) -> float64 [len(ids),3]"""
    v = np.asarray(vertices32, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[ids]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    E1, E2 = b - a, c - a
    with np.errstate(all="ignore"):
        return np.stack(R._cross([E1[:, d] for d in range(3)], [E2[:, d] for d in range(3)]), -1)


def vertex_sums(vertices32, faces):
    """S of every vertex, float64 [V,3]: from +0.0, N_f added face by face in ascending index, once per corner"""
    v = np.asarray(vertices32, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.nonzero(valid_faces(v, f))[0]
    N = face_normals(v, f, ids)
    S = np.zeros((len(v), 3))
    with np.errstate(all="ignore"):
        for k, face in enumerate(ids):
            for corner in f[face]:
                S[corner] = S[corner] + N[k]
    return S


def vertex_normals(vertices32, faces):
    """the header's rule of mipsf_shade_vertex_normals -> fp32 [V,3]"""
    S = vertex_sums(vertices32, faces)
    with np.errstate(all="ignore"):
        u, ok = _unit([S[:, 0], S[:, 1], S[:, 2]])
        return np.stack([np.where(ok, u[k], 0.0) for k in range(3)], -1).astype(np.float32)


def shade(vertices32, faces, poses, K, face_image, colors=None, normals32=None, mode=FLAT, background=(0.0, 0.0, 0.0), want_normals=True):
    """the header's rule of mipsf_shade_pixels -> dict(color fp32 [n,H,W,3] or None, normals fp32 [n,H,W,3], shaded fp32 [n,H,W],
    record (hits, shaded), and in float64 for the CPU tests: hit bool [n,H,W], weights [n,H,W,3] (wA, wB, wC), s [n,H,W] (nan where
    there is no n), color64 [n,H,W,3] before its rounding).  colors may be float64 (widening is then the identity)."""
    v32 = np.asarray(vertices32, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = R._poses(poses)
    img = np.asarray(face_image, np.int64)
    n, H, W = img.shape
    valid = valid_faces(v32, f)
    col = None if colors is None else np.asarray(colors).astype(np.float64).reshape(-1, 3)
    vn = None if normals32 is None else np.asarray(normals32, np.float32).astype(np.float64).reshape(-1, 3)
    bg = np.asarray(background, np.float32)
    out = {"color": None if col is None else np.empty((n, H, W, 3), np.float32), "normals": np.zeros((n, H, W, 3), np.float32),
           "shaded": np.zeros((n, H, W), np.float32), "hit": np.zeros((n, H, W), bool), "weights": np.full((n, H, W, 3), np.nan),
           "s": np.full((n, H, W), np.nan), "color64": None if col is None else np.full((n, H, W, 3), np.nan)}
    hits = with_n = 0
    with np.errstate(all="ignore"):
        for k, pose in enumerate(P):
            fi = img[k].reshape(-1)
            ok = (fi >= 0) & (fi < len(f))
            ok &= valid[np.where(ok, fi, 0)] if len(f) else False
            idx = f[np.where(ok, fi, 0)] if len(f) else np.zeros((H * W, 3), np.int64)
            idx = np.where(ok[:, None], idx, 0)
            t = pose[:3, 3]
            dw = R.pixel_rays(pose, K, H, W)
            pts = v[idx] if len(v) else np.zeros((H * W, 3, 3))
            A, B, C = ([pts[:, c, d] - t[d] for d in range(3)] for c in range(3))
            nAB, nBC, nCA = R._cross(A, B), R._cross(B, C), R._cross(C, A)
            e0, e1, e2 = R._dot(dw, nAB), R._dot(dw, nBC), R._dot(dw, nCA)
            den = (e0 + e1) + e2
            hit = ok & (den != 0) & np.isfinite(den)
            w = [e1 / den, e2 / den, e0 / den]
            out["hit"][k] = hit.reshape(H, W)
            out["weights"][k] = np.where(hit[:, None], np.stack(w, -1), np.nan).reshape(H, W, 3)
            hits += int(hit.sum())
            if col is not None:
                c64 = np.stack([(w[0] * col[idx[:, 0], ch] + w[1] * col[idx[:, 1], ch]) + w[2] * col[idx[:, 2], ch] for ch in range(3)], -1)
                out["color64"][k] = np.where(hit[:, None], c64, np.nan).reshape(H, W, 3)
                out["color"][k] = np.where(hit[:, None], c64.astype(np.float32), bg).reshape(H, W, 3)
            if not want_normals:
                continue
            if mode == SMOOTH:
                m = [(w[0] * vn[idx[:, 0], d] + w[1] * vn[idx[:, 1], d]) + w[2] * vn[idx[:, 2], d] for d in range(3)]
            else:
                E1 = [pts[:, 1, d] - pts[:, 0, d] for d in range(3)]
                E2 = [pts[:, 2, d] - pts[:, 0, d] for d in range(3)]
                m = list(R._cross(E1, E2))
            u, has = _unit(m)
            has &= hit
            s = R._dot(u, dw)
            u = [np.where(s > 0, -u[d], u[d]) for d in range(3)]
            lambert = np.abs(s) / np.sqrt(R._dot(dw, dw))
            out["normals"][k] = np.where(has[:, None], np.stack(u, -1).astype(np.float32), np.float32(0)).reshape(H, W, 3)
            out["shaded"][k] = np.where(has, lambert.astype(np.float32), np.float32(0)).reshape(H, W)
            out["s"][k] = np.where(has, s, np.nan).reshape(H, W)
            with_n += int(has.sum())
    out["record"] = (hits, with_n)
    return out


# ------------------------------------------------------------------------------------------------------------ colours
def uniform_colors(V, seed=22):
    """a uniform fp32 draw per vertex and channel"""
    return np.random.default_rng(seed).random((V, 3), dtype=np.float32)


LINEAR_A = np.array([[0.11, -0.07, 0.05], [0.02, 0.09, -0.04], [-0.06, 0.03, 0.08]])      # c(x) = x . a + b, per channel a column
LINEAR_B = np.array([0.4, 0.5, 0.45])


def linear_field(x):
    """the linear colour field at points float64 [...,3] -> float64 [...,3], each channel (x.x*a0 + x.y*a1) + x.z*a2 + b"""
    x = np.asarray(x, np.float64)
    return np.stack([((x[..., 0] * LINEAR_A[0, ch] + x[..., 1] * LINEAR_A[1, ch]) + x[..., 2] * LINEAR_A[2, ch]) + LINEAR_B[ch] for ch in range(3)], -1)


# ------------------------------------------------------------------------------------------------------------ cases
def sphere(res=16, r=0.6):
    """tests/mcubes_cpu.marching_cubes of |x| - r on res^3 voxels over -1 .. 1 -> (vertices float64 about the origin, faces int64)"""
    from . import mcubes_cpu
    ticks = np.linspace(-1.0, 1.0, res)
    p = np.stack(np.meshgrid(ticks, ticks, ticks, indexing="ij"), -1)
    sdf = (np.sqrt((p * p).sum(-1)) - r).astype(np.float32)
    mv, mf = mcubes_cpu.marching_cubes(sdf, 0.0, 3.0)
    return -1.0 + mv * (2.0 / (res - 1)), mf


def fan(k=2000):
    """k faces round vertex 0, which every face names: the rim is a closed, wavy ring below it -> (vertices fp32, faces int64)"""
    a = 2.0 * np.pi * np.arange(k) / k
    rim = np.stack([np.cos(a) * (1.0 + 0.2 * np.sin(7 * a)), np.sin(a) * (1.0 + 0.2 * np.sin(7 * a)), -0.5 + 0.1 * np.cos(5 * a)], -1)
    v = np.concatenate([[[0.05, -0.03, 0.4]], rim]).astype(np.float32)
    f = np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], -1)
    return v, f


_cases = {}


def case(name):
    """name (one of raster_cpu's depth cases) -> dict(depth case's fields, colors fp32 [V,3], vertex_normals fp32 [V,3]), once"""
    if name not in _cases:
        c = dict(R.depth_case(name))
        c["colors"] = uniform_colors(len(c["vertices"]))
        c["vertex_normals"] = vertex_normals(c["vertices"], c["faces"])
        _cases[name] = c
    return _cases[name]


_wants = {}


def want(name, mode, colored=True, background=(0.0, 0.0, 0.0)):
    """the restatement's answer for a case, computed once per (name, mode, colored, background)"""
    key = (name, mode, colored, tuple(background))
    if key not in _wants:
        c = case(name)
        _wants[key] = shade(c["vertices"], c["faces"], c["poses"], c["K"], c["face"], c["colors"] if colored else None, c["vertex_normals"], mode,
                            background)
    return _wants[key]


# ------------------------------------------------------------------------------------------------------------ the chain
_chain = None


def chain_case():
    """Colour frames of the box room (tests/tsdf_cpu.case("colour"): analytic wall colours, ten views at 33 x 47) fused, marched
    and coloured by the restatements -> dict(vertices fp32, faces, colors fp32, poses, K, H, W, rgb [n,H,W,3], depth [n,H,W])"""
    global _chain
    if _chain is None:
        from . import tsdf_cpu as T
        c = T.case("colour")
        v, f, v_index = T.extract_mesh(c["state"], c["origin"], c["voxel"])
        colors = T.sample_color(v_index, c["state"]["weight"], c["state"]["color"])
        _chain = {"vertices": v.astype(np.float32), "faces": f, "colors": colors, "poses": c["poses"], "K": c["K"], "H": c["H"], "W": c["W"],
                  "rgb": c["rgb"], "depth": c["depth"]}
    return _chain
