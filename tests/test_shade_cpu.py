"""CPU: the float64 restatement of the mesh shader (tests/shade_cpu.py) held to what is known without a GPU -- barycentric weights
that lie in the face and add up to one, a linear colour field reproduced at the hit point, the axis normals of the box room, the
radial normals of a marched sphere, the vertices that must have no normal -- and the C ABI of the new entry points.
tests/test_gpu_shade.py holds the device to the restatement for equality of words.  Every gate below is twice what this file
measured, with the measurement next to it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from mipsfusion_amd import _lib

from . import raster_cpu as R
from . import shade_cpu as S
from .conftest import ROOT


# ------------------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("name", S.SHADE_CASES)
def test_the_weights_lie_in_the_face_and_add_up_to_one(name):
    """Measured over the six cases: no weight outside [0, 1] (the smallest is -0.0, on the square's border), the largest
    |wA + wB + wC - 1| is 4.4e-16 (box room; 2.2e-16 elsewhere, 0 on the square); the gate is twice that.  No hit pixel has s == 0
    and the smallest |s| is 0.045 (one_face, the view along the face), 12 orders above rounding: the cases hold no ambiguous
    facing decision, so equality of the normals' signs on the device is not luck.  Every hit pixel has a normal."""
    c = S.case(name)
    for mode in (S.FLAT, S.SMOOTH):
        w = S.want(name, mode)
        hit = w["hit"]
        assert np.array_equal(hit, c["face"] >= 0) and hit.any()                          # what the rasteriser hits has a usable den
        W3, s = w["weights"][hit], w["s"][hit]
        print(f"{name} mode {mode}: {hit.sum()} hits, weights {W3.min():.3e} .. {W3.max():.6f}, max |sum - 1| {np.abs(W3.sum(-1) - 1).max():.3e}, "
              f"min |s| {np.abs(s).min():.4f}")
        assert np.all((W3 >= 0) & (W3 <= 1))
        assert np.abs((W3[:, 0] + W3[:, 1]) + W3[:, 2] - 1).max() <= 2 * 4.4e-16
        assert not np.isnan(s).any() and not (s == 0).any() and np.abs(s).min() >= 0.5 * 0.0447
        assert w["record"] == (int(hit.sum()), int(hit.sum()))
        assert np.all(w["shaded"][hit] > 0) and np.all(w["shaded"] <= 1) and not w["shaded"][~hit].any() and not w["normals"][~hit].any()
        length = np.linalg.norm(w["normals"][hit].astype(np.float64), axis=1)
        assert np.abs(length - 1).max() < 2e-7                                             # three fp32 roundings of a unit vector
        if not hit.all():
            assert np.all(w["color"][~hit] == 0)


def test_a_linear_colour_field_is_reproduced():
    """c(x) = x.a + b at the vertices, in float64: the interpolated colour equals c at the hit point t + tt*dw, with tt the float64
    depth of the rasteriser's restatement.  Measured: 4.4e-16 on the box room (values of about 0.5: two ulps) and 6.2e-15 on the
    marched room, whose faces are 20 cm wide and 3 m away: cross(A,B) of two nearly equal vectors loses a digit and a half, and the
    weights and tt inherit that.  The gate is twice the larger.  Against the fp32 depth the difference is 1.8e-7, the depth's own
    rounding."""
    worst = 0.0
    for name in ("box_room/33x47", "marched_24/33x47"):
        c = S.case(name)
        _, face, tt = R.render_depth(c["vertices"], c["faces"], c["poses"], c["K"], c["H"], c["W"], return_tt=True)
        assert np.array_equal(face, c["face"])
        colors = S.linear_field(c["vertices"].astype(np.float64))
        w = S.shade(c["vertices"], c["faces"], c["poses"], c["K"], face, colors, want_normals=False)
        for k, pose in enumerate(R._poses(c["poses"])):
            dw = np.stack(R.pixel_rays(pose, c["K"], c["H"], c["W"]), -1).reshape(c["H"], c["W"], 3)
            x = pose[:3, 3] + tt[k][..., None] * dw
            err = np.abs(w["color64"][k] - S.linear_field(x))[face[k] >= 0]
            worst = max(worst, float(err.max()))
        print(f"{name}: largest |interpolated - c(hit point)| so far {worst:.3e}")
    assert worst <= 2 * 6.2e-15


# ------------------------------------------------------------------------------------------------------------ flat normals
def test_the_box_rooms_flat_normals_are_the_walls_axis_normals():
    """the exact words 0 and +-1, pointing into the room: at the hit point on a wall, away from that wall's plane"""
    c = S.case("box_room/33x47")
    w = S.want("box_room/33x47", S.FLAT)
    _, _, lo, hi = R.box_room()
    n = w["normals"]
    assert np.all(np.isin(n, (-1.0, 0.0, 1.0))) and np.all(np.abs(n).sum(-1) == 1)
    _, _, tt = R.render_depth(c["vertices"], c["faces"], c["poses"], c["K"], c["H"], c["W"], return_tt=True)
    for k, pose in enumerate(R._poses(c["poses"])):
        dw = np.stack(R.pixel_rays(pose, c["K"], c["H"], c["W"]), -1).reshape(c["H"], c["W"], 3)
        x = pose[:3, 3] + tt[k][..., None] * dw
        axis = np.abs(n[k]).argmax(-1)
        sign = np.take_along_axis(n[k], axis[..., None], -1)[..., 0]
        wall = np.where(sign > 0, lo[axis], hi[axis])                                      # +1 on the low wall, -1 on the high wall
        assert np.abs(np.take_along_axis(x, axis[..., None], -1)[..., 0] - wall).max() < 1e-6
    # head-on, the shading of a wall is the cosine between the ray and the axis
    view = 2                                                                               # yaw 0, pitch 0: looks along -z
    dw = np.stack(R.pixel_rays(R._poses(c["poses"])[view], c["K"], c["H"], c["W"]), -1).reshape(c["H"], c["W"], 3)
    on_z = np.abs(n[view][..., 2]) == 1
    assert on_z.any() and np.abs(w["shaded"][view][on_z] - (np.abs(dw[..., 2]) / np.linalg.norm(dw, axis=-1))[on_z]).max() < 1e-7


def test_one_face_from_behind_has_the_negated_normal():
    w = S.want("one_face/40x56", S.FLAT)
    front, behind = w["normals"][0][w["hit"][0]], w["normals"][2][w["hit"][2]]
    assert len(front) and len(behind) and len(np.unique(front, axis=0)) == 1 and len(np.unique(behind, axis=0)) == 1
    assert np.array_equal(behind[0], -front[0]) and front[0].any()


# ------------------------------------------------------------------------------------------------------------ vertex normals
def test_a_marched_spheres_vertex_normals_are_radial():
    """366 vertices, 728 faces on 16^3 voxels.  Measured: every normal points outwards, the largest angle to the radial direction
    is 9.08 degrees (the facets are a seventh of the radius wide); the gate is twice that."""
    v, f = S.sphere()
    n = S.vertex_normals(v.astype(np.float32), f).astype(np.float64)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    cos = (n * radial).sum(1)
    angle = np.degrees(np.arccos(np.clip(cos, -1, 1)))
    print(f"sphere: {len(v)} vertices, {len(f)} faces, angle to the radial direction max {angle.max():.3f} deg, mean {angle.mean():.3f} deg")
    assert len(f) > 500 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 2e-7
    assert angle.max() <= 2 * 9.08


def test_vertices_that_have_no_normal_and_faces_that_add_nothing():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [np.nan, 0, 0]], np.float32)
    tri = np.array([[0, 1, 2]])
    base = S.vertex_normals(v, tri)
    assert np.array_equal(base[:3], np.array([[0, 0, 1]] * 3, np.float32)) and not base[3:].any()      # 3, 4, 5 are isolated
    cancelling = S.vertex_normals(v, np.array([[0, 1, 2], [0, 2, 1]]))
    assert not cancelling.any() and not np.signbit(cancelling).any()
    for odd in ([0, 1, 6], [0, -1, 2], [0, 1, 5], [0, 1, 1], [0, 0, 0]):                   # out of range, NaN vertex, repeated vertices
        got = S.vertex_normals(v, np.array([[0, 1, 2], odd]))
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), odd
        assert not S.vertex_normals(v, np.array([odd])).any()
    assert S.valid_faces(v, np.array([[0, 1, 2], [0, 1, 6], [0, 1, 5], [0, 1, 1]])).tolist() == [True, False, False, True]
    assert S.vertex_normals(v[:0], np.zeros((0, 3), np.int64)).shape == (0, 3)
    # the order of the sum is part of the rule: the fan's apex adds 2 000 faces in ascending index
    fv, ff = S.fan(2000)
    S_apex = S.vertex_sums(fv, ff)[0]
    N = S.face_normals(fv, ff, np.arange(len(ff)))
    run = np.zeros(3)
    for k in range(len(ff)):
        run = run + N[k]
    assert np.array_equal(S_apex, run) and not np.array_equal(S_apex, N[::-1].cumsum(0)[-1])


# ------------------------------------------------------------------------------------------------------------ the chain
def test_the_chain_from_colour_frames_to_a_rendered_colour():
    """Ten colour frames of the box room (analytic wall colours, 33 x 47) -> tsdf_cpu fusion at 20 cm voxels -> marching cubes and
    vertex colours -> rendered from the same poses -> PSNR against the input frames over the pixels the mesh hits, both images
    times the mask and the mean over all pixels, as image_metrics scores it.  A description of the feature, not a gate on the
    device: measured 29.43 dB over the ten views at a coverage of 0.673."""
    ch = S.chain_case()
    _, face = R.render_depth(ch["vertices"], ch["faces"], ch["poses"], ch["K"], ch["H"], ch["W"])
    w = S.shade(ch["vertices"], ch["faces"], ch["poses"], ch["K"], face, ch["colors"], S.vertex_normals(ch["vertices"], ch["faces"]), S.SMOOTH)
    mask = (face >= 0) & (ch["depth"] > 0)
    a, b = w["color"].astype(np.float64) * mask[..., None], ch["rgb"].astype(np.float64) * mask[..., None]
    psnr = [-10.0 * math.log10(((a[k] - b[k]) ** 2).mean()) for k in range(len(a))]
    print(f"chain: {len(ch['vertices'])} vertices, {len(ch['faces'])} faces, coverage {mask.mean():.4f}, PSNR per view {[round(p, 2) for p in psnr]}, "
          f"mean {np.mean(psnr):.2f} dB; shaded mean {w['shaded'][face >= 0].mean():.3f}")
    assert w["record"][0] == int((face >= 0).sum()) and np.mean(psnr) > 20 and 0.5 < mask.mean() <= 1


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_library_and_package_agree():
    header = open(os.path.join(ROOT, "include", "mipsf_shade.h")).read()
    declared = set(re.findall(r"\b(mipsf_shade_[a-z0-9_]+)\s*\(", header))
    assert declared == {"mipsf_shade_workspace_bytes", "mipsf_shade_vertex_normals", "mipsf_shade_pixels"} == set(_lib.SHADE_SIGNATURES)
    assert not re.findall(r"\bmipsf_(raster|track)_[a-z0-9_]+\s*\(", header.split("#ifndef")[1])
    handle = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    for macro, value in (("MIPSF_SHADE_TILE", _lib.SHADE_TILE), ("MIPSF_SHADE_MAX_FACES", _lib.SHADE_MAX_FACES), ("MIPSF_SHADE_MAX_VERTICES", _lib.SHADE_MAX_VERTICES),
                         ("MIPSF_SHADE_MAX_SIDE", _lib.SHADE_MAX_SIDE), ("MIPSF_SHADE_MAX_PIXELS", _lib.SHADE_MAX_PIXELS), ("MIPSF_SHADE_MAX_ITEMS", _lib.SHADE_MAX_ITEMS),
                         ("MIPSF_SHADE_SHORT_SEGMENT", _lib.SHADE_SHORT_SEGMENT), ("MIPSF_SHADE_FLAT", _lib.SHADE_FLAT), ("MIPSF_SHADE_SMOOTH", _lib.SHADE_SMOOTH),
                         ("MIPSF_SHADE_RECORD_WORDS", _lib.SHADE_RECORD_WORDS)):
        text = re.search(rf"#define {macro} +\(?(0x[0-9a-f]+|\d+)u( << (\d+))?", header)
        assert int(text.group(1), 0) << int(text.group(3) or 0) == value, macro
    assert int(re.search(r"#define MIPSF_SHADE_WS_VERTEX_NORMALS +(\d+)", header).group(1)) == _lib.SHADE_WS_VERTEX_NORMALS
    assert (S.FLAT, S.SMOOTH) == (_lib.SHADE_FLAT, _lib.SHADE_SMOOTH)
    assert (_lib.SHADE_MAX_FACES, _lib.SHADE_MAX_SIDE, _lib.SHADE_MAX_PIXELS, _lib.SHADE_MAX_ITEMS) == (_lib.RASTER_MAX_FACES, _lib.RASTER_MAX_SIDE,
                                                                                                     _lib.RASTER_MAX_PIXELS, _lib.RASTER_MAX_ITEMS)
    # 4 words, 4 pointers; 8 words, 4 doubles, 4 floats, 10 pointers: what the header's structs come to on this ABI
    assert C.sizeof(_lib.ShadeVertexNormalsArgs) == 16 + 32 and C.sizeof(_lib.ShadePixelsArgs) == 32 + 32 + 16 + 80
    ws = _lib.lib().mipsf_shade_workspace_bytes
    assert ws(_lib.SHADE_WS_VERTEX_NORMALS, 8, 12) >= 2 * 4 * 8 + 4 * 36 and ws(_lib.SHADE_WS_VERTEX_NORMALS, 0, 0) > 0
    assert ws(_lib.SHADE_WS_VERTEX_NORMALS, 8, 12) % 16 == 0
    assert ws(_lib.SHADE_WS_VERTEX_NORMALS, _lib.SHADE_MAX_VERTICES + 1, 12) == 0 and ws(_lib.SHADE_WS_VERTEX_NORMALS, 8, _lib.SHADE_MAX_FACES + 1) == 0
    assert ws(0, 8, 12) == 0 and ws(2, 8, 12) == 0
    import mipsfusion_amd
    from mipsfusion_amd import mesh_render
    for name in ("render_mesh", "vertex_normals", "mesh_render_metrics", "MeshRender"):
        assert getattr(mipsfusion_amd, name) is getattr(mesh_render, name)
    assert "multiplies" in mesh_render.mesh_render_metrics.__doc__.lower() and "all pixels" in mesh_render.mesh_render_metrics.__doc__.lower()


FAKE = 0x1000                                   # never used: every call below is refused before a pointer is


def _pixels_block(**kw):
    a = dict(V=8, F=12, n=2, H=8, W=9, flags=_lib.SHADE_FLAT, fx=10.0, fy=10.0, cx=4.0, cy=4.0, vertices=FAKE, faces=FAKE, poses=FAKE, face=FAKE,
             record=FAKE)
    a.update(kw)
    return _lib.ShadePixelsArgs.new(**a)


def _normals_block(**kw):
    a = dict(V=8, F=12, vertices=FAKE, faces=FAKE, normals=FAKE, workspace=FAKE)
    a.update(kw)
    return _lib.ShadeVertexNormalsArgs.new(**a)


PIXELS_REFUSALS = [(dict(F=0), "without faces"), (dict(H=0), "no pixels"), (dict(W=0), "no pixels"), (dict(W=8193), "a side"), (dict(H=8193), "a side"),
                   (dict(F=(1 << 30) + 1), "faces, at most"), (dict(n=17, H=8192, W=8192), "pixels a call"), (dict(n=3, F=1 << 30), "pairs a call"),
                   (dict(fx=0.0), "intrinsics"), (dict(fy=math.inf), "intrinsics"), (dict(cx=math.nan), "intrinsics"), (dict(cy=math.inf), "intrinsics"),
                   (dict(flags=0), "flags"), (dict(flags=3), "flags"), (dict(flags=4), "flags"),
                   (dict(vertices=None), "null pointer"), (dict(faces=None), "null pointer"), (dict(poses=None), "null pointer"),
                   (dict(face=None), "null pointer"), (dict(record=None), "null pointer"), (dict(n=0, record=None), "null pointer"),
                   (dict(color=FAKE), "without vertex colours"), (dict(flags=_lib.SHADE_SMOOTH, normals=FAKE), "without vertex_normals"),
                   (dict(flags=_lib.SHADE_SMOOTH, shaded=FAKE), "without vertex_normals")]
NORMALS_REFUSALS = [(dict(V=0x80000000), "vertices, at most"), (dict(F=(1 << 30) + 1), "faces, at most"), (dict(vertices=None), "null pointer"),
                    (dict(faces=None), "null pointer"), (dict(normals=None), "null pointer"), (dict(workspace=None), "null pointer"),
                    (dict(V=0, F=0, workspace=None), "null pointer"), (dict(workspace=FAKE + 8), "16-byte")]


def _ids(refusals):
    return ["+".join(f"{k}={v}" for k, v in c.items()) for c, _ in refusals]


@pytest.mark.parametrize("change,said", PIXELS_REFUSALS, ids=_ids(PIXELS_REFUSALS))
def test_the_pixel_pass_refuses_what_is_out_of_range(change, said):
    lib = _lib.lib()
    assert lib.mipsf_shade_pixels(C.byref(_pixels_block(**change)), None) != 0
    assert b"mipsf_shade_pixels" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


@pytest.mark.parametrize("change,said", NORMALS_REFUSALS, ids=_ids(NORMALS_REFUSALS))
def test_the_vertex_normals_refuse_what_is_out_of_range(change, said):
    lib = _lib.lib()
    assert lib.mipsf_shade_vertex_normals(C.byref(_normals_block(**change)), None) != 0
    assert b"mipsf_shade_vertex_normals" in lib.mipsf_last_error() and said.encode() in lib.mipsf_last_error(), lib.mipsf_last_error()


def test_struct_sizes_are_checked():
    lib = _lib.lib()
    for cls, fn in ((_lib.ShadePixelsArgs, lib.mipsf_shade_pixels), (_lib.ShadeVertexNormalsArgs, lib.mipsf_shade_vertex_normals)):
        blk = cls.new()
        blk.struct_size -= 4
        assert fn(C.byref(blk), None) != 0 and b"struct_size" in lib.mipsf_last_error()
        assert fn(None, None) != 0 and b"null argument block" in lib.mipsf_last_error()
