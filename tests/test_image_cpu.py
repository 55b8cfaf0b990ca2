"""tests/image_cpu.py, the float64 restatement of include/mipsf_image.h, held to five conditions without a GPU: (a) torch's grouped
conv2d and avg_pool2d in float64, (b) the planted cases, (c) the pyramid's shapes, (d) the host build of the device's own
per-pixel arithmetic (tools/image_host.hip), word for word, (e) PSNR and L1 against the plain numpy expressions."""
import math
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mipsfusion_amd import _lib

from . import image_cpu as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = I.gaussian_window()
C1, C2 = I.constants(1.0)


def words(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def torch_maps(a, b, window, c1, c2):
    """the conv2d formulation: the outer-product window, one group per channel, float64"""
    x, y = (torch.from_numpy(np.moveaxis(I.as_stack(v), 3, 1).copy()) for v in (a, b))
    C = x.shape[1]
    w = torch.from_numpy(np.outer(window, window))[None, None].repeat(C, 1, 1, 1)
    f = lambda q: F.conv2d(q, w, groups=C)                                  # noqa: E731
    m1, m2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - m1 * m1, f(y * y) - m2 * m2, f(x * y) - m1 * m2
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    return (((2 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1)) * cs).numpy(), cs.numpy()


# ---------------------------------------------------------------------------------------------------------------- (a)
def test_maps_and_pool_agree_with_torch():
    """Gates: 1e-12 on every ssim and cs value, 1e-15 on the pool: 100 x and 10 x the 1.1e-14 and 1.1e-16 first measured up to
    176 x 162.  On the cases here, all of uniform noise (a window's variance stands in cs's denominator beside C2 = 9e-4: on smooth
    images the rounding of the 121 products is amplified a thousandfold and 4e-13 .. 8e-13 was measured): 2.1e-14 and 0."""
    worst_map = worst_pool = 0.0
    cases = [I.images(name) for name in I.SSIM_SHAPES] + [I.metric_images(name) for name in I.METRIC_CASES]
    for a, b in cases:
        ssim, cs = I.ssim_maps(a, b, WINDOW, C1, C2)
        t_ssim, t_cs = torch_maps(a, b, WINDOW, C1, C2)
        assert ssim.shape == t_ssim.shape == (a.shape[0], a.shape[3], a.shape[1] - 10, a.shape[2] - 10)
        here = max(float(np.abs(ssim - t_ssim).max()), float(np.abs(cs - t_cs).max()))
        print(a.shape, f"maps {here:.2e}")
        worst_map = max(worst_map, here)
        x = torch.from_numpy(np.moveaxis(I.as_stack(a), 3, 1).copy())
        want = F.avg_pool2d(x, 2, padding=(a.shape[1] % 2, a.shape[2] % 2), count_include_pad=True).numpy()
        got = np.moveaxis(I.pool2(a), 3, 1)
        assert got.shape == want.shape
        worst_pool = max(worst_pool, float(np.abs(got - want).max()))
    print(f"largest difference to torch: maps {worst_map:.2e}, pool {worst_pool:.2e}")
    assert worst_map <= 1e-12 and worst_pool <= 1e-15


def test_the_window():
    assert WINDOW.shape == (11,) and abs(WINDOW.sum() - 1.0) < 1e-15 and np.array_equal(WINDOW, WINDOW[::-1])
    assert WINDOW[5] == WINDOW.max() and abs(WINDOW[4] / WINDOW[5] - math.exp(-1 / 4.5)) < 1e-15
    from mipsfusion_amd import image_metrics as M
    assert np.array_equal(np.array(M.gaussian_window()), WINDOW) and M.ssim_constants(255.0) == I.constants(255.0)
    assert M.MS_WEIGHTS == I.MS_WEIGHTS


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_identical_images_are_exactly_one(dtype):
    for kind in ("identical", "constant"):
        a, b, rng = I.planted(kind, dtype)
        ssim, cs = I.ssim_maps(a, b, WINDOW, *I.constants(rng))
        assert (ssim == 1.0).all() and (cs == 1.0).all(), kind
        recs = I.ssim_records(a, b, WINDOW, *I.constants(rng))
        assert all(r["sum_ssim"] == r["count"] == r["sum_cs"] == 33 * 27 for r in recs)
        e = I.error_records(a, b)
        assert all(r["sum_sq"] == 0.0 and r["sum_abs"] == 0.0 and r["max_abs"] == 0.0 for r in e)
    a, _, _ = I.planted("identical", dtype)
    big = I.metrics(np.tile(a, (1, 4, 5, 1))[:1, :161, :163], np.tile(a, (1, 4, 5, 1))[:1, :161, :163])
    assert big["ssim"] == 1.0 and big["ms_ssim"] == 1.0 and big["psnr"] == math.inf and big["mse"] == 0.0


def test_swapped_arguments_give_identical_words():
    for kind in ("swapped", "outside", "range255"):
        a, b, rng = I.planted(kind)
        c = I.constants(rng)
        for x, y in zip(I.ssim_maps(a, b, WINDOW, *c), I.ssim_maps(b, a, WINDOW, *c)):
            assert np.array_equal(words(x), words(y))
        assert I.ssim_records(a, b, WINDOW, *c) == I.ssim_records(b, a, WINDOW, *c)
        assert I.error_records(a, b) == I.error_records(b, a)


def test_an_inverted_image_has_negative_cs_and_ms_ssim_zero():
    g = np.random.default_rng(3)
    a = g.uniform(0, 1, (1, 161, 163, 1))
    m = I.metrics(a, 1.0 - a)
    cs_means = [lv[0]["sum_cs"] / lv[0]["count"] for lv in m["levels"]]
    print("cs means of b = 1 - a:", cs_means)
    assert all(v < 0 for v in cs_means[:4]) and abs(cs_means[0] + 0.99) < 0.01           # the levels MS-SSIM takes the cs mean of
    assert m["ms_ssim"] == 0.0 and m["ms_ssim_per_view"] == (0.0,)
    assert m["ssim"] < 0


def test_values_outside_the_unit_range_and_uint8():
    a, b, rng = I.planted("outside")
    assert a.min() < 0 and a.max() > 1
    ssim, cs = I.ssim_maps(a, b, WINDOW, *I.constants(rng))
    assert np.isfinite(ssim).all() and (np.abs(ssim) <= 1).all()
    # data_range = 255 on images scaled by 255 gives the numbers of the unit range, up to the rounding of the scale
    a1, b1, _ = I.planted("swapped", "float64")
    a255, b255 = a1 * 255.0, b1 * 255.0
    s1 = I.metrics(a1, b1, 1.0, ms_ssim=False)
    s255 = I.metrics(a255, b255, 255.0, ms_ssim=False)
    assert abs(s1["ssim"] - s255["ssim"]) < 1e-12 and abs(s1["psnr"] - s255["psnr"]) < 1e-10
    # uint8 is divided by 255 in float64
    u, v, _ = I.planted("uint8")
    assert u.dtype == np.uint8
    m8 = I.metrics(u, v, ms_ssim=False)
    mf = I.metrics(u.astype(np.float64) / 255.0, v.astype(np.float64) / 255.0, ms_ssim=False)
    assert m8["ssim_per_view"] == mf["ssim_per_view"] and m8["psnr_per_view"] == mf["psnr_per_view"]


# ---------------------------------------------------------------------------------------------------------------- (c)
def test_the_pyramid_s_shapes():
    for (H, W), want in (((161, 163), [(81, 82), (41, 41), (21, 21), (11, 11)]), ((176, 162), [(88, 81), (44, 41), (22, 21), (11, 11)])):
        x = np.random.default_rng(0).uniform(0, 1, (1, H, W, 2))
        got = []
        for _ in range(4):
            x = I.pool2(x)
            got.append(x.shape[1:3])
            assert x.shape[1:3] == (I.pool_out(got[-2][0] if len(got) > 1 else H), I.pool_out(got[-2][1] if len(got) > 1 else W))
        assert got == want
    # the last level is a single window
    a, b = I.metric_images("161x163x3n2")
    m = I.reference_metrics("161x163x3n2")
    assert [lv[0]["count"] for lv in m["levels"]] == [151 * 153, 71 * 72, 31 * 31, 11 * 11, 1]
    assert all(0 < v < 1 for v in m["ms_ssim_per_view"]) and all(0 < v < 1 for v in m["ssim_per_view"])
    # an odd side is padded on BOTH ends, a last row without a partner is dropped
    x = np.arange(15.0).reshape(1, 3, 5, 1)
    p = I.pool2(x)[0, :, :, 0]
    assert p.shape == (2, 3)
    assert p[0, 0] == x[0, 0, 0, 0] * 0.25 and p[0, 1] == (x[0, 0, 1, 0] + x[0, 0, 2, 0]) * 0.25
    assert p[1, 2] == ((x[0, 1, 3, 0] + x[0, 1, 4, 0]) + (x[0, 2, 3, 0] + x[0, 2, 4, 0])) * 0.25


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    """tools/image_host.hip: image_dev.h compiled for the host, driven by the kernels' loops"""
    import shutil
    import subprocess
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("image_host")
    exe = str(d / "image_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "image_host.hip"), "-o", exe], check=True)

    def run(a, b, window, c1, c2):
        n, H, W, C = a.shape
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64)
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("6I", n, H, W, C, int(a.dtype == np.float64), 0) + struct.pack("13d", *window, c1, c2))
            f.write(np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(b).tobytes())
        subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], check=True, capture_output=True, text=True)
        raw = np.fromfile(d / "out.bin", np.uint64)
        out, at = {}, 0
        out["errors"] = raw[at:at + 4 * n].reshape(n, 4)
        at += 4 * n
        m = n * I.pool_out(H) * I.pool_out(W) * C
        out["pool"] = raw[at:at + m].reshape(n, I.pool_out(H), I.pool_out(W), C)
        at += m
        if H >= 11 and W >= 11:
            m = n * C * (H - 10) * (W - 10)
            out["ssim"], out["cs"] = raw[at:at + m].reshape(n, C, H - 10, W - 10), raw[at + m:at + 2 * m].reshape(n, C, H - 10, W - 10)
            at += 2 * m
            out["records"] = raw[at:at + 4 * n * C].reshape(n * C, 4)
            at += 4 * n * C
        assert at == raw.size
        return out
    return run


def word(x):
    return struct.unpack("Q", struct.pack("d", x))[0]


def error_words(recs):
    return np.array([[word(r["sum_sq"]), word(r["sum_abs"]), word(r["max_abs"]), r["count"]] for r in recs], np.uint64)


def ssim_words(recs):
    return np.array([[word(r["sum_ssim"]), word(r["sum_cs"]), r["count"], 0] for r in recs], np.uint64)


def check_host(host_build, a, b, rng=1.0):
    c = I.constants(rng)
    got = host_build(a, b, WINDOW, *c)
    ssim, cs = I.ssim_maps(a, b, WINDOW, *c)
    assert np.array_equal(got["ssim"], words(ssim)) and np.array_equal(got["cs"], words(cs))
    assert np.array_equal(got["records"], ssim_words(I.ssim_records(a, b, WINDOW, *c)))
    assert np.array_equal(got["errors"], error_words(I.error_records(a, b)))
    assert np.array_equal(got["pool"], words(I.pool2(a)))


@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("name", list(I.SSIM_SHAPES))
def test_the_host_build_gives_the_restatement_s_words(host_build, name, dtype):
    check_host(host_build, *I.images(name, dtype))


@pytest.mark.parametrize("kind", [k for k in I.PLANTED if k != "uint8"])
def test_the_host_build_on_the_planted_cases(host_build, kind):
    check_host(host_build, *I.planted(kind))


def test_the_host_build_on_one_pyramid(host_build):
    a, b = I.metric_images("161x163x3n2")
    for level in range(5):
        check_host(host_build, a, b)
        a, b = I.pool2(a), I.pool2(b)
    assert a.shape[1:3] == (6, 6)


# ---------------------------------------------------------------------------------------------------------------- (e)
def test_psnr_and_l1_against_plain_numpy():
    """a fixed-order sum of m non-negative terms differs from the exact one by at most m * 2^-53 relative (as distance_stats)"""
    for a, b in [I.images(name) for name in I.SSIM_SHAPES] + [I.metric_images(name) for name in I.METRIC_CASES]:
        m = I.metrics(a, b, ms_ssim=False)
        for v in range(a.shape[0]):
            d = a[v].astype(np.float64) - b[v].astype(np.float64)
            gate = d.size * 2.0 ** -53
            mse, l1 = math.fsum((d * d).ravel()) / d.size, math.fsum(np.abs(d).ravel()) / d.size
            assert abs(m["mse_per_view"][v] - mse) <= gate * mse and abs(m["l1_per_view"][v] - l1) <= gate * l1
            assert m["max_abs_per_view"][v] == np.abs(d).max()
            # the sum's gate through d(10 log10 x) = 10 / (x ln 10) dx, plus 4 ulp of a value below 32 for the logarithm and the product
            assert abs(m["psnr_per_view"][v] - (-10 * math.log10(mse))) <= 10 * gate / math.log(10) + 4 * 2.0 ** -48
            assert abs(m["psnr_per_view"][v] - 10 * np.log10(1.0 / np.mean(d * d))) < 1e-10


# ---------------------------------------------------------------------------------------------------------------- the library
def test_the_library_exports_the_image_metrics():
    lib = _lib.lib()
    for name in _lib.IMAGE_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.mipsf_image_workspace_bytes(_lib.IMAGE_WS_SSIM, 2, 3, 43, 37) == 2 * 3 * 3 * 1 * 16
    assert lib.mipsf_image_workspace_bytes(_lib.IMAGE_WS_ERROR, 2, 3, 43, 37) == 2 * 19 * 32
    assert lib.mipsf_image_workspace_bytes(_lib.IMAGE_WS_ERROR, 1, 3, 460, 620) == 256 * 32
    for bad in ((0, 3, 43, 37), (1, 0, 43, 37), (1, 5, 43, 37), (1, 3, 0, 37), (1, 3, 10, 37), (1, 3, 43, 10), (1, 1, _lib.IMAGE_MAX_SIDE + 1, 11),
                (65536, 1, 11, 11), (16384, 4, 11, 11), (64, 4, 4096, 4096)):
        assert lib.mipsf_image_workspace_bytes(_lib.IMAGE_WS_SSIM, *bad) == 0, bad
    assert lib.mipsf_image_workspace_bytes(_lib.IMAGE_WS_ERROR, 1, 3, 10, 37) > 0          # only the window needs 11
    assert lib.mipsf_image_workspace_bytes(3, 1, 3, 43, 37) == 0
    assert (_lib.IMAGE_TILE_H, _lib.IMAGE_TILE_W, _lib.IMAGE_ERROR_MAX_BLOCKS) == (I.TILE_H, I.TILE_W, I.ERROR_MAX_BLOCKS)
    import ctypes as C
    assert C.sizeof(_lib.ImageErrorRecord) == _lib.IMAGE_ERROR_RECORD_BYTES and C.sizeof(_lib.ImageSsimRecord) == _lib.IMAGE_SSIM_RECORD_BYTES
    assert (C.sizeof(_lib.ImageErrorArgs), C.sizeof(_lib.ImageSsimArgs), C.sizeof(_lib.ImagePool2Args)) == (56, 160, 40)
    import mipsfusion_amd
    assert callable(mipsfusion_amd.psnr) and callable(mipsfusion_amd.ssim) and callable(mipsfusion_amd.ms_ssim)
    assert callable(mipsfusion_amd.image_metrics.image_metrics) and callable(mipsfusion_amd.render_metrics)
