"""The image-metric kernels (include/mipsf_image.h, mipsfusion_amd/image_metrics.py) against the float64 restatement of
tests/image_cpu.py: the records and the pooled images EQUAL it word for word, image_metrics equals its combination, refusals
launch nothing, the same call gives the same bytes, and render_metrics equals the pieces it is made of."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

from mipsfusion_amd import _lib, image_metrics as M

from . import image_cpu as I

pytestmark = pytest.mark.gpu
WINDOW = I.gaussian_window()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return torch.device("cuda:0")


def word(x):
    return struct.unpack("Q", struct.pack("d", x))[0]


def want_error(recs):
    return np.array([[word(r["sum_sq"]), word(r["sum_abs"]), word(r["max_abs"]), r["count"]] for r in recs], np.uint64)


def want_ssim(recs):
    return np.array([[word(r["sum_ssim"]), word(r["sum_cs"]), r["count"], 0] for r in recs], np.uint64)


def got_words(records):
    return records.cpu().numpy().view(np.uint64).reshape(records.shape[0], 4)


def device_records(a, b, rng, dev):
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    c = I.constants(rng)
    return (got_words(M.ssim_enqueue(ta, tb, WINDOW, *c)), got_words(M.error_enqueue(ta, tb)),
            M.pool_enqueue(ta).cpu().numpy().view(np.uint64))


def check(a, b, rng, dev, what, want=None):
    ssim, err, pool = device_records(a, b, rng, dev)
    c = I.constants(rng)
    w_ssim, w_err = want if want is not None else (I.ssim_records(a, b, WINDOW, *c), I.error_records(a, b))
    w_ssim, w_err, w_pool = want_ssim(w_ssim), want_error(w_err), I.pool2(a).view(np.uint64)
    print(f"{what}: differing words: ssim records {int((ssim != w_ssim).sum())}, error records {int((err != w_err).sum())}, "
          f"pool {int((pool != w_pool).sum())} of {pool.size}")
    assert np.array_equal(ssim, w_ssim), what
    assert np.array_equal(err, w_err), what
    assert pool.shape == w_pool.shape and np.array_equal(pool, w_pool), what


# ------------------------------------------------------------------------------------------------------------- 1. equality
@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("name", list(I.SSIM_SHAPES))
def test_records_and_pool_equal_the_restatement(dev, name, dtype):
    a, b = I.images(name, dtype)
    check(a, b, 1.0, dev, f"{name} {dtype}", I.reference_records(name, dtype))


@pytest.mark.parametrize("kind", [k for k in I.PLANTED if k != "uint8"])
def test_the_planted_cases(dev, kind):
    a, b, rng = I.planted(kind)
    check(a, b, rng, dev, kind)
    ssim, _, _ = device_records(a, b, rng, dev)
    if kind in ("identical", "constant"):
        assert (ssim[:, 0] == word(33.0 * 27.0)).all() and (ssim[:, 1] == word(33.0 * 27.0)).all()         # exactly 1.0 at every position
    swapped, err_swapped, _ = device_records(b, a, rng, dev)
    assert np.array_equal(ssim, swapped)
    assert np.array_equal(err_swapped, device_records(a, b, rng, dev)[1])


def test_an_error_stack_longer_than_one_round(dev):
    """more values a view than 256 blocks x 256 threads: the lanes take several rounds, and a pool of an odd and an even side"""
    g = np.random.default_rng(5)
    a = g.uniform(0, 1, (2, 161, 150, 3)).astype(np.float32)
    b = g.uniform(0, 1, (2, 161, 150, 3)).astype(np.float32)
    assert a[0].size > 256 * 256
    check(a, b, 1.0, dev, "161x150x3")


# ------------------------------------------------------------------------------------------------------------- 2. image_metrics
FIELDS = ("mse_per_view", "psnr_per_view", "l1_per_view", "ssim_per_view", "ms_ssim_per_view", "max_abs_per_view", "mse", "psnr", "l1",
          "ssim", "ms_ssim", "n_views", "shape")


def same(m, want):
    for f in FIELDS:
        g, w = getattr(m, f), want[f]
        assert g == w or (isinstance(w, float) and math.isnan(w) and math.isnan(g)), (f, g, w)


@pytest.mark.parametrize("name", list(I.METRIC_CASES))
def test_image_metrics_equals_the_restatement(dev, name, monkeypatch):
    a, b = I.metric_images(name)
    reads = []
    real = M.read_back
    monkeypatch.setattr(M, "read_back", lambda r: reads.append(tuple(r.shape)) or real(r))
    m = M.image_metrics(a, b)                                                      # host arrays
    n, H, W, Cc = a.shape
    assert reads == [(n + 5 * n * Cc, 32)], "one read-back a call"
    want = I.reference_metrics(name)
    print(name, "ssim", m.ssim_per_view, "ms_ssim", m.ms_ssim_per_view, "psnr", m.psnr_per_view)
    same(m, want)
    same(M.image_metrics(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)), want)       # device tensors
    assert M.ssim(a, b) == want["ssim"] and M.ms_ssim(a, b) == want["ms_ssim"] and M.psnr(a, b) == want["psnr"]
    same(M.image_metrics(a[0], b[0], ms_ssim=False), I.metrics(a[0], b[0], ms_ssim=False))           # a single image, [H,W,C]
    mask = np.random.default_rng(1).uniform(0, 1, a.shape[:3]) > 0.2
    same(M.image_metrics(a, b, mask=mask), I.metrics(a, b, mask=mask))


def test_image_metrics_takes_uint8_and_a_data_range_and_a_plain_image(dev):
    u, v, _ = I.planted("uint8")
    same(M.image_metrics(u, v, ms_ssim=False), I.metrics(u, v, ms_ssim=False))
    same(M.image_metrics(torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev), ms_ssim=False), I.metrics(u, v, ms_ssim=False))
    a, b, rng = I.planted("range255")
    same(M.image_metrics(a, b, data_range=rng, ms_ssim=False), I.metrics(a, b, rng, ms_ssim=False))
    same(M.image_metrics(a[0, :, :, 0], b[0, :, :, 0], data_range=rng, ms_ssim=False), I.metrics(a[0, :, :, 0], b[0, :, :, 0], rng, ms_ssim=False))
    m = M.image_metrics(a, a, data_range=rng, ms_ssim=False)
    assert m.psnr == math.inf and m.ssim == 1.0 and m.mse == 0.0
    g = np.random.default_rng(3)
    x = g.uniform(0, 1, (1, 161, 163, 1))
    assert M.image_metrics(x, 1.0 - x).ms_ssim == 0.0                              # negative cs means, clamped


def test_image_metrics_refuses_small_images(dev):
    x = np.zeros((160, 200, 3), np.float32)
    with pytest.raises(ValueError, match="160 x 200"):
        M.image_metrics(x, x, ms_ssim=True)
    assert M.image_metrics(x, x, ms_ssim=False).ssim == 1.0
    y = np.zeros((10, 40, 3), np.float32)
    with pytest.raises(ValueError, match="10 x 40"):
        M.image_metrics(y, y, ms_ssim=False)
    with pytest.raises(ValueError):
        M.image_metrics(x, y)
    with pytest.raises(ValueError):
        M.image_metrics(x.astype(np.int32), x.astype(np.int32))


# ------------------------------------------------------------------------------------------------------------- 3. refusals
def test_what_is_out_of_range_is_refused_on_the_host(dev):
    """refused with a message before anything is launched: the outputs keep the value they were filled with"""
    a = torch.rand(2, 20, 30, 3, device=dev)
    c = I.constants(1.0)
    rec = torch.full((6, 32), 7, dtype=torch.uint8, device=dev)
    pooled = torch.full((2, 10, 15, 3), -7.0, dtype=torch.float64, device=dev)
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="no place for a window"):
        M.ssim_enqueue(a[:, :10].contiguous(), a[:, :10].contiguous(), WINDOW, *c, out=rec)
    with pytest.raises(RuntimeError, match="no place for a window"):
        M.ssim_enqueue(a[:, :, :10].contiguous(), a[:, :, :10].contiguous(), WINDOW, *c, out=rec)
    with pytest.raises(RuntimeError, match="at least one of each"):
        M.ssim_enqueue(a[:0], a[:0], WINDOW, *c)
    with pytest.raises(RuntimeError, match="at least one of each"):
        M.error_enqueue(a[:, :, :, :0], a[:, :, :, :0])
    with pytest.raises(RuntimeError, match="no pixels"):
        M.error_enqueue(a[:, :0], a[:, :0], out=rec[:2])
    with pytest.raises(RuntimeError, match="no pixels"):
        M.pool_enqueue(a[:, :, :0])
    five = torch.rand(1, 12, 12, 5, device=dev)
    with pytest.raises(RuntimeError, match="at most 4 channels"):
        M.error_enqueue(five, five)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        M.ssim_enqueue(a, a, WINDOW, *c, out=rec, workspace=ws[8:])
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        M.error_enqueue(a, a, out=rec[:2], workspace=ws[8:])
    # through the C ABI itself: a null pointer, a bad dtype, a bad struct_size, too many values
    args = _lib.ImageSsimArgs.new(n=2, H=20, W=30, C=3, dtype=_lib.IMAGE_F32, window=(C.c_double * 11)(*WINDOW), C1=c[0], C2=c[1],
                                  a=a.data_ptr(), b=None, records=rec.data_ptr(), workspace=ws.data_ptr())
    assert lib.mipsf_image_ssim(C.byref(args), _lib.stream_ptr()) != 0 and b"null pointer" in lib.mipsf_last_error()
    args.b, args.dtype = a.data_ptr(), 2
    assert lib.mipsf_image_ssim(C.byref(args), _lib.stream_ptr()) != 0 and b"dtype" in lib.mipsf_last_error()
    args.dtype, args.struct_size = _lib.IMAGE_F32, 8
    assert lib.mipsf_image_ssim(C.byref(args), _lib.stream_ptr()) != 0 and b"struct_size" in lib.mipsf_last_error()
    big = _lib.ImagePool2Args.new(n=64, H=4096, W=4096, C=4, dtype=_lib.IMAGE_F32, in_=a.data_ptr(), out=pooled.data_ptr())
    assert lib.mipsf_image_pool2(C.byref(big), _lib.stream_ptr()) != 0 and b"values a call" in lib.mipsf_last_error()
    big = _lib.ImagePool2Args.new(n=2, H=20, W=30, C=3, dtype=_lib.IMAGE_F32, in_=None, out=pooled.data_ptr())
    assert lib.mipsf_image_pool2(C.byref(big), _lib.stream_ptr()) != 0 and b"null pointer" in lib.mipsf_last_error()
    wide = _lib.ImageErrorArgs.new(n=1, H=_lib.IMAGE_MAX_SIDE + 1, W=1, C=1, dtype=_lib.IMAGE_F32, a=a.data_ptr(), b=a.data_ptr(),
                                   records=rec.data_ptr(), workspace=ws.data_ptr())
    assert lib.mipsf_image_error(C.byref(wide), _lib.stream_ptr()) != 0 and b"8192 a side" in lib.mipsf_last_error()
    torch.cuda.synchronize()
    assert bool((rec == 7).all()) and bool((pooled == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- 4. repeatability
def test_the_same_call_gives_the_same_bytes_and_a_cut_changes_nothing(dev):
    a, b = (torch.from_numpy(x).to(dev) for x in I.images("43x37x3n3"))
    c = I.constants(1.0)
    s1, s2 = M.ssim_enqueue(a, b, WINDOW, *c), M.ssim_enqueue(a, b, WINDOW, *c)
    e1, e2 = M.error_enqueue(a, b), M.error_enqueue(a, b)
    p1, p2 = M.pool_enqueue(a), M.pool_enqueue(a)
    assert torch.equal(s1, s2) and torch.equal(e1, e2) and torch.equal(p1.view(torch.int64), p2.view(torch.int64))
    cut = torch.cat([M.ssim_enqueue(a[:1], b[:1], WINDOW, *c), M.ssim_enqueue(a[1:], b[1:], WINDOW, *c)])
    assert torch.equal(cut, s1)
    assert torch.equal(torch.cat([M.error_enqueue(a[:2], b[:2]), M.error_enqueue(a[2:], b[2:])]), e1)
    assert torch.equal(torch.cat([M.pool_enqueue(a[:2]), M.pool_enqueue(a[2:])]).view(torch.int64), p1.view(torch.int64))
    x, y = I.metric_images("176x162x1")
    assert M.image_metrics(x, y) == M.image_metrics(x, y)


# ------------------------------------------------------------------------------------------------------------- 5. render_metrics
def test_render_metrics_equals_its_pieces(dev):
    """two frames of the plumbing scene cut to 24 x 32 pixels: render_metrics equals image_metrics and the depth expression applied to
    render_full_img's own outputs, whatever the chunking"""
    from mipsfusion_amd import inference, mesh_render, synth
    from mipsfusion_amd.model import JointEncoding
    from .conftest import load_golden
    g = load_golden("scene_cfg1.npz")
    cfg = synth.config_plumbing()
    model = JointEncoding(cfg, torch.from_numpy(np.asarray(g["bound"])), torch.from_numpy(np.asarray(g["half_len"]))).to(dev)
    model.load_state_dict({k[2:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("w.")})
    model.eval()
    frames = [synth.make_frame(cfg, seed=2), synth.make_frame(cfg, seed=3, frame_id=1)]
    assert frames[0]["depth"].shape == (32, 32)
    H, W = 24, 32                                                                  # the upper 24 rows: H != W shows a mixed-up axis
    frames = [{k: (v[:H].contiguous() if k in ("depth", "rgb", "direction") else v) for k, v in f.items()} for f in frames]
    S = cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"]
    torch.manual_seed(3)
    noise = torch.rand(H * W, S).to(dev)
    depth = [f["depth"].clone() for f in frames]
    depth[1][:3] = 0                                                               # pixels without captured depth
    poses, rgb = torch.stack([f["c2w"] for f in frames]), torch.stack([f["rgb"] for f in frames])
    got = M.render_metrics(model, frames[0]["direction"], poses, rgb, depth, H, W, ray_batch_size=300, ms_ssim=False, noise=noise)
    pred, pred_d = zip(*[inference.render_full_img(model, frames[0]["direction"], poses[k], depth[k], H, W, ray_batch_size=300, noise=noise)
                         for k in range(2)])
    want = M.image_metrics(torch.stack(pred), rgb, ms_ssim=False)
    assert got.image == want and got.n_views == 2 and want.shape == (H, W, 3)
    assert all(math.isfinite(v) for v in want.psnr_per_view) and all(-1 <= v <= 1 for v in want.ssim_per_view)
    want_d = []
    for k in range(2):
        gt_d = depth[k].to(dev, torch.float32)
        p = torch.where(gt_d == 0, torch.zeros_like(pred_d[k]), pred_d[k])
        r = mesh_render.read_l1_records(mesh_render.l1_enqueue(p[None].contiguous(), gt_d[None].contiguous()))[0]
        assert r.both + r.gt_only == int((gt_d != 0).sum()) and r.rec_only == 0
        want_d.append(r.sum_all / (r.both + r.gt_only))
        plain = float((pred_d[k].double() - gt_d.double()).abs()[gt_d > 0].mean())
        assert abs(want_d[-1] - plain) <= 1e-12 * max(plain, 1.0)
    assert got.depth_l1_per_view == tuple(want_d) and got.depth_l1 == math.fsum(want_d) / 2
    assert M.render_metrics(model, frames[0]["direction"], poses, rgb, depth, H, W, ray_batch_size=300, ms_ssim=False, noise=noise, chunk=1) == got
    with pytest.raises(ValueError, match="MS-SSIM"):
        M.render_metrics(model, frames[0]["direction"], poses, rgb, depth, H, W, ms_ssim=True, noise=noise)
