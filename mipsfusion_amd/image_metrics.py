"""Rendered frames scored against captured ones: MSE / PSNR / L1, SSIM and MS-SSIM of image stacks, and ``render_metrics`` for
the frames of a sequence.  Every windowed moment and every sum is a HIP kernel of ``csrc/image.hip`` (C ABI:
include/mipsf_image.h); the few sums per view are combined on the host in Python float64 from ONE read-back.

    image_metrics       two stacks [n,H,W,C] -> ImageMetrics (per view and mean: mse, psnr, l1, ssim, ms_ssim)
    psnr, ssim, ms_ssim the mean of one of them
    render_metrics      a model's renders of captured frames -> RenderMetrics (the above for the colour, depth L1)

This is the Gaussian-window (11 taps, sigma 1.5), valid-region SSIM / MS-SSIM of the published NeRF-SLAM evaluations, restated
from the formula; it is not pinned to any package.  It is NOT the zero-padded "same" SSIM of the Gaussian-splatting code bases,
whose numbers differ at the border.  LPIPS needs network weights and is out of scope.  The records EQUAL those of the float64
restatement in tests/image_cpu.py: the header fixes every operation and the order of every sum.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import pose_corrector as pc
from .evaluate import _device

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_MIN_SIDE = 161                    # five levels of 2 x 2 means leave an 11 x 11 window's place only from this side on


class ImageMetrics(NamedTuple):
    mse: float                       # means over the views
    psnr: float
    l1: float
    ssim: float
    ms_ssim: float                   # nan when it was not asked for
    mse_per_view: Tuple[float, ...]
    psnr_per_view: Tuple[float, ...]         # -10*log10(mse / data_range^2); inf for an exact match
    l1_per_view: Tuple[float, ...]
    ssim_per_view: Tuple[float, ...]         # the mean over the channels of sum_ssim / count
    ms_ssim_per_view: Tuple[float, ...]      # empty when it was not asked for
    max_abs_per_view: Tuple[float, ...]
    n_views: int
    shape: Tuple[int, int, int]              # H, W, C


class RenderMetrics(NamedTuple):
    image: ImageMetrics                      # the rendered colour against the captured one
    depth_l1: float                          # mean over the frames of depth_l1_per_view, metres
    depth_l1_per_view: Tuple[float, ...]     # mean |rendered - captured| over the pixels with captured depth > 0; nan when none
    n_views: int


def gaussian_window() -> Tuple[float, ...]:
    """the 11 weights: g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), summed ascending, each divided by the sum: Python float64"""
    g = [math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)]
    s = 0.0
    for v in g:
        s += v
    return tuple(v / s for v in g)


def ssim_constants(data_range: float) -> Tuple[float, float]:
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


# --------------------------------------------------------------------------------------------------------------- inputs
def _stack(x, what: str, dev=None) -> torch.Tensor:
    """-> fp32 or fp64 [n,H,W,C] on the device, contiguous; uint8 is divided by 255 in float64"""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() == 2:
        t = t[None, :, :, None]
    elif t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"{what}: expected [n,H,W,C], [H,W,C] or [H,W], got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(_device() if dev is None else dev)
    if t.dtype == torch.uint8:
        t = t.to(torch.float64) / 255.0
    elif t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: expected float32, float64 or uint8, got {t.dtype}")
    return t.contiguous()


def _pair(pred, gt, mask=None):
    a = _stack(pred, "pred")
    b = _stack(gt, "gt", a.device)
    if a.shape != b.shape:
        raise ValueError(f"pred and gt: {tuple(a.shape)} against {tuple(b.shape)}")
    if b.device != a.device:
        b = b.to(a.device)
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
        if m.dim() == 2:
            m = m[None]
        if tuple(m.shape) != tuple(a.shape[:3]):
            raise ValueError(f"mask: expected {tuple(a.shape[:3])}, got {tuple(m.shape)}")
        m = m.to(a.device).to(torch.float64)[..., None]
        a, b = (a.to(torch.float64) * m).contiguous(), (b.to(torch.float64) * m).contiguous()
    if a.dtype != b.dtype:
        a, b = a.to(torch.float64), b.to(torch.float64)
    return a, b


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.IMAGE_F32
    if t.dtype == torch.float64:
        return _lib.IMAGE_F64
    raise RuntimeError(f"expected float32 or float64, got {t.dtype}")


def _check_pair(a: torch.Tensor, b: torch.Tensor):
    _lib.dptr(a, a.dtype), _lib.dptr(b, a.dtype)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"image stacks: expected two of [n,H,W,C], got {tuple(a.shape)} and {tuple(b.shape)}")
    return tuple(int(s) for s in a.shape)


def _workspace(which: int, n: int, Cc: int, H: int, W: int, dev) -> torch.Tensor:
    # what is out of range has no workspace size: a granule is handed over and the library refuses with its own message
    size = int(_lib.lib().mipsf_image_workspace_bytes(which, n, Cc, H, W)) if 0 <= min(n, Cc, H, W) and max(n, Cc, H, W) < 1 << 32 else 0
    return pc._bytes(max(size, 16), dev)


def _records(out: Optional[torch.Tensor], rows: int, width: int, dev) -> torch.Tensor:
    if out is None:
        return torch.zeros(max(rows, 1), width, dtype=torch.uint8, device=dev)[:rows]
    if out.dtype != torch.uint8 or tuple(out.shape) != (rows, width) or not out.is_contiguous():
        raise ValueError(f"records: expected contiguous uint8 [{rows},{width}]")
    return out


# --------------------------------------------------------------------------------------------------------------- enqueue only
def error_enqueue(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, workspace=None) -> torch.Tensor:
    """two stacks [n,H,W,C] of one dtype on the device -> records uint8 [n,32] = mipsf_image_error_record per view, on the device"""
    n, H, W, Cc = _check_pair(a, b)
    dev = a.device
    with torch.cuda.device(dev):
        records = _records(out, n, _lib.IMAGE_ERROR_RECORD_BYTES, dev)
        ws = _workspace(_lib.IMAGE_WS_ERROR, n, Cc, H, W, dev) if workspace is None else workspace
        args = _lib.ImageErrorArgs.new(n=n, H=H, W=W, C=Cc, dtype=_dtype_code(a), a=a.data_ptr(), b=b.data_ptr(),
                                       records=records.data_ptr(), workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_image_error(C.byref(args), _lib.stream_ptr()), "image_error")
    return records


def ssim_enqueue(a: torch.Tensor, b: torch.Tensor, window, C1: float, C2: float, out: Optional[torch.Tensor] = None,
                 workspace=None) -> torch.Tensor:
    """-> records uint8 [n*C,32] = mipsf_image_ssim_record per (view, channel), on the device; window: the 11 weights"""
    n, H, W, Cc = _check_pair(a, b)
    if len(window) != _lib.IMAGE_WINDOW:
        raise ValueError(f"window: expected {_lib.IMAGE_WINDOW} weights")
    dev = a.device
    with torch.cuda.device(dev):
        records = _records(out, n * Cc, _lib.IMAGE_SSIM_RECORD_BYTES, dev)
        ws = _workspace(_lib.IMAGE_WS_SSIM, n, Cc, H, W, dev) if workspace is None else workspace
        args = _lib.ImageSsimArgs.new(n=n, H=H, W=W, C=Cc, dtype=_dtype_code(a), window=(C.c_double * 11)(*[float(w) for w in window]),
                                      C1=float(C1), C2=float(C2), a=a.data_ptr(), b=b.data_ptr(), records=records.data_ptr(),
                                      workspace=ws.data_ptr())
        _lib.check(_lib.lib().mipsf_image_ssim(C.byref(args), _lib.stream_ptr()), "image_ssim")
    return records


def pool_out(side: int) -> int:
    return (side + 2 * (side % 2) - 2) // 2 + 1


def pool_enqueue(x: torch.Tensor) -> torch.Tensor:
    """a stack [n,H,W,C] on the device -> its 2 x 2 mean fp64 [n,Ho,Wo,C] (an odd side zero-padded by one on both ends)"""
    _lib.dptr(x, x.dtype)
    if x.dim() != 4:
        raise ValueError(f"image stack: expected [n,H,W,C], got {tuple(x.shape)}")
    n, H, W, Cc = (int(s) for s in x.shape)
    dev = x.device
    with torch.cuda.device(dev):
        Ho, Wo = (pool_out(H), pool_out(W)) if H > 0 and W > 0 else (0, 0)
        out = torch.empty(max(n * Ho * Wo * Cc, 1), dtype=torch.float64, device=dev)[:n * Ho * Wo * Cc].view(n, Ho, Wo, Cc)
        args = _lib.ImagePool2Args.new(n=n, H=H, W=W, C=Cc, dtype=_dtype_code(x), in_=x.data_ptr(), out=out.data_ptr())
        _lib.check(_lib.lib().mipsf_image_pool2(C.byref(args), _lib.stream_ptr()), "image_pool2")
    return out


def read_back(records: torch.Tensor) -> bytes:
    """the one device-to-host copy of a call"""
    return records.cpu().numpy().tobytes()


def read_error_records(raw: bytes, n: int, offset: int = 0):
    size = _lib.IMAGE_ERROR_RECORD_BYTES
    return [_lib.ImageErrorRecord.from_buffer_copy(raw[offset + k * size:offset + (k + 1) * size]) for k in range(n)]


def read_ssim_records(raw: bytes, n: int, offset: int = 0):
    size = _lib.IMAGE_SSIM_RECORD_BYTES
    return [_lib.ImageSsimRecord.from_buffer_copy(raw[offset + k * size:offset + (k + 1) * size]) for k in range(n)]


# --------------------------------------------------------------------------------------------------------------- public
def combine(errors, levels, n: int, shape, data_range: float) -> ImageMetrics:
    """The records of one call -> ImageMetrics, in Python float64.  errors: n error records; levels: per pyramid level the n*C
    SSIM records (one level: SSIM only; five: MS-SSIM too)."""
    H, W, Cc = shape
    mse = tuple(r.sum_sq / r.count for r in errors)
    l1 = tuple(r.sum_abs / r.count for r in errors)
    psnr = tuple(-10.0 * math.log10(m / data_range ** 2) if m > 0 else (math.inf if m == 0 else math.nan) for m in mse)
    ssim_v, ms_v = [], []
    for v in range(n):
        s = 0.0
        for c in range(Cc):
            r = levels[0][v * Cc + c]
            s += r.sum_ssim / r.count
        ssim_v.append(s / Cc)
        if len(levels) > 1:
            s = 0.0
            for c in range(Cc):
                prod = 1.0
                for i, w in enumerate(MS_WEIGHTS):
                    r = levels[i][v * Cc + c]
                    val = (r.sum_cs if i + 1 < len(MS_WEIGHTS) else r.sum_ssim) / r.count
                    prod = prod * (max(val, 0.0) ** w)
                s += prod
            ms_v.append(s / Cc)
    mean = lambda x: math.fsum(x) / n                                                      # noqa: E731
    return ImageMetrics(mean(mse), mean(psnr), mean(l1), mean(ssim_v), mean(ms_v) if ms_v else math.nan, mse, psnr, l1, tuple(ssim_v),
                        tuple(ms_v), tuple(r.max_abs for r in errors), n, (H, W, Cc))


def image_metrics(pred, gt, data_range: float = 1.0, ms_ssim: bool = True, mask=None) -> ImageMetrics:
    """Two image stacks -> ImageMetrics.  pred, gt: fp32 / fp64 / uint8 tensors or arrays [n,H,W,C], [H,W,C] or [H,W], on the host
    or on the device; uint8 is divided by 255 in float64.  mask [n,H,W], if given, multiplies both images first (in float64), as the
    published evaluations apply a valid-depth mask; the metrics are then over ALL pixels.  SSIM: 11-tap Gaussian window of sigma 1.5,
    valid region, C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2, mean over positions, then over channels.  MS-SSIM: five levels
    of 2 x 2 means with the weights MS_WEIGHTS, per channel prod_i max(v_i, 0)^w_i with v_i the cs mean on levels 0..3 and the ssim
    mean on level 4, then the mean over channels; it needs min(H, W) > 160 (``ms_ssim=False`` skips it).  One read-back a call."""
    a, b = _pair(pred, gt, mask)
    n, H, W, Cc = (int(s) for s in a.shape)
    if min(H, W) < _lib.IMAGE_WINDOW:
        raise ValueError(f"image_metrics: an image of {H} x {W} has no place for the {_lib.IMAGE_WINDOW} x {_lib.IMAGE_WINDOW} window")
    if ms_ssim and min(H, W) < MS_MIN_SIDE:
        raise ValueError(f"image_metrics: MS-SSIM needs sides above {MS_MIN_SIDE - 1}, the images are {H} x {W} (ms_ssim=False skips it)")
    if n == 0:
        raise ValueError("image_metrics: no views")
    window, (C1, C2) = gaussian_window(), ssim_constants(float(data_range))
    n_levels = len(MS_WEIGHTS) if ms_ssim else 1
    with torch.cuda.device(a.device):
        rows = n + n_levels * n * Cc
        buf = torch.zeros(rows, 32, dtype=torch.uint8, device=a.device)
        error_enqueue(a, b, buf[:n])
        for i in range(n_levels):
            ssim_enqueue(a, b, window, C1, C2, buf[n + i * n * Cc:n + (i + 1) * n * Cc])
            if i + 1 < n_levels:
                a, b = pool_enqueue(a), pool_enqueue(b)
        raw = read_back(buf)
    errors = read_error_records(raw, n)
    levels = [read_ssim_records(raw, n * Cc, 32 * (n + i * n * Cc)) for i in range(n_levels)]
    return combine(errors, levels, n, (H, W, Cc), float(data_range))


def psnr(pred, gt, data_range: float = 1.0, mask=None) -> float:
    a, b = _pair(pred, gt, mask)
    n = a.shape[0]
    errors = read_error_records(read_back(error_enqueue(a, b)), n)
    return math.fsum(-10.0 * math.log10(m / data_range ** 2) if m > 0 else (math.inf if m == 0 else math.nan)
                     for m in (r.sum_sq / r.count for r in errors)) / n


def ssim(pred, gt, data_range: float = 1.0, mask=None) -> float:
    return image_metrics(pred, gt, data_range, ms_ssim=False, mask=mask).ssim


def ms_ssim(pred, gt, data_range: float = 1.0, mask=None) -> float:
    return image_metrics(pred, gt, data_range, ms_ssim=True, mask=mask).ms_ssim


@torch.no_grad()
def render_metrics(model, rays_d_cam, poses_local, rgb, depth, H: int, W: int, ray_batch_size: int = 10000, ms_ssim: bool = True,
                   noise=None, chunk: int = 8) -> RenderMetrics:
    """Renders each frame with ``inference.render_full_img``, depth-guided by the frame's own depth (as Logger.img_render_save
    does), and scores it against the captured frame: the colour with ``image_metrics``, the depth as the mean |rendered - captured|
    over the pixels with captured depth > 0 (the rendered depth is zeroed where the captured one is 0, then ``mesh_render.l1_enqueue``
    and sum_all / (both + gt_only)).  rays_d_cam [H,W,3]; poses_local [n,4,4]; rgb [n,H,W,3]; depth [n,H,W]; noise: optional
    [H*W,S] jitter table for every frame.  The frames are taken in chunks of `chunk`, so no more than a chunk's images live on the
    device; the cut does not reach a result.  SSIM is the valid-region Gaussian-window form (see the module's head); LPIPS is out
    of scope."""
    from . import inference, mesh_render
    dev = model.embed_fn.params.device
    n, H, W = len(poses_local), int(H), int(W)
    if n == 0 or len(rgb) != n or len(depth) != n:
        raise ValueError(f"render_metrics: {n} poses, {len(rgb)} colour and {len(depth)} depth frames")
    if chunk < 1:
        raise ValueError("chunk must be positive")
    if ms_ssim and min(H, W) < MS_MIN_SIDE:
        raise ValueError(f"render_metrics: MS-SSIM needs sides above {MS_MIN_SIDE - 1}, the frames are {H} x {W} (ms_ssim=False skips it)")
    parts, depth_l1 = [], []
    for k in range(0, n, chunk):
        m = min(chunk, n - k)
        pred = torch.empty(m, H, W, 3, dtype=torch.float32, device=dev)
        pred_d = torch.empty(m, H, W, dtype=torch.float32, device=dev)
        gt = torch.stack([torch.as_tensor(rgb[k + i]) for i in range(m)]).to(dev)
        gt_d = torch.stack([torch.as_tensor(depth[k + i]) for i in range(m)]).to(dev, torch.float32).reshape(m, H, W).contiguous()
        for i in range(m):
            pred[i], pred_d[i] = inference.render_full_img(model, rays_d_cam, torch.as_tensor(poses_local[k + i]), gt_d[i], H, W,
                                                           ray_batch_size=ray_batch_size, noise=noise)
        parts.append(image_metrics(pred, gt.reshape(m, H, W, 3), 1.0, ms_ssim))
        pred_d = torch.where(gt_d == 0, torch.zeros_like(pred_d), pred_d).contiguous()
        for r in mesh_render.read_l1_records(mesh_render.l1_enqueue(pred_d, gt_d)):
            seen = int(r.both) + int(r.gt_only)
            depth_l1.append(r.sum_all / seen if seen else math.nan)
    cat = lambda name: tuple(x for p in parts for x in getattr(p, name))                     # noqa: E731
    mean = lambda x: math.fsum(x) / n                                                        # noqa: E731
    per = {name: cat(name) for name in ("mse_per_view", "psnr_per_view", "l1_per_view", "ssim_per_view", "ms_ssim_per_view", "max_abs_per_view")}
    image = ImageMetrics(mean(per["mse_per_view"]), mean(per["psnr_per_view"]), mean(per["l1_per_view"]), mean(per["ssim_per_view"]),
                         mean(per["ms_ssim_per_view"]) if ms_ssim else math.nan, per["mse_per_view"], per["psnr_per_view"],
                         per["l1_per_view"], per["ssim_per_view"], per["ms_ssim_per_view"], per["max_abs_per_view"], n, (H, W, 3))
    return RenderMetrics(image, math.fsum(depth_l1) / n, tuple(depth_l1), n)
