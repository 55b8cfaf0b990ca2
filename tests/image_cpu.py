"""numpy float64 restatement of include/mipsf_image.h: the window, the two filter passes, the ssim / cs maps, the 2 x 2 mean, the
pyramid, and every sum in the device's order (lane, wave butterfly, waves ascending, block or tile partials, one finishing wave).
numpy's element-wise operations round one at a time and never fuse, so the words are those of the kernels.  Also the cases the
tests of the image metrics share (tests/test_image_cpu.py, tests/test_gpu_image.py).
"""
import functools
import math

import numpy as np

TAPS, TILE_H, TILE_W, TPB, WAVE, ERROR_MAX_BLOCKS = 11, 16, 32, 256, 64, 256
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_window():
    g = [math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], np.float64)


def constants(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def as_stack(x):
    """-> float64 [n,H,W,C]; uint8 is divided by 255 in float64; float32 widens exactly"""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None, :, :, None]
    elif x.ndim == 3:
        x = x[None]
    return x.astype(np.float64) / 255.0 if x.dtype == np.uint8 else x.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the sums' order
def butterfly(v, op=np.add):
    """v [..., 64] -> the value every lane holds after v = op(v, v[lane ^ o]) for o = 32 .. 1"""
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lane ^ o])
    return v[..., 0]


def max_keep(x, y):
    return np.where(y > x, y, x)


def block_reduce(v, op=np.add):
    """v [..., 256] thread values -> the block's value: butterfly over each wave, waves ascending"""
    w = butterfly(v.reshape(v.shape[:-1] + (TPB // WAVE, WAVE)), op)
    r = w[..., 0]
    for k in range(1, TPB // WAVE):
        r = op(r, w[..., k])
    return r


def finish(p, op=np.add):
    """p [..., m] partials -> one finishing wave: lane l starts from 0.0 and takes l, l + 64, .. ascending; butterfly"""
    m = p.shape[-1]
    rounds = -(-m // WAVE)
    q = np.zeros(p.shape[:-1] + (rounds * WAVE,), np.float64)
    q[..., :m] = p
    q = q.reshape(p.shape[:-1] + (rounds, WAVE))
    s = np.zeros(p.shape[:-1] + (WAVE,), np.float64)
    for j in range(rounds):                                  # a lane past the last partial adds nothing: + 0.0 changes no word
        s = op(s, q[..., j, :])
    return butterfly(s, op)


# ------------------------------------------------------------------------------------------------------------ error sums
def error_records(a, b):
    """-> per view dict(sum_sq, sum_abs, max_abs, count) in the order of mipsf_image_error"""
    a, b = as_stack(a), as_stack(b)
    out = []
    for x, y in zip(a, b):
        d = x.reshape(-1) - y.reshape(-1)
        m = d.size
        nb = min(-(-m // TPB), ERROR_MAX_BLOCKS)
        stride = nb * TPB
        rounds = -(-m // stride)
        rec = {"count": m}
        for name, term, op in (("sum_sq", d * d, np.add), ("sum_abs", np.abs(d), np.add), ("max_abs", np.abs(d), max_keep)):
            q = np.zeros(rounds * stride, np.float64)
            q[:m] = term
            q = q.reshape(rounds, nb, TPB)
            s = np.zeros((nb, TPB), np.float64)
            for j in range(rounds):
                s = op(s, q[j])
            rec[name] = float(finish(block_reduce(s, op), op))
        out.append(rec)
    return out


# ------------------------------------------------------------------------------------------------------------ SSIM
def _filter(q, w, axis):
    n = q.shape[axis] - (TAPS - 1)
    take = lambda k: np.take(q, np.arange(k, k + n), axis=axis)          # noqa: E731
    acc = w[0] * take(0)
    for k in range(1, TAPS):
        acc = acc + w[k] * take(k)
    return acc


def ssim_maps(a, b, window, C1, C2):
    """a, b [n,H,W,C] -> (ssim, cs) maps float64 [n,C,H-10,W-10]"""
    x, y = (np.moveaxis(as_stack(v), 3, 1) for v in (a, b))
    f = [_filter(_filter(q, window, 2), window, 3) for q in (x, y, x * x, y * y, x * y)]
    m1, m2 = f[0], f[1]
    m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
    s1, s2, s12 = f[2] - m11, f[3] - m22, f[4] - m12
    with np.errstate(divide="ignore", invalid="ignore"):
        cs = (2.0 * s12 + C2) / ((s1 + s2) + C2)
        ssim = ((2.0 * m12 + C1) / ((m11 + m22) + C1)) * cs
    return ssim, cs


def map_sum(m):
    """m [n,C,Ho,Wo] -> [n,C]: the sum of a map in the order of mipsf_image_ssim"""
    n, C, Ho, Wo = m.shape
    ty, tx = -(-Ho // TILE_H), -(-Wo // TILE_W)
    p = np.zeros((n, C, ty * TILE_H, tx * TILE_W), np.float64)
    p[:, :, :Ho, :Wo] = m
    t = p.reshape(n, C, ty, TILE_H, tx, TILE_W).transpose(0, 1, 2, 4, 3, 5)         # [n,C,ty,tx,16,32]
    lanes = (t[..., :TILE_H // 2, :] + t[..., TILE_H // 2:, :]).reshape(n, C, ty * tx, TPB)
    return finish(block_reduce(lanes))


def ssim_records(a, b, window, C1, C2):
    """-> per (view, channel), view-major, dict(sum_ssim, sum_cs, count)"""
    ssim, cs = ssim_maps(a, b, window, C1, C2)
    s, k = map_sum(ssim), map_sum(cs)
    count = ssim.shape[2] * ssim.shape[3]
    return [{"sum_ssim": float(s[v, c]), "sum_cs": float(k[v, c]), "count": count} for v in range(s.shape[0]) for c in range(s.shape[1])]


# ------------------------------------------------------------------------------------------------------------ the pyramid
def pool_out(side):
    return (side + 2 * (side % 2) - 2) // 2 + 1


def pool2(x):
    """[n,H,W,C] -> float64 [n,Ho,Wo,C]"""
    x = as_stack(x)
    n, H, W, C = x.shape
    ph, pw = H % 2, W % 2
    Ho, Wo = pool_out(H), pool_out(W)
    p = np.pad(x, ((0, 0), (ph, ph), (pw, pw), (0, 0)))[:, :2 * Ho, :2 * Wo]
    return ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])) * 0.25


def metrics(pred, gt, data_range=1.0, ms_ssim=True, mask=None):
    """the fields of mipsfusion_amd.image_metrics.ImageMetrics as a dict, from the restated records"""
    a, b = as_stack(pred), as_stack(gt)
    if mask is not None:
        m = np.asarray(mask, np.float64)
        m = (m[None] if m.ndim == 2 else m)[..., None]
        a, b = a * m, b * m
    n, H, W, C = a.shape
    window, (C1, C2) = gaussian_window(), constants(float(data_range))
    errors = error_records(a, b)
    levels = []
    for i in range(len(MS_WEIGHTS) if ms_ssim else 1):
        levels.append(ssim_records(a, b, window, C1, C2))
        if ms_ssim and i + 1 < len(MS_WEIGHTS):
            a, b = pool2(a), pool2(b)
    mse = tuple(r["sum_sq"] / r["count"] for r in errors)
    l1 = tuple(r["sum_abs"] / r["count"] for r in errors)
    psnr = tuple(-10.0 * math.log10(v / data_range ** 2) if v > 0 else (math.inf if v == 0 else math.nan) for v in mse)
    ssim_v, ms_v = [], []
    for v in range(n):
        s = 0.0
        for c in range(C):
            r = levels[0][v * C + c]
            s += r["sum_ssim"] / r["count"]
        ssim_v.append(s / C)
        if ms_ssim:
            s = 0.0
            for c in range(C):
                prod = 1.0
                for i, w in enumerate(MS_WEIGHTS):
                    r = levels[i][v * C + c]
                    val = (r["sum_cs"] if i < 4 else r["sum_ssim"]) / r["count"]
                    prod = prod * (max(val, 0.0) ** w)
                s += prod
            ms_v.append(s / C)
    mean = lambda x: math.fsum(x) / n                                    # noqa: E731
    return {"mse": mean(mse), "psnr": mean(psnr), "l1": mean(l1), "ssim": mean(ssim_v), "ms_ssim": mean(ms_v) if ms_v else math.nan,
            "mse_per_view": mse, "psnr_per_view": psnr, "l1_per_view": l1, "ssim_per_view": tuple(ssim_v), "ms_ssim_per_view": tuple(ms_v),
            "max_abs_per_view": tuple(r["max_abs"] for r in errors), "n_views": n, "shape": (H, W, C), "errors": errors, "levels": levels}


# ------------------------------------------------------------------------------------------------------------ shared cases
# T is the output tile's size in that direction: (T+9) x (T+10) has one position less than a tile, exactly a tile; (T+11) x
# (2T+10) one more, exactly two
SSIM_SHAPES = {
    "11x11x1": (1, 11, 11, 1), "11x75x3": (1, 11, 75, 3), "12x29x3": (1, 12, 29, 3),
    "25x42x3": (1, TILE_H + 9, TILE_W + 10, 3), "27x74x1": (1, TILE_H + 11, 2 * TILE_W + 10, 1),
    "43x37x3n3": (3, 43, 37, 3), "20x33x4": (2, 20, 33, 4), "35x60x2": (1, 35, 60, 2),
}
PLANTED = ("identical", "swapped", "inverted", "constant", "outside", "range255", "uint8")


@functools.lru_cache(maxsize=None)
def images(name, dtype="float32"):
    """the seeded image pair of a shape case: uniform noise and a disturbed copy, read-only"""
    n, H, W, C = SSIM_SHAPES[name]
    g = np.random.default_rng(sorted(SSIM_SHAPES).index(name) + 11)
    a = g.uniform(0, 1, (n, H, W, C))
    b = np.clip(a + g.normal(0, 0.1, a.shape), 0, 1)
    a, b = a.astype(dtype), b.astype(dtype)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def planted(kind, dtype="float32"):
    """-> (a, b, data_range) at 43 x 37 x 3, n = 2"""
    g = np.random.default_rng(PLANTED.index(kind) + 101)
    a = g.uniform(0, 1, (2, 43, 37, 3))
    b = np.clip(a + g.normal(0, 0.15, a.shape), 0, 1)
    rng = 1.0
    if kind == "identical":
        b = a
    elif kind == "inverted":
        b = 1.0 - a.astype(dtype).astype(np.float64)
    elif kind == "constant":
        a = np.full_like(a, 0.37)
        b = a
    elif kind == "outside":
        a, b = a * 1.7 - 0.3, b * 1.7 - 0.3
    elif kind == "range255":
        a, b, rng = a * 255.0, b * 255.0, 255.0
    if kind == "uint8":
        a, b = (a * 255).astype(np.uint8), (b * 255).astype(np.uint8)
    else:
        a, b = a.astype(dtype), b.astype(dtype)
    a.setflags(write=False), b.setflags(write=False)
    return a, b, rng


@functools.lru_cache(maxsize=None)
def reference_records(name, dtype="float32"):
    a, b = images(name, dtype)
    return ssim_records(a, b, gaussian_window(), *constants(1.0)), error_records(a, b)


METRIC_CASES = {"161x163x3n2": (2, 161, 163, 3), "176x162x1": (1, 176, 162, 1)}


@functools.lru_cache(maxsize=None)
def metric_images(name):
    """uniform noise over a ramp and a noisy copy: MS-SSIM well inside (0, 1), and the variance of every window large beside
    C2 = 9e-4, so that the maps are well conditioned (the variance stands in the denominator of cs; on smooth images the
    rounding of the 121 products, 1e-16 each, is amplified a thousandfold and the comparison with conv2d measures that)"""
    n, H, W, C = METRIC_CASES[name]
    g = np.random.default_rng(sorted(METRIC_CASES).index(name) + 5)
    a = 0.8 * g.uniform(0, 1, (n, H, W, C)) + 0.2 * np.linspace(0, 1, W)[None, None, :, None]
    b = np.clip(a + g.normal(0, 0.1, a.shape), 0, 1)
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def reference_metrics(name):
    return metrics(*metric_images(name))
