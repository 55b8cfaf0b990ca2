// The per-pixel arithmetic of include/mipsf_image.h, stated once for the device (image.hip) and for the host build that checks it
// without a GPU (tools/image_host.hip).  Every line is one float64 operation of the header's rule; both builds compile with
// -ffp-contract=off, so none is fused.
#pragma once
#include <stdint.h>

#include "../../include/mipsf_image.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MIPSF_IMAGE_HD __host__ __device__ __forceinline__
#else
#define MIPSF_IMAGE_HD inline
#endif

namespace mipsf {
namespace image {

constexpr int TAPS = MIPSF_IMAGE_WINDOW;
constexpr int HALO = TAPS - 1;
constexpr int TILE_H = MIPSF_IMAGE_TILE_H, TILE_W = MIPSF_IMAGE_TILE_W;
constexpr int IN_H = TILE_H + HALO, IN_W = TILE_W + HALO;      // a tile with its halo: 26 x 42 pixels

struct Window {
    double w[TAPS];
};

// the five planes of one pixel pair, each product rounded on its own
struct Planes {
    double q[5];
};
MIPSF_IMAGE_HD Planes planes_of(double x, double y) { return Planes{{x, y, x * x, y * y, x * y}}; }

// one tap of a pass: the first starts the sum, the others add to it
MIPSF_IMAGE_HD double tap_first(double w0, double q) { return w0 * q; }
MIPSF_IMAGE_HD double tap_next(double acc, double wk, double q) {
    const double p = wk * q;
    return acc + p;
}

// the 11 taps over q[0], q[stride], .. q[10*stride]
MIPSF_IMAGE_HD double filter11(const Window& win, const double* q, int stride) {
    double acc = tap_first(win.w[0], q[0]);
#pragma unroll
    for (int k = 1; k < TAPS; ++k) acc = tap_next(acc, win.w[k], q[k * stride]);
    return acc;
}

// the first pass at one pixel column: the five planes of (x[k*stride], y[k*stride]), k = 0..10, filtered along H
MIPSF_IMAGE_HD void pass_h(const Window& win, const double* x, const double* y, int stride, double* g) {
    const Planes p0 = planes_of(x[0], y[0]);
#pragma unroll
    for (int q = 0; q < 5; ++q) g[q] = tap_first(win.w[0], p0.q[q]);
#pragma unroll
    for (int k = 1; k < TAPS; ++k) {
        const Planes p = planes_of(x[k * stride], y[k * stride]);
#pragma unroll
        for (int q = 0; q < 5; ++q) g[q] = tap_next(g[q], win.w[k], p.q[q]);
    }
}

// f[0..4] = the filtered planes x, y, x*x, y*y, x*y at one position
MIPSF_IMAGE_HD void ssim_cs(const double* f, double C1, double C2, double& ssim, double& cs) {
    const double m1 = f[0], m2 = f[1];
    const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
    const double s1 = f[2] - m11, s2 = f[3] - m22, s12 = f[4] - m12;
    cs = (2.0 * s12 + C2) / ((s1 + s2) + C2);
    ssim = ((2.0 * m12 + C1) / ((m11 + m22) + C1)) * cs;
}

MIPSF_IMAGE_HD double pool4(double x00, double x01, double x10, double x11) { return ((x00 + x01) + (x10 + x11)) * 0.25; }
MIPSF_IMAGE_HD uint32_t pool_pad(uint32_t side) { return side % 2u; }
MIPSF_IMAGE_HD uint32_t pool_out(uint32_t side) { return (side + 2u * pool_pad(side) - 2u) / 2u + 1u; }

// one output pixel of the pool; px(row, col) gives an image pixel of this view and channel as double
template <class Px>
MIPSF_IMAGE_HD double pool_pixel(uint32_t H, uint32_t W, uint32_t i, uint32_t j, Px px) {
    const int64_t r0 = (int64_t)2 * i - pool_pad(H), c0 = (int64_t)2 * j - pool_pad(W);
    double x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t r = r0 + (k >> 1), c = c0 + (k & 1);
        x[k] = (r >= 0 && r < (int64_t)H && c >= 0 && c < (int64_t)W) ? px((uint32_t)r, (uint32_t)c) : 0.0;
    }
    return pool4(x[0], x[1], x[2], x[3]);
}

MIPSF_IMAGE_HD double max_keep(double x, double y) { return y > x ? y : x; }

MIPSF_IMAGE_HD uint32_t tiles_x(uint32_t W) { return (W - HALO + TILE_W - 1) / TILE_W; }
MIPSF_IMAGE_HD uint32_t tiles_y(uint32_t H) { return (H - HALO + TILE_H - 1) / TILE_H; }

}  // namespace image
}  // namespace mipsf
