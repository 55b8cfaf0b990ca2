// Two stacks of images compared (include/mipsf_image.h): the error sums behind MSE / PSNR / L1, the Gaussian-window valid-region
// SSIM with its contrast-structure term, and the 2 x 2 mean of the MS-SSIM pyramid.  Upstream has no such code; the formulas are
// the published ones.  DESIGN.md 4.20.
//
// Shape of the SSIM kernel: one block takes a 16 x 32 tile of window positions of one (view, channel).  It stages the tile with
// its 10-pixel halo, 26 x 42 pixels of both images, in LDS as float64; the first pass filters the five planes along H into five
// 16 x 42 LDS planes; the second filters along W into registers, two positions a thread.  Consecutive lanes read consecutive
// doubles of a row in both passes: 32 lanes x 8 bytes cover the 64 four-byte banks once.  44 352 + 32 bytes of static LDS.
// The per-pixel arithmetic is image_dev.h's, which tools/image_host.hip compiles for the host.
#include "block_dev.h"
#include "image_dev.h"

namespace mipsf {
namespace {

using namespace image;

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
static_assert(TPB / TILE_W * 2 == TILE_H, "a thread owns two positions of a tile, 8 rows apart");
static_assert(sizeof(mipsf_image_error_record) == 32 && sizeof(mipsf_image_ssim_record) == 32, "image records");
static_assert(sizeof(mipsf_image_error_args) == 56 && sizeof(mipsf_image_ssim_args) == 160 && sizeof(mipsf_image_pool2_args) == 40, "image argument blocks");
static_assert(sizeof(double) * (2 * IN_H * IN_W + 5 * TILE_H * IN_W + WAVES) <= 64 * 1024, "static LDS");

struct MaxKeep {
    __device__ __forceinline__ double operator()(double x, double y) const { return max_keep(x, y); }
};

bool in_range(uint32_t n, uint32_t C, uint32_t H, uint32_t W) {
    return n >= 1 && C >= 1 && C <= MIPSF_IMAGE_MAX_CHANNELS && H >= 1 && W >= 1 && H <= MIPSF_IMAGE_MAX_SIDE && W <= MIPSF_IMAGE_MAX_SIDE &&
           (uint64_t)n * C <= MIPSF_IMAGE_MAX_PLANES && (uint64_t)n * H * W * C <= MIPSF_IMAGE_MAX_VALUES;
}

// ------------------------------------------------------------------------------------------------ error sums
struct ErrorPartial {
    double sum_sq, sum_abs, max_abs, pad;
};
static_assert(sizeof(ErrorPartial) == 32, "error partial");

inline uint32_t error_blocks(uint64_t m) { return min(blocks_for(m, TPB), MIPSF_IMAGE_ERROR_MAX_BLOCKS); }

// block (k, view), thread t takes the values (k*TPB + t) + j * (blocks*TPB) of the view; butterfly over the wave; waves ascending
template <class T>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) image_error_partial_kernel(const T* __restrict__ a, const T* __restrict__ b, uint32_t m,
                                                                                    ErrorPartial* __restrict__ part) {
    __shared__ double sm[WAVES];
    const size_t off = (size_t)blockIdx.y * m;
    double sq = 0.0, ab = 0.0, mx = 0.0;
    const uint32_t stride = gridDim.x * TPB;
    for (uint64_t p = blockIdx.x * TPB + threadIdx.x; p < m; p += stride) {
        const double d = (double)a[off + p] - (double)b[off + p];
        const double dd = d * d, da = fabs(d);
        sq = sq + dd;
        ab = ab + da;
        mx = max_keep(mx, da);
    }
    sq = block_reduce<WAVES>(sq, sm, Add());
    ab = block_reduce<WAVES>(ab, sm, Add());
    mx = block_reduce<WAVES>(mx, sm, MaxKeep());
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ErrorPartial{sq, ab, mx, 0.0};
}

// one wave per view: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) image_error_finish_kernel(const ErrorPartial* __restrict__ part, uint32_t nb,
                                                                                          uint64_t m, mipsf_image_error_record* __restrict__ rec) {
    double sq = 0.0, ab = 0.0, mx = 0.0;
    for (uint32_t k = threadIdx.x; k < nb; k += MIPSF_WAVE) {
        const ErrorPartial p = part[(size_t)blockIdx.x * nb + k];
        sq = sq + p.sum_sq;
        ab = ab + p.sum_abs;
        mx = max_keep(mx, p.max_abs);
    }
    sq = wave_reduce(sq, Add()), ab = wave_reduce(ab, Add()), mx = wave_reduce(mx, MaxKeep());
    if (threadIdx.x == 0) rec[blockIdx.x] = mipsf_image_error_record{sq, ab, mx, m};
}

// ------------------------------------------------------------------------------------------------ SSIM
// block (tile, view*C + channel); part[(plane * tiles + tile) * 2 + {0: ssim, 1: cs}]
template <class T>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) image_ssim_tile_kernel(const T* __restrict__ a, const T* __restrict__ b, uint32_t H,
                                                                                uint32_t W, uint32_t C, Window win, double C1, double C2,
                                                                                double* __restrict__ part) {
    __shared__ double X[IN_H][IN_W], Y[IN_H][IN_W], G[5][TILE_H][IN_W], sm[WAVES];
    const uint32_t ntx = tiles_x(W);
    const uint32_t r0 = blockIdx.x / ntx * TILE_H, c0 = blockIdx.x % ntx * TILE_W;
    const uint32_t view = blockIdx.y / C, ch = blockIdx.y % C;
    const size_t base = (size_t)view * H * W * C + ch;

    // the tile and its halo; a pixel outside the image is 0.0 and only reaches positions outside the valid region
    for (int idx = threadIdx.x; idx < IN_H * IN_W; idx += TPB) {
        const int r = idx / IN_W, c = idx % IN_W;
        const uint32_t gr = r0 + r, gc = c0 + c;
        const bool inside = gr < H && gc < W;
        const size_t off = inside ? base + ((size_t)gr * W + gc) * C : base;
        const T x = a[off], y = b[off];
        X[r][c] = inside ? (double)x : 0.0;
        Y[r][c] = inside ? (double)y : 0.0;
    }
    __syncthreads();
    // along H
    for (int idx = threadIdx.x; idx < TILE_H * IN_W; idx += TPB) {
        const int r = idx / IN_W, c = idx % IN_W;
        double g[5];
        pass_h(win, &X[r][c], &Y[r][c], IN_W, g);
#pragma unroll
        for (int q = 0; q < 5; ++q) G[q][r][c] = g[q];
    }
    __syncthreads();
    // along W, the maps, the thread's two positions in ascending order
    double v_ssim[2], v_cs[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = threadIdx.x / TILE_W + h * (TILE_H / 2), c = threadIdx.x % TILE_W;
        double f[5], s, k;
#pragma unroll
        for (int q = 0; q < 5; ++q) f[q] = filter11(win, &G[q][r][c], 1);
        ssim_cs(f, C1, C2, s, k);
        const bool valid = r0 + r < H - HALO && c0 + c < W - HALO;
        v_ssim[h] = valid ? s : 0.0;
        v_cs[h] = valid ? k : 0.0;
    }
    const double t_ssim = block_reduce<WAVES>(v_ssim[0] + v_ssim[1], sm, Add());
    const double t_cs = block_reduce<WAVES>(v_cs[0] + v_cs[1], sm, Add());
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = t_ssim, p[1] = t_cs;
    }
}

// one wave per (view, channel): lane l adds the tiles l, l + 64, ... in ascending order, then the butterfly
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) image_ssim_finish_kernel(const double* __restrict__ part, uint32_t tiles,
                                                                                         uint64_t count, mipsf_image_ssim_record* __restrict__ rec) {
    double s = 0.0, k = 0.0;
    for (uint32_t t = threadIdx.x; t < tiles; t += MIPSF_WAVE) {
        const double* p = part + ((size_t)blockIdx.x * tiles + t) * 2;
        s = s + p[0];
        k = k + p[1];
    }
    s = wave_reduce(s, Add()), k = wave_reduce(k, Add());
    if (threadIdx.x == 0) rec[blockIdx.x] = mipsf_image_ssim_record{s, k, count, 0};
}

// ------------------------------------------------------------------------------------------------ the pyramid's 2 x 2 mean
// one thread per output value [n,Ho,Wo,C]
template <class T>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) image_pool2_kernel(const T* __restrict__ in, uint32_t H, uint32_t W, uint32_t C,
                                                                            uint64_t total, double* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= total) return;
    const uint32_t Ho = pool_out(H), Wo = pool_out(W);
    const uint32_t ch = (uint32_t)(e % C), j = (uint32_t)(e / C % Wo), i = (uint32_t)(e / C / Wo % Ho), view = (uint32_t)(e / C / Wo / Ho);
    const T* img = in + (size_t)view * H * W * C + ch;
    out[e] = pool_pixel(H, W, i, j, [&](uint32_t r, uint32_t c) { return (double)img[((size_t)r * W + c) * C]; });
}

inline bool dtype_ok(uint32_t d) { return d == MIPSF_IMAGE_F32 || d == MIPSF_IMAGE_F64; }

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_image_workspace_bytes(int which, uint32_t n, uint32_t C, uint32_t H, uint32_t W) {
    if (!in_range(n, C, H, W)) return 0;
    switch (which) {
        case MIPSF_IMAGE_WS_ERROR:
            return (uint64_t)n * error_blocks((uint64_t)H * W * C) * sizeof(ErrorPartial);
        case MIPSF_IMAGE_WS_SSIM:
            if (H < MIPSF_IMAGE_WINDOW || W < MIPSF_IMAGE_WINDOW) return 0;
            return (uint64_t)n * C * tiles_x(W) * tiles_y(H) * 2 * sizeof(double);
    }
    return 0;
}

#define MIPSF_IMAGE_COMMON(a, name)                                                                                                     \
    MIPSF_REQUIRE((a)->n > 0 && (a)->C > 0, name ": %u views of %u channels: there must be at least one of each", (a)->n, (a)->C);      \
    MIPSF_REQUIRE((a)->H > 0 && (a)->W > 0, name ": an image of %u x %u has no pixels", (a)->H, (a)->W);                                \
    MIPSF_REQUIRE(in_range((a)->n, (a)->C, (a)->H, (a)->W),                                                                             \
                  name ": %u views of %u x %u x %u: at most %u channels, %u a side, %u (view, channel) planes and %u values a call",    \
                  (a)->n, (a)->H, (a)->W, (a)->C, MIPSF_IMAGE_MAX_CHANNELS, MIPSF_IMAGE_MAX_SIDE, MIPSF_IMAGE_MAX_PLANES,               \
                  MIPSF_IMAGE_MAX_VALUES);                                                                                              \
    MIPSF_REQUIRE(dtype_ok((a)->dtype), name ": dtype %u is neither MIPSF_IMAGE_F32 nor MIPSF_IMAGE_F64", (a)->dtype)

extern "C" int mipsf_image_error(const mipsf_image_error_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_image_error_args, "mipsf_image_error");
    MIPSF_IMAGE_COMMON(a, "mipsf_image_error");
    MIPSF_REQUIRE(a->a && a->b && a->records && a->workspace, "mipsf_image_error: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_image_error: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t m = a->H * a->W * a->C, nb = error_blocks(m);
    ErrorPartial* part = (ErrorPartial*)a->workspace;
    if (a->dtype == MIPSF_IMAGE_F32)
        hipLaunchKernelGGL(image_error_partial_kernel<float>, dim3(nb, a->n), dim3(TPB), 0, st, (const float*)a->a, (const float*)a->b, m, part);
    else
        hipLaunchKernelGGL(image_error_partial_kernel<double>, dim3(nb, a->n), dim3(TPB), 0, st, (const double*)a->a, (const double*)a->b, m, part);
    hipLaunchKernelGGL(image_error_finish_kernel, dim3(a->n), dim3(MIPSF_WAVE), 0, st, (const ErrorPartial*)part, nb, (uint64_t)m, a->records);
    return check_launch("image_error");
}

extern "C" int mipsf_image_ssim(const mipsf_image_ssim_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_image_ssim_args, "mipsf_image_ssim");
    MIPSF_IMAGE_COMMON(a, "mipsf_image_ssim");
    MIPSF_REQUIRE(a->H >= MIPSF_IMAGE_WINDOW && a->W >= MIPSF_IMAGE_WINDOW, "mipsf_image_ssim: an image of %u x %u has no place for a window of %u x %u",
                  a->H, a->W, MIPSF_IMAGE_WINDOW, MIPSF_IMAGE_WINDOW);
    MIPSF_REQUIRE(a->a && a->b && a->records && a->workspace, "mipsf_image_ssim: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_image_ssim: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t tiles = tiles_x(a->W) * tiles_y(a->H), planes = a->n * a->C;
    Window win;
    for (int k = 0; k < TAPS; ++k) win.w[k] = a->window[k];
    double* part = (double*)a->workspace;
    if (a->dtype == MIPSF_IMAGE_F32)
        hipLaunchKernelGGL(image_ssim_tile_kernel<float>, dim3(tiles, planes), dim3(TPB), 0, st, (const float*)a->a, (const float*)a->b, a->H, a->W,
                           a->C, win, a->C1, a->C2, part);
    else
        hipLaunchKernelGGL(image_ssim_tile_kernel<double>, dim3(tiles, planes), dim3(TPB), 0, st, (const double*)a->a, (const double*)a->b, a->H,
                           a->W, a->C, win, a->C1, a->C2, part);
    hipLaunchKernelGGL(image_ssim_finish_kernel, dim3(planes), dim3(MIPSF_WAVE), 0, st, (const double*)part, tiles,
                       (uint64_t)(a->H - HALO) * (a->W - HALO), a->records);
    return check_launch("image_ssim");
}

extern "C" int mipsf_image_pool2(const mipsf_image_pool2_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_image_pool2_args, "mipsf_image_pool2");
    MIPSF_IMAGE_COMMON(a, "mipsf_image_pool2");
    MIPSF_REQUIRE(a->in && a->out, "mipsf_image_pool2: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t total = (uint64_t)a->n * pool_out(a->H) * pool_out(a->W) * a->C;
    if (a->dtype == MIPSF_IMAGE_F32)
        hipLaunchKernelGGL(image_pool2_kernel<float>, dim3(blocks_for(total, TPB)), dim3(TPB), 0, st, (const float*)a->in, a->H, a->W, a->C, total,
                           a->out);
    else
        hipLaunchKernelGGL(image_pool2_kernel<double>, dim3(blocks_for(total, TPB)), dim3(TPB), 0, st, (const double*)a->in, a->H, a->W, a->C, total,
                           a->out);
    return check_launch("image_pool2");
}
