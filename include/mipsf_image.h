/*
 * mipsf_image.h -- two stacks of images compared: the squared and absolute error behind MSE / PSNR / L1, the Gaussian-window
 * "valid" SSIM of the published NeRF-SLAM evaluations with its contrast-structure term, and the 2 x 2 mean that builds the MS-SSIM
 * pyramid.  DESIGN.md 4.20; mipsfusion_amd/image_metrics.py.
 *
 * Same conventions as mipsf_raster.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Workspaces are
 * the caller's; mipsf_image_workspace_bytes() gives their sizes.  Nothing here uses a floating-point atomic and no kernel waits
 * on another workgroup; the same call gives the same bytes.  Images are channel-last [n,H,W,C], C = 1..4, fp32 or fp64 (`dtype`);
 * an fp32 value is widened first, and every floating-point operation named below is one IEEE float64 operation rounded on its own
 * (no contraction), so a float64 restatement on the host (tests/image_cpu.py) gives the same words.
 *
 * A wave is 64 lanes, a block 256 threads = 4 waves.  "Butterfly" is v = v + (the v of lane ^ o) for o = 32, 16, 8, 4, 2, 1;
 * "waves ascending" is ((w0 + w1) + w2) + w3 (mipsfusion_amd/csrc/block_dev.h).
 */
#ifndef MIPSF_IMAGE_H
#define MIPSF_IMAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_IMAGE_F32 0u
#define MIPSF_IMAGE_F64 1u

#define MIPSF_IMAGE_WINDOW 11u                   /* taps of the SSIM window; an image has (H - 10) x (W - 10) positions        */
#define MIPSF_IMAGE_TILE_H 16u                   /* the SSIM kernel's output tile: 16 rows x 32 columns of window positions,   */
#define MIPSF_IMAGE_TILE_W 32u                   /* one block a tile; the tiles of an image are numbered row-major             */
#define MIPSF_IMAGE_MAX_CHANNELS 4u
#define MIPSF_IMAGE_MAX_SIDE 8192u               /* H and W                                                                     */
#define MIPSF_IMAGE_MAX_PLANES 65535u            /* n * C of one call                                                           */
#define MIPSF_IMAGE_MAX_VALUES 0x7fffffffu       /* n * H * W * C of one call                                                   */
#define MIPSF_IMAGE_ERROR_MAX_BLOCKS 256u        /* block partials per view of mipsf_image_error                               */

/* mipsf_image_workspace_bytes(which, n, C, H, W): bytes of a workspace; 0 = out of range */
#define MIPSF_IMAGE_WS_ERROR 1                   /* mipsf_image_error for n views of H x W x C                                  */
#define MIPSF_IMAGE_WS_SSIM 2                    /* mipsf_image_ssim for n views of H x W x C (H, W >= 11)                       */
uint64_t mipsf_image_workspace_bytes(int which, uint32_t n, uint32_t C, uint32_t H, uint32_t W);

/* Two stacks [n,H,W,C] -> one record per view over its m = H*W*C values, taken as one flat array in memory order.
 *   d = (double)a - (double)b;   sq = d*d;   ab = |d|
 *   sum_sq, sum_abs: B = min(ceil(m / 256), MIPSF_IMAGE_ERROR_MAX_BLOCKS) blocks a view.  Thread t of block k starts from 0.0 and
 *       adds the terms of the values (k*256 + t) + j*(B*256), j = 0, 1, .. in ascending j; butterfly over each wave; waves
 *       ascending: the block's partial.  One finishing wave per view: lane l starts from 0.0 and adds the partials l, l + 64, ..
 *       in ascending order; butterfly.
 *   max_abs: along the same path with max(x, y) = (y > x ? y : x) from 0.0: the largest |d| that is not NaN
 *   count   = m
 * A NaN in either image reaches sum_sq and sum_abs as NaN: nothing is masked.
 * Refused on the host, with nothing launched: n, C or H*W zero, C above MIPSF_IMAGE_MAX_CHANNELS, H or W above
 * MIPSF_IMAGE_MAX_SIDE, n*C above MIPSF_IMAGE_MAX_PLANES, n*H*W*C above MIPSF_IMAGE_MAX_VALUES, a dtype that is neither of the
 * two, a null pointer, a workspace that is not 16-byte aligned. */
typedef struct mipsf_image_error_record {
    double sum_sq, sum_abs, max_abs;
    uint64_t count;
} mipsf_image_error_record;

typedef struct mipsf_image_error_args {
    uint32_t struct_size;
    uint32_t n, H, W, C;
    uint32_t dtype;                     /* MIPSF_IMAGE_F32 or MIPSF_IMAGE_F64, of both a and b                              */
    const void* a;                      /* [n,H,W,C]                                                                       */
    const void* b;                      /* [n,H,W,C]                                                                       */
    mipsf_image_error_record* records;  /* [n]                                                                             */
    void* workspace;                    /* MIPSF_IMAGE_WS_ERROR bytes for (n, C, H, W), 16-byte aligned                      */
} mipsf_image_error_args;

int mipsf_image_error(const mipsf_image_error_args* a, void* stream);

/* SSIM with a separable 11-tap window w over the "valid" region: position (r, c), 0 <= r < H - 10, 0 <= c < W - 10, of one
 * channel of one view covers the pixels [r, r + 10] x [c, c + 10].  With x = (double)a, y = (double)b of a pixel, for each of the
 * five planes q in { x, y, x*x, y*y, x*y } (each product rounded first):
 *   along H:   g[r][c] = w[0]*q[r][c];      then  g[r][c] = g[r][c] + w[k]*q[r+k][c]   for k = 1 .. 10, ascending
 *   along W:   f[r][c] = w[0]*g[r][c];      then  f[r][c] = f[r][c] + w[k]*g[r][c+k]   for k = 1 .. 10, ascending
 * (a multiplication and an addition, never fused).  Then with m1 = f(x), m2 = f(y):
 *   m11 = m1*m1;  m22 = m2*m2;  m12 = m1*m2
 *   s1 = f(x*x) - m11;  s2 = f(y*y) - m22;  s12 = f(x*y) - m12
 *   cs   = (2*s12 + C2) / ((s1 + s2) + C2)
 *   ssim = ((2*m12 + C1) / ((m11 + m22) + C1)) * cs
 * Two identical images give the same words in numerator and denominator (2*s == s + s), so ssim == cs == 1.0 at every
 * position; swapping a and b changes no word.  A NaN in a window reaches that position's values, and the sums, as NaN.
 * One record per (view, channel), records[view*C + channel], both maps summed in this order: the positions are cut into tiles of
 * MIPSF_IMAGE_TILE_H x MIPSF_IMAGE_TILE_W, numbered row-major, ceil((W-10)/32) a row.  Thread t of a tile's block owns the
 * positions (row t/32, column t%32) and (row t/32 + 8, column t%32) of the tile; its value is v0 + v1 in that order, where a
 * position outside the image's valid region counts as 0.0.  Butterfly over each wave; waves ascending: the tile's partial.  One
 * finishing wave per (view, channel): lane l starts from 0.0 and adds the partials of the tiles l, l + 64, .. in ascending
 * order; butterfly.
 *   count = (H - 10) * (W - 10)
 * Refused on the host, with nothing launched: what mipsf_image_error refuses, and H or W below MIPSF_IMAGE_WINDOW. */
typedef struct mipsf_image_ssim_record {
    double sum_ssim, sum_cs;
    uint64_t count;
    uint64_t reserved;
} mipsf_image_ssim_record;

typedef struct mipsf_image_ssim_args {
    uint32_t struct_size;
    uint32_t n, H, W, C;
    uint32_t dtype;                     /* of both a and b                                                                 */
    double window[11];                  /* w[0..10]                                                                        */
    double C1, C2;
    const void* a;                      /* [n,H,W,C]                                                                       */
    const void* b;                      /* [n,H,W,C]                                                                       */
    mipsf_image_ssim_record* records;   /* [n*C]                                                                           */
    void* workspace;                    /* MIPSF_IMAGE_WS_SSIM bytes for (n, C, H, W), 16-byte aligned                       */
} mipsf_image_ssim_args;

int mipsf_image_ssim(const mipsf_image_ssim_args* a, void* stream);

/* The 2 x 2 mean of the MS-SSIM pyramid: avg_pool2d(kernel 2, stride 2, padding = side % 2, padding counted).  A side of odd
 * length is zero-padded by one pixel on BOTH ends: p = side % 2, out = (side + 2*p - 2)/2 + 1 in integer division.  Output pixel
 * (i, j) covers the padded rows 2i, 2i + 1 and columns 2j, 2j + 1 (padded index - p is the image's); a last padded row or column
 * without a partner is dropped.  With x00, x01 the two of row 2i and x10, x11 those of row 2i + 1, padding as 0.0:
 *   out = ((x00 + x01) + (x10 + x11)) * 0.25
 * Refused on the host, with nothing launched: what mipsf_image_error refuses (there is no workspace). */
typedef struct mipsf_image_pool2_args {
    uint32_t struct_size;
    uint32_t n, H, W, C;
    uint32_t dtype;                     /* of `in`                                                                         */
    const void* in;                     /* [n,H,W,C]                                                                       */
    double* out;                        /* [n,Ho,Wo,C] fp64                                                                */
} mipsf_image_pool2_args;

int mipsf_image_pool2(const mipsf_image_pool2_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_IMAGE_H */
