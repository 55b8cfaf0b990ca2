/*
 * mipsf_tsdf.h -- depth frames fused into a dense truncated signed distance volume (running mean per voxel), and the colour of
 * marched vertices from the fused colour volume.  The step between depth images and a volume that mcubes.hip can march: the
 * rendered-depth meshing protocol, the classical baseline, a stand-in ground truth.  DESIGN.md 4.19; mipsfusion_amd/tsdf.py.
 *
 * Same conventions as mipsf_raster.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Nothing here uses
 * a floating-point atomic (the two counts are integer sums); a voxel is owned by one lane for the whole call; the same call gives
 * the same bytes.  Every floating-point operation named below is one IEEE float64 operation rounded on its own (no contraction,
 * no reciprocal), fp32 inputs widened first, so a float64 restatement on the host (tests/tsdf_cpu.py) gives the same words.
 */
#ifndef MIPSF_TSDF_H
#define MIPSF_TSDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_TSDF_MAX_VOXELS 0x7fffffffu        /* X * Y * Z of a volume: below 2^31                                          */
#define MIPSF_TSDF_MAX_SIDE 8192u                /* H and W of an image                                                         */
#define MIPSF_TSDF_VIEW_CHUNK 256u               /* capacity of a workgroup's list of surviving views: the views of a call are   */
                                                 /* taken in chunks of this many inside the kernel, in ascending order           */
#define MIPSF_TSDF_BRICK_X 8u                    /* a workgroup owns a brick of 8 x 8 x 16 voxels; a lane owns 4 voxels along z  */
#define MIPSF_TSDF_BRICK_Y 8u
#define MIPSF_TSDF_BRICK_Z 16u
#define MIPSF_TSDF_MAX_BRICKS 0xffffffu           /* bricks of a volume: 256 lanes each, below 2^32 lanes a launch (a cube of 2^31 */
                                                 /* voxels has 2^21; only a volume a few voxels thin comes near)                  */

/* mipsf_tsdf_integrate_args.flags */
#define MIPSF_TSDF_NO_CULL 1u                    /* every brick tests every view (tools/tsdf_time.py times the culling with it)  */

typedef struct mipsf_tsdf_record {
    uint64_t updates;                   /* (voxel, view) pairs of this call with `updated` below                              */
    uint64_t observed;                  /* voxels whose weight is positive after the call                                      */
} mipsf_tsdf_record;

/* The state of a volume is the caller's: tsdf fp32 [X,Y,Z], weight fp32 [X,Y,Z], optionally color fp32 [X,Y,Z,3], C order, all
 * zero before the first call.  Voxel (i,j,k) sits at the world position p = ((float)ticks[0][i], (float)ticks[1][j],
 * (float)ticks[2][k]): three float64 tick arrays, the grid description of mipsf_fuse.h.
 *
 * mipsf_tsdf_integrate fuses n views: depth fp32 [n,H,W] (0 = no measurement, the datasets' value), optionally rgb fp32
 * [n,H,W,3], poses fp32 [n,4,4] (camera to world, row-major, the OpenGL convention: the camera looks along its -z, +y is up;
 * R = pose[:3,:3], t = pose[:3,3]; taken as rigid: the transpose of R stands for its inverse).  The projection is word for word
 * that of mipsf_raster_visible, so a voxel lands on the pixel mipsf_raster_depth drew for it.  In float64, parentheses give the
 * order, for voxel p and the views k = 0 .. n-1 IN THIS ORDER:
 *   q = p - t;  cam[c] = (R[0][c]*q.x + R[1][c]*q.y) + R[2][c]*q.z;  z = -cam.z
 *   u = cx + fx*(cam.x/z);  v = cy - fy*(cam.y/z);  col = floor(u + 0.5);  row = floor(v + 0.5)
 *   inside  = z > 0 && 0 <= col && col < W && 0 <= row && row < H     (compared as doubles, before any conversion to an integer;
 *                                                                      a NaN fails every comparison)
 *   d       = (double)D[k][row][col];   usable = d > 0 && d < inf && d <= depth_max
 *   sdf     = d - z;                    updated = inside && usable && sdf >= -trunc
 *   val     = sdf/trunc;  if (val > 1.0) val = 1.0
 *   w0      = (double)weight[p];  w1 = w0 + 1.0
 *   tsdf[p]     = (float)((((double)tsdf[p])*w0 + val) / w1)
 *   color[p][c] = (float)((((double)color[p][c])*w0 + (double)rgb[k][row][col][c]) / w1)      c = 0..2, when colour is fused
 *   weight[p]   = (float)(w1 < max_weight ? w1 : max_weight)
 * The running values are rounded to fp32 after EVERY view (they live in registers across the views of a call, as fp32), so
 * cutting the views into several calls does not reach the bytes.  The sign is the project's: positive in free space, negative
 * behind the surface.  A voxel no view updates keeps its words.
 *
 * Kernel: a workgroup owns a brick of voxels.  Per chunk of MIPSF_TSDF_VIEW_CHUNK views, one lane per view tests the brick's
 * bounding sphere against the view's frustum (a pixel wider on every side), the camera plane and the depth depth_max + trunc
 * beyond which nothing updates; the survivors go to a list in ascending view order (ballot, exclusive scan) and every lane takes
 * its voxels through the list.  The test has arithmetic of its own; it never leaves out a pair the rule above updates
 * (tests/test_gpu_tsdf.py compares against a restatement that tests every pair).
 *
 * record: filled with the two counts (cleared first; integer sums).  n = 0 is a no-op that writes a zero record.
 * Refused on the host, with nothing launched: X, Y, Z, H or W zero (H and W may be zero when n is), X * Y * Z above
 * MIPSF_TSDF_MAX_VOXELS, more than MIPSF_TSDF_MAX_BRICKS bricks, H or W above MIPSF_TSDF_MAX_SIDE, trunc not positive and finite, fx or fy not positive and finite, cx or
 * cy not finite, a NaN among the doubles, depth_max NaN, max_weight < 1 or NaN, unknown flags, rgb without color or color without
 * rgb, a null pointer (depth, rgb and poses are not looked at when n is 0: an empty stack has no address). */
typedef struct mipsf_tsdf_integrate_args {
    uint32_t struct_size;
    uint32_t X, Y, Z;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_TSDF_NO_CULL                                                                  */
    double fx, fy, cx, cy, trunc, depth_max, max_weight;
    const double* ticks[3];             /* [X], [Y], [Z]                                                                       */
    const float* depth;                 /* [n,H,W]                                                                             */
    const float* rgb;                   /* [n,H,W,3] or null                                                                   */
    const float* poses;                 /* [n,4,4]                                                                             */
    float* tsdf;                        /* [X,Y,Z]                                                                             */
    float* weight;                      /* [X,Y,Z]                                                                             */
    float* color;                       /* [X,Y,Z,3] or null; there exactly when rgb is                                        */
    mipsf_tsdf_record* record;
} mipsf_tsdf_integrate_args;

int mipsf_tsdf_integrate(const mipsf_tsdf_integrate_args* a, void* stream);

/* The colour of m points given in INDEX units (float64 [m,3], what marching cubes returns): trilinear interpolation of `color`
 * over the eight surrounding voxels, each voxel's share multiplied by (weight > 0) and the shares renormalised.  In float64, per
 * axis a with coordinate x and D voxels:
 *   i0 = D > 1 ? min(max(floor(x), 0), D - 2) : 0;  i1 = D > 1 ? i0 + 1 : 0;  f = min(max(x - i0, 0.0), 1.0)
 * and over the corners (a, b, c) in the order 000, 001, 010, 011, 100, 101, 110, 111 (c, the z bit, fastest):
 *   s   = ((a ? fx : 1.0 - fx) * (b ? fy : 1.0 - fy)) * (c ? fz : 1.0 - fz);   m = weight[corner] > 0 ? s : 0.0
 *   den = den + m;  num[ch] = num[ch] + m * (double)color[corner][ch]          (both start at 0.0)
 *   out[ch] = den > 0 ? (float)(num[ch] / den) : 0
 * A point with a coordinate that is not finite gets 0.  m = 0 is a no-op. */
typedef struct mipsf_tsdf_sample_args {
    uint32_t struct_size;
    uint32_t X, Y, Z;
    uint32_t m;
    uint32_t reserved;
    const double* points;               /* [m,3] in index units                                                                */
    const float* weight;                /* [X,Y,Z]                                                                             */
    const float* color;                 /* [X,Y,Z,3]                                                                           */
    float* out;                         /* [m,3]                                                                               */
} mipsf_tsdf_sample_args;

int mipsf_tsdf_sample(const mipsf_tsdf_sample_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_TSDF_H */
