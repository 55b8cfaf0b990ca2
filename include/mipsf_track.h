/*
 * mipsf_track.h -- the model side of a frame-to-model depth tracker over the volume of mipsf_tsdf.h: depth, normal and colour
 * images of the volume from a pose by ray casting (no marching, no rasterising), and a point-to-plane registration of a live depth
 * frame against such images by projective association.  DESIGN.md 4.21; mipsfusion_amd/tsdf.py.
 *
 * Same conventions as mipsf_tsdf.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation; workspaces are the
 * caller's (mipsf_track_workspace_bytes), 16-byte aligned.  Nothing here uses a floating-point atomic (the hit count is an integer
 * sum; the registration's sums are added lane -> wave -> block partials -> one wave, in index order); the same call gives the same
 * bytes.  Every floating-point operation named below is one IEEE float64 operation rounded on its own (no contraction, no
 * reciprocal), fp32 inputs widened first, so a float64 restatement on the host (tests/track_cpu.py) gives the same words; the sines
 * and cosines of the registration's update are the only operations not fixed to a word.
 */
#ifndef MIPSF_TRACK_H
#define MIPSF_TRACK_H

#include <stdint.h>

#include "mipsf_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_TRACK_MAX_SAMPLES 0x100000u        /* samples of a ray: the walk ends at this index at the latest                  */
#define MIPSF_TRACK_TILE 16u                     /* a workgroup takes 16 x 16 pixels of one view, a wave 8 x 8 of them           */
#define MIPSF_TRACK_RESULT_DOUBLES 20u           /* = MIPSF_ICP_RESULT_DOUBLES: T row major, pairs, fitness, rmse, iterations    */
#define MIPSF_TRACK_MAX_ITERATION 1000u
#define MIPSF_TRACK_MAX_VIEWS 65535u               /* views of one ray-cast call (the second grid dimension)                       */

/* mipsf_track_raycast_args.flags */
#define MIPSF_TRACK_NO_SKIP 1u                   /* every sample is evaluated (tools/track_time.py times the skipping with it)   */

/* mipsf_track_workspace_bytes(which, a, b, c) */
#define MIPSF_TRACK_WS_RAYCAST 1                 /* a, b, c = X, Y, Z                                                            */
#define MIPSF_TRACK_WS_REGISTER 2                /* a, b = H, W                                                                  */

typedef struct mipsf_track_record {
    uint64_t hits;                      /* pixels of this call with a depth (integer sum)                                      */
    uint64_t marked;                    /* bricks the marking pass marked (0 with MIPSF_TRACK_NO_SKIP)                          */
} mipsf_track_record;

/* 0: a side is 0, the volume has more than MIPSF_TSDF_MAX_VOXELS voxels or MIPSF_TSDF_MAX_BRICKS bricks, or `which` is unknown */
uint64_t mipsf_track_workspace_bytes(int which, uint32_t a, uint32_t b, uint32_t c);

/* mipsf_track_raycast: depth fp32 [n,H,W] (z-depth as the datasets give it, 0 = no hit), optionally normals fp32 [n,H,W,3] (world
 * frame, pointing into free space, 0 0 0 = none) and colour fp32 [n,H,W,3] of the volume tsdf fp32 [X,Y,Z], weight fp32 [X,Y,Z],
 * color fp32 [X,Y,Z,3] seen from n poses fp32 [n,4,4] (camera to world, the OpenGL convention of mipsf_tsdf.h: R = pose[:3,:3],
 * t = pose[:3,3]).  Voxel (i,j,k) sits at origin + voxel*(i,j,k) in float64; mipsf_tsdf_integrate placed it at the fp32 rounding of
 * that tick, so the two differ by at most half an fp32 ulp of the coordinate.  The tsdf and weight words are read as fp32 and
 * widened; D_a are X, Y, Z.  Per view and pixel (row, col), in float64, parentheses give the order:
 *
 *   dc   = ((col - cx)/fx, -((row - cy)/fy), -1)
 *   d[r] = (R[r][0]*dc.x + R[r][1]*dc.y) + R[r][2]*dc.z
 *   len  = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);  miss unless len > 0 && len < inf
 *   dt   = step/len                              (the ray parameter IS the z-depth, because dc.z = -1)
 *   box: lo[a] = origin[a], hi[a] = origin[a] + voxel*(D_a - 1)
 *   per axis with d[a] != 0: ta = (lo[a] - t[a])/d[a], tb = (hi[a] - t[a])/d[a]
 *        an axis with d[a] == 0 misses when t[a] < lo[a] or t[a] > hi[a], and is ignored otherwise
 *   t_in  = max(near, max over the axes of min(ta, tb));  t_out = min(far, min over the axes of max(ta, tb))
 *        (max(x, y) = y > x ? y : x and min(x, y) = y < x ? y : x, folded over the axes 0, 1, 2 starting from near and far)
 *   miss unless t_out >= t_in
 *   samples: t_i = t_in + (double)i*dt for i = 0, 1, ... while t_i <= t_out and i < MIPSF_TRACK_MAX_SAMPLES  (no running sum)
 *
 *   field at p[a] = t[a] + d[a]*t_i:
 *        g[a] = (p[a] - origin[a])/voxel;  i0[a] = floor(g[a])
 *        KNOWN only when 0 <= i0[a] <= D_a - 2 on every axis and all eight corner weights (double)w >= min_weight
 *        fr = g - i0
 *        c_ab = v_ab0*(1 - fr.z) + v_ab1*fr.z;  c_a = c_a0*(1 - fr.y) + c_a1*fr.y;  f = c_0*(1 - fr.x) + c_1*fr.x
 *   walk, with prev = the sample before (unknown before the first):
 *        prev known, cur known, prev > 0, cur <= 0  ->  HIT: t* = t_{i-1} + dt*(prev/(prev - cur));  depth = (float)t*;  stop
 *        prev known, cur known, prev < 0, cur > 0   ->  back face: stop, no hit
 *        otherwise go on
 *   A hit whose (float)t* is not positive and finite counts as no hit.
 *   normal at p*[a] = t[a] + d[a]*t*:  grad[a] = f(p* + voxel*e_a) - f(p* - voxel*e_a)   (p*[a] + voxel, p*[a] - voxel)
 *        all six known and L = sqrt((gx*gx + gy*gy) + gz*gz) positive and finite:  n = (float)(grad/L);  else n = 0 0 0, the depth stays
 *   colour at p*: the rule of mipsf_tsdf_sample at the index-unit point g(p*), word for word.
 *
 * A rigid pose advances p by `step` metres a sample, so a ray has at most diag/step + 2 samples inside the box, with
 * diag = voxel*sqrt((X-1)^2 + (Y-1)^2 + (Z-1)^2); a step for which that exceeds MIPSF_TRACK_MAX_SAMPLES is refused.
 *
 * Empty-space skipping.  One launch marks every brick of MIPSF_TSDF_BRICK_X x _Y x _Z voxels, bricks in (x, y, z) order with z
 * fastest, one byte a brick in the workspace: the mark is set when the brick, taken with an apron of one voxel on every side
 * (clipped to the volume), holds a voxel with (double)weight >= min_weight and tsdf <= 0.  Call a sample FREE when some i0[a] is
 * outside 0 .. D_a - 2 (it is unknown), or the brick of voxel i0 is unmarked: its eight corners i0 .. i0 + 1 lie in that brick's
 * apron, so each is below min_weight or positive, and the sample is unknown or -- a sum of non-negative products of positive words
 * of which one has all three shares >= 1/2 -- positive.  A hit needs cur <= 0 and a back face prev < 0, so a free sample fires
 * neither as cur, and as prev it can only feed the hit of a sample that is not free.  Hence sample i is evaluated exactly when
 * sample i or sample i + 1 is not free (a sample past t_out counts as free); a sample left out is handed on as `unknown`, which
 * only a free successor ever sees.  MIPSF_TRACK_NO_SKIP evaluates every sample; the words are the same either way.  The six
 * samples of the normal are always evaluated.
 *
 * Kernel: a workgroup of 256 lanes takes a tile of 16 x 16 pixels of one view, a wave 8 x 8 of them, a lane one ray: neighbouring
 * rays read the same bricks and marks.  A lane that has hit or left the box idles until its wave is through.
 *
 * record: cleared first, then filled.  n = 0 is a no-op that writes a zero record.  Refused on the host, with nothing launched:
 * X, Y, Z zero, X*Y*Z above MIPSF_TSDF_MAX_VOXELS, more than MIPSF_TSDF_MAX_BRICKS bricks, H or W zero (unless n is) or above
 * MIPSF_TSDF_MAX_SIDE, n above MIPSF_TRACK_MAX_VIEWS, voxel, trunc, step, fx or fy not positive and finite, cx, cy or an origin not finite, near or far NaN,
 * min_weight NaN, a step too small for the volume (above), unknown flags, color_out without color, a null pointer (poses, depth
 * are not looked at when n is 0), a workspace that is not 16-byte aligned. */
typedef struct mipsf_track_raycast_args {
    uint32_t struct_size;
    uint32_t X, Y, Z;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_TRACK_NO_SKIP                                                                 */
    double origin[3], voxel, trunc;
    double fx, fy, cx, cy, near, far, step, min_weight;
    const float* tsdf;                  /* [X,Y,Z]                                                                             */
    const float* weight;                /* [X,Y,Z]                                                                             */
    const float* color;                 /* [X,Y,Z,3] or null                                                                   */
    const float* poses;                 /* [n,4,4]                                                                             */
    float* depth;                       /* [n,H,W]                                                                             */
    float* normals;                     /* [n,H,W,3] or null                                                                   */
    float* color_out;                   /* [n,H,W,3] or null                                                                   */
    mipsf_track_record* record;
    void* workspace;                    /* mipsf_track_workspace_bytes(MIPSF_TRACK_WS_RAYCAST, X, Y, Z)                         */
} mipsf_track_raycast_args;

int mipsf_track_raycast(const mipsf_track_raycast_args* a, void* stream);

/* mipsf_track_register: frame-to-model point-to-plane ICP by projective association.  model_depth fp32 [H,W] and model_normals
 * fp32 [H,W,3] are one view of mipsf_track_raycast, cast from pose_ref fp32 [4,4]; live fp32 [H,W] is the depth frame; T, the live
 * camera's camera-to-world pose in float64, starts at pose_init fp32 [4,4] widened.  All of them are DEVICE pointers, the poses
 * too, so the stages of an odometry loop hand the pose on without the host.
 *
 * One evaluation, per live pixel (row, col) with d = (double)live[row][col], usable = d > 0 && d < inf && d <= depth_max:
 *   p_c = (d*((col - cx)/fx), -(d*((row - cy)/fy)), -d)
 *   p[r] = ((T[r][0]*p_c.x + T[r][1]*p_c.y) + T[r][2]*p_c.z) + T[r][3]
 *   q = p - t_ref;  cam[c] = (R_ref[0][c]*q.x + R_ref[1][c]*q.y) + R_ref[2][c]*q.z;  z = -cam.z
 *   u = cx + fx*(cam.x/z);  v = cy - fy*(cam.y/z);  col2 = floor(u + 0.5);  row2 = floor(v + 0.5)
 *   inside = z > 0 && 0 <= col2 && col2 < W && 0 <= row2 && row2 < H          (the projection of mipsf_tsdf_integrate)
 *   dm = (double)model_depth[row2][col2], must be > 0 and < inf
 *   m_c = (dm*((col2 - cx)/fx), -(dm*((row2 - cy)/fy)), -dm);  v_m[r] = ((R_ref[r][0]*m_c.x + R_ref[r][1]*m_c.y) + R_ref[r][2]*m_c.z) + t_ref[r]
 *   nrm = (double)model_normals[row2][col2], with (nx*nx + ny*ny) + nz*nz > 0
 *   dx, dy, dz = p - v_m;  d2 = (dx*dx + dy*dy) + dz*dz;  pair when d2 <= max_dist*max_dist
 *   r = (dx*nx + dy*ny) + dz*nz;  J = (p x nrm, nrm)
 * The sums are those of mipsf_icp_register (the upper triangle of J^T J row by row, J^T r, the pair count, the sum of d2) and the
 * count of usable pixels, per block of 256 pixels in row-major order and then in block order.  The judgement, the Cholesky with
 * its 1e-12 pivot rule, R = Rz Ry Rx, T <- U T and the stop are those of mipsf_icp_register (csrc/icp_dev.h states them once for
 * both): fitness = pairs / usable pixels, rmse = sqrt(sum d2 / pairs).  max_iteration + 1 evaluations are enqueued; once the loop
 * has stopped the later ones return at once.
 *
 * result: MIPSF_TRACK_RESULT_DOUBLES doubles -- T row major, correspondences, fitness, inlier rmse, iterations.  pose_out fp32
 * [4,4] = (float)T, rewritten by every finished evaluation (it may be neither pose_init nor pose_ref).  partner (optional) int32
 * [H,W]: the model pixel row2*W + col2 of the last evaluation, or -1.
 * Refused on the host: H or W zero or above MIPSF_TSDF_MAX_SIDE, fx or fy not positive and finite, cx or cy not finite, depth_max
 * NaN, max_dist negative, infinite or NaN, max_iteration above MIPSF_TRACK_MAX_ITERATION, a null pointer, a workspace that is not
 * 16-byte aligned. */
typedef struct mipsf_track_register_args {
    uint32_t struct_size;
    uint32_t H, W;
    uint32_t max_iteration;
    double fx, fy, cx, cy, depth_max, max_dist, relative_fitness, relative_rmse;
    const float* model_depth;           /* [H,W]                                                                               */
    const float* model_normals;         /* [H,W,3]                                                                             */
    const float* pose_ref;              /* [4,4]                                                                               */
    const float* live;                  /* [H,W]                                                                               */
    const float* pose_init;             /* [4,4]                                                                               */
    double* result;                     /* [MIPSF_TRACK_RESULT_DOUBLES]                                                        */
    float* pose_out;                    /* [4,4]                                                                               */
    int32_t* partner;                   /* [H,W] or null                                                                       */
    void* workspace;                    /* mipsf_track_workspace_bytes(MIPSF_TRACK_WS_REGISTER, H, W, 0)                        */
} mipsf_track_register_args;

int mipsf_track_register(const mipsf_track_register_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_TRACK_H */
