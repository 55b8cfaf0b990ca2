/*
 * mipsf_deintegrate.h -- views taken out of the dense TSDF volume of mipsf_tsdf.h again: the inverse of the running mean of
 * mipsf_tsdf_integrate, for the views whose pose a loop closure moved (remove at the old pose, fuse at the new one) and for a
 * frame that turned out to be bad.  DESIGN.md 4.26; mipsfusion_amd/tsdf.py (TSDFVolume.deintegrate, reintegrate).
 *
 * Same conventions as mipsf_tsdf.h: int return code, message through mipsf_last_error(), one argument block with `struct_size`
 * first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Nothing here uses a
 * floating-point atomic (the four counts are integer sums); a voxel is owned by one lane for the whole call; the same call gives
 * the same bytes.  Every floating-point operation named below is one IEEE float64 operation rounded on its own (no contraction, no
 * reciprocal), fp32 inputs widened first, so a float64 restatement on the host (tests/tsdf_remove_cpu.py) gives the same words.
 */
#ifndef MIPSF_DEINTEGRATE_H
#define MIPSF_DEINTEGRATE_H

#include <stdint.h>

#include "mipsf_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mipsf_deintegrate_record {
    uint64_t removed;                   /* (voxel, view) pairs of this call taken out of a voxel with a positive weight         */
    uint64_t missing;                   /* pairs the rule hits whose voxel had no positive weight left: nothing to take out     */
    uint64_t emptied;                   /* removals that brought a voxel back to the never-observed state                       */
    uint64_t observed;                  /* voxels whose weight is positive after the call                                       */
} mipsf_deintegrate_record;

/* The state, the ticks, the views and the limits on them are those of mipsf_tsdf_integrate (mipsf_tsdf.h), and so are, word for
 * word, the projection, `inside`, `usable`, `sdf` and `val`; flags takes MIPSF_TSDF_NO_CULL.  For voxel p and the views
 * k = 0 .. n-1 IN THIS ORDER, with hit = inside && usable && sdf >= -trunc (`updated` of the fusion):
 *   w0 = (double)weight[p]
 *   hit && !(w0 > 0):  missing += 1, the words stay        (nothing of this view is in the voxel; a NaN weight lands here)
 *   hit &&   w0 > 0 :  removed += 1;  w1 = w0 - 1.0
 *        !(w1 > 0):    tsdf[p] = 0, color[p][:] = 0, weight[p] = 0;  emptied += 1      (the never-observed state, no division)
 *        else:         tsdf[p]     = (float)((((double)tsdf[p])*w0 - val) / w1)
 *                      color[p][c] = (float)((((double)color[p][c])*w0 - (double)rgb[k][row][col][c]) / w1)       c = 0..2
 *                      weight[p]   = (float)w1
 *   observed = voxels with a positive weight after the call
 * The running words are rounded to fp32 after EVERY view, so cutting the views into several calls does not reach the bytes.
 *
 * What the caller owes:
 *   - depth, rgb, poses, the intrinsics, trunc and depth_max are those the views were fused with: the rule finds the pairs of a
 *     view by projecting again, and takes out the value it computes;
 *   - the volume was never capped: a running mean with a finite max_weight is a moving average, which has no removal (there is
 *     no max_weight here);
 *   - `missing` is a diagnostic, not a guarantee: a view that was never fused, removed from voxels other views did reach, counts
 *     as removed and spoils them;
 *   - a pose with a NaN removes nothing, as it fused nothing.
 * Removing in another order than fusing, or some views only, gives the mean of the remaining views up to the rounding of the
 * steps (measured in DESIGN.md 4.26); removing every view gives the all-zero state exactly.
 *
 * Kernel: that of mipsf_tsdf_integrate (a workgroup per brick, four voxels a lane, the chunk's views tested against the brick's
 * ball, the survivors listed in ascending order); the counts are integer block sums and one integer atomic each per workgroup.
 *
 * record: cleared first.  n = 0 is a no-op that writes a zero record.  Refused on the host, with nothing launched: what
 * mipsf_tsdf_integrate refuses, less max_weight. */
typedef struct mipsf_deintegrate_args {
    uint32_t struct_size;
    uint32_t X, Y, Z;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_TSDF_NO_CULL                                                                  */
    double fx, fy, cx, cy, trunc, depth_max;
    const double* ticks[3];             /* [X], [Y], [Z]                                                                       */
    const float* depth;                 /* [n,H,W]                                                                             */
    const float* rgb;                   /* [n,H,W,3] or null                                                                   */
    const float* poses;                 /* [n,4,4]                                                                             */
    float* tsdf;                        /* [X,Y,Z]                                                                             */
    float* weight;                      /* [X,Y,Z]                                                                             */
    float* color;                       /* [X,Y,Z,3] or null; there exactly when rgb is                                        */
    mipsf_deintegrate_record* record;
} mipsf_deintegrate_args;

int mipsf_deintegrate_views(const mipsf_deintegrate_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_DEINTEGRATE_H */
