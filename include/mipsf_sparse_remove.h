/*
 * mipsf_sparse_remove.h -- views taken out of the brick-sparse volume of mipsf_sparse.h again, for the views whose pose a loop
 * closure moved (remove at the old pose, fuse at the new one) and for a frame that turned out to be bad.  A brick takes the views
 * of a call only from the view that first marked it (`birth`, mipsf_sparse.h), so a removal has to know which views a brick
 * holds: an opt-in per-brick history, one word per slot, kept by mipsf_sparse_stamp.  DESIGN.md 4.27; mipsfusion_amd/sparse_tsdf.py
 * (SparseTSDFVolume(history=True), deintegrate, reintegrate).
 *
 * Same conventions as mipsf_sparse.h: int return code, message through mipsf_last_error(), one argument block with `struct_size`
 * first, DEVICE pointers, everything enqueued on `stream`, kernels only (a call replays from a captured graph), no allocation and
 * no synchronisation.  Nothing here uses a floating-point atomic (the five counts are integer sums); a voxel is owned by one lane
 * for the whole call; the same call gives the same bytes.  Every floating-point operation is one IEEE float64 operation rounded on
 * its own, fp32 inputs widened first, so a float64 restatement on the host (tests/sparse_remove_cpu.py) gives the same words.
 */
#ifndef MIPSF_SPARSE_REMOVE_H
#define MIPSF_SPARSE_REMOVE_H

#include <stdint.h>

#include "mipsf_deintegrate.h"
#include "mipsf_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_SPARSE_UNBORN 0xffffffffu          /* born[slot] of a slot that took no view yet                                    */
#define MIPSF_SPARSE_MAX_VIEW_ID 0xfffffffeu     /* the largest view id; the host stops fusing before the serial passes it        */

/* The history of a volume is the caller's, on the device, beside the state of mipsf_sparse.h:
 *   born   uint32 [capacity]: the id of the first view a slot took; MIPSF_SPARSE_UNBORN before (all of it before the first call)
 *   serial uint32 [1]: the id of the next view (0 before the first call)
 * The id of a view is the count of views handed to mipsf_sparse_stamp before it, whatever their poses: a view with a NaN pose,
 * which marks and updates nothing, has one too.
 *
 * mipsf_sparse_stamp: between mipsf_sparse_allocate and mipsf_sparse_integrate of the SAME n views.  Two launches:
 *   1. for every slot s < min(count, capacity) with born[s] == MIPSF_SPARSE_UNBORN:  born[s] = serial[0] + birth[s]
 *      (birth is what mipsf_sparse_allocate left: the first view of this call the slot takes, 0 for a slot from before)
 *   2. one lane: serial[0] = serial[0] + n
 * The second launch follows the first on the stream, so no lane reads serial while it changes.  Because the slots in use before
 * the call are stamped already and the new ones have birth = their first view, "the views k >= birth of this call and all views of
 * later calls" is "the views with id >= born[s]", whatever the cut into calls.  n = 0 stamps nothing new and leaves serial.
 * Nothing but born and serial is written.  Refused on the host, with nothing launched: what mipsf_sparse_allocate refuses of the
 * volume; n above MIPSF_SPARSE_MAX_VIEWS; a null born or serial.  (serial + n passing MIPSF_SPARSE_MAX_VIEW_ID is the caller's to
 * prevent: the word lives on the device.) */
typedef struct mipsf_sparse_stamp_args {
    uint32_t struct_size;
    uint32_t n;
    mipsf_sparse_volume vol;
    uint32_t* born;                     /* [capacity]                                                                          */
    uint32_t* serial;                   /* [1]                                                                                 */
} mipsf_sparse_stamp_args;

int mipsf_sparse_stamp(const mipsf_sparse_stamp_args* a, void* stream);

typedef struct mipsf_sparse_remove_record {
    uint64_t removed;                   /* (voxel, view) pairs of this call taken out of a voxel with a positive weight         */
    uint64_t missing;                   /* pairs the rule hits whose voxel had no positive weight left: nothing to take out     */
    uint64_t emptied;                   /* removals that brought a voxel back to the never-observed state                       */
    uint64_t observed;                  /* voxels of the slots in use whose weight is positive after the call                   */
    uint64_t bricks_emptied;            /* slots in use without a voxel of positive weight after the call                       */
} mipsf_sparse_remove_record;

/* mipsf_sparse_deintegrate: the views, the intrinsics, trunc, depth_max and flags (MIPSF_TSDF_NO_CULL) are those of
 * mipsf_sparse_integrate; view_ids[k] is the id view k was fused under.  For every voxel p of every slot s < min(count, capacity)
 * that lies inside the grid, at ((float)ticks[0][i], (float)ticks[1][j], (float)ticks[2][k]), and the views k = 0 .. n-1 IN THIS
 * ORDER:
 *   view k is skipped unless view_ids[k] >= born[s]            (the brick never took it; an unstamped slot takes none)
 *   otherwise, with the projection, `inside`, `usable`, `sdf` and `val` of mipsf_tsdf_integrate word for word and
 *   hit = inside && usable && sdf >= -trunc:
 *     w0 = (double)weight[p]
 *     hit && !(w0 > 0):  missing += 1, the words stay        (nothing of this view is in the voxel; a NaN weight lands here)
 *     hit &&   w0 > 0 :  removed += 1;  w1 = w0 - 1.0
 *          !(w1 > 0):    tsdf[p] = 0, color[p][:] = 0, weight[p] = 0;  emptied += 1    (the never-observed state, no division)
 *          else:         tsdf[p]     = (float)((((double)tsdf[p])*w0 - val) / w1)
 *                        color[p][c] = (float)((((double)color[p][c])*w0 - (double)rgb[k][row][col][c]) / w1)       c = 0..2
 *                        weight[p]   = (float)w1
 *   observed       = voxels of the slots in use with a positive weight after the call
 *   bricks_emptied = slots in use with no such voxel after the call: where a later freeing of bricks would start
 * which is the rule of mipsf_deintegrate_views (mipsf_deintegrate.h) under the mask of the history.  The running words are rounded
 * to fp32 after EVERY view, so cutting the views into several calls does not reach the bytes.  Words of a slot that lie outside
 * the grid stay zero.  Nothing is freed: table, slot_brick, count, birth, born are read only, and nothing is written at or beyond
 * slot `count`.
 *
 * What the caller owes is what mipsf_deintegrate_views asks: the same images, poses, intrinsics, trunc and depth_max the views
 * were fused with, a volume that was never capped (there is no max_weight here), and ids that are those views' ids.
 *
 * Kernel: that of mipsf_sparse_integrate: a workgroup per slot, `capacity` launched, those at or beyond `count` return; four
 * voxels a lane, kept in registers across the views; per chunk of 256 views one lane per view tests the brick's ball AND
 * view_ids[k] >= born[s]; the survivors are listed in ascending k.  The counts are integer block sums and one integer atomic each
 * per workgroup.
 *
 * record: cleared first (by a kernel).  n = 0 takes no view out: removed, missing and emptied are 0, observed and bricks_emptied
 * are counted.  Refused on the host, with nothing launched: what mipsf_sparse_integrate refuses, less max_weight; a null view_ids
 * (unless n is 0) or born. */
typedef struct mipsf_sparse_deintegrate_args {
    uint32_t struct_size;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_TSDF_NO_CULL                                                                  */
    uint32_t reserved;
    double fx, fy, cx, cy, trunc, depth_max;
    mipsf_sparse_volume vol;
    const float* depth;                 /* [n,H,W]                                                                             */
    const float* rgb;                   /* [n,H,W,3] or null; there exactly when vol.color is                                  */
    const float* poses;                 /* [n,4,4]                                                                             */
    const uint32_t* view_ids;           /* [n]                                                                                 */
    const uint32_t* born;               /* [capacity]                                                                          */
    mipsf_sparse_remove_record* record;
} mipsf_sparse_deintegrate_args;

int mipsf_sparse_deintegrate(const mipsf_sparse_deintegrate_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SPARSE_REMOVE_H */
