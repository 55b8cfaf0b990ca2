/*
 * mipsf_compact.h -- the live-sample list of the decoder's backward: the samples whose incoming gradient is not zero, packed
 * into dense 32-sample tiles for mipsf_decoder_bwd_chain16 and mipsf_decoder_wgrad16 (their `live_list` fields, mipsf.h) and for
 * the streaming d(x) of the hash grid.  DESIGN.md 4.4.
 *
 * Same conventions as mipsf.h: int return code, message through mipsf_last_error(), DEVICE pointers, everything enqueued on
 * `stream`, no allocation and no synchronisation.
 */
#ifndef MIPSF_COMPACT_H
#define MIPSF_COMPACT_H

#include "mipsf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LIVE-SAMPLE LIST.  A sample is live iff any of the 10 components of its incoming gradient dout [M,10] is != 0.0f (-0.0 is
 * dead, a subnormal is live).  live_list (MIPSF_SIZE_DECODER_LIVE_LIST words) receives
 *     [0]                    n_live
 *     [1]                    the number of compact 32-sample tiles, ceil(n_live / 32)
 *     [2 .. MIPSF_LIVE_HEADER)  scratch of the call
 *     [MIPSF_LIVE_HEADER + k]   the k-th live sample in ASCENDING order (whatever the schedule), k < n_live; then
 *                               MIPSF_LIVE_PAD up to the next multiple of 32
 * and every dead sample gets zeros in dfeat (its 32 floats in `feat_layout`) and dx [M,3].  Two launches whose grids depend on M
 * only, no host synchronisation: capturable in a hipGraph. */
#define MIPSF_LIVE_HEADER 16u
#define MIPSF_LIVE_PAD 0xffffffffu
int mipsf_decoder_live_compact(const float* dout, uint32_t M, uint32_t* live_list, float* dfeat, float* dx, int feat_layout,
                               void* stream);

/* mipsf_hashgrid_dx_from_jac for the samples of a live-sample list only: one thread per list entry, the
 * same arithmetic per sample.  The samples that are not listed have a zero feature gradient and add nothing. */
int mipsf_hashgrid_dx_from_jac_list(const float* jac, const float* dout, float* dx, const uint32_t* live_list, uint32_t M,
                                    const mipsf_grid_meta* meta_host, int layout, void* stream);

/* RAY MASK.  `wants_dx`: one uint32 per ray of S consecutive samples; 0 = the gradient of the ray's points reaches no
 * parameter (its pose is one of the fixed ones), so nobody needs d feat / d x of its samples.
 *   mipsf_gather_pose_place_fwd_masked   mipsf_gather_pose_place_fwd that also writes the mask: wants_dx[n] = owner[n] >= F
 *                                        (an owner out of range counts as pose 0, as in mipsf_place_pose_bwd)
 *   mipsf_hashgrid_fwd_masked            mipsf_hashgrid_fwd; with jac and ray_mask != NULL the Jacobian of a masked ray's
 *                                        samples is NOT stored (those words of jac keep what they held); out is unchanged
 *   mipsf_hashgrid_dx_from_jac_masked    mipsf_hashgrid_dx_from_jac (tile_live) / _list (live_list), at most one of the two;
 *                                        a sample of a masked ray that the call visits gets dx = +0.0f (what was there is
 *                                        dropped) and neither its Jacobian nor its gradient is read
 * M must be a multiple of S.  ray_mask == NULL: exactly the unmasked functions. */
int mipsf_gather_pose_place_fwd_masked(const float* db, uint64_t n_rows, const int64_t* idx, const float* fixed_poses,
                                       const float* rot, const float* trans, uint32_t F, uint32_t K, const int64_t* owner,
                                       const float* noise, const float* z_uniform, const float* z_near_offsets,
                                       const float* z_near_nodepth, const mipsf_render_cfg* cfg_host, float* d_cam, float* rgb,
                                       float* depth, float* z_vals, float* xn, uint32_t* counts, uint32_t* wants_dx, uint32_t N,
                                       void* stream);
int mipsf_hashgrid_fwd_masked(const float* x, const float* params, float* out, float* jac, const uint32_t* ray_mask, uint32_t S,
                              uint32_t M, const mipsf_grid_meta* meta_host, int layout, void* stream);
int mipsf_hashgrid_dx_from_jac_masked(const float* jac, const float* dout, float* dx, const uint32_t* tile_live,
                                      const uint32_t* live_list, const uint32_t* ray_mask, uint32_t S, uint32_t M,
                                      const mipsf_grid_meta* meta_host, int layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif
