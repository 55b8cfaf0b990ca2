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

#ifdef __cplusplus
}
#endif
#endif
