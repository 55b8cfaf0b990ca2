/*
 * mipsf_submap.h -- the geometry behind a sub-map decision (upstream: Manager.py process_keyframe_normal /
 * process_keyframe_wait_loop / find_overlapping_region, all host torch on a host copy of the depth image).  The decision rules
 * stay on the host (mipsfusion_amd/submap_manager.py); these calls reduce a frame that is already on the device to integer
 * counts, float32 minima / maxima and a few float64 sums.  DESIGN.md 4.16 states what is computed; tests/submap_cpu.py restates it.
 *
 * Same conventions as mipsf_posegraph.h: int return code, message through mipsf_last_error(), one argument block with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation, capturable.
 * Nothing uses an atomic of any kind: every count and every sum is a fixed tree, the same call gives the same bytes.
 *
 * A frame is ray rows [H*W,7] (direction, rgb, depth) and a camera -> world pose [4,4] float32.  A point is
 *   d_world[i] = (x*R[i][0] + y*R[i][1]) + z*R[i][2];   p[i] = t[i] + d_world[i]*depth          (float32, no contraction)
 * A lattice (num_h, num_w) is helper_functions/sampling_helper.py sample_pixels_uniformly(H, W, num_h, num_w) as index arithmetic.
 */
#ifndef MIPSF_SUBMAP_H
#define MIPSF_SUBMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_SUBMAP_MAX_BOXES 64u        /* the pose graph's MIPSF_POSEGRAPH_MAX_NODES */
#define MIPSF_SUBMAP_MAX_TOP_KF 10u       /* keyframeSet.near_kf_num */
#define MIPSF_SUBMAP_HEADER_WORDS 16u
#define MIPSF_SUBMAP_BOX_WORDS 12u
#define MIPSF_SUBMAP_RECORD_WORDS (MIPSF_SUBMAP_HEADER_WORDS + MIPSF_SUBMAP_MAX_BOXES * MIPSF_SUBMAP_BOX_WORDS)
#define MIPSF_SUBMAP_WORKSPACE_BYTES 8192u /* 256 partial surface boxes of 8 words */

/* The record (32-bit words; f = float32 bits, u = uint32):
 *   0      u  pixels with near < depth < far
 *   1..3   f  min of their points (+inf when word 0 is 0)      4..6  f  max (-inf)
 *   7      u  lattice A points with depth > 0
 *   8..13     lattice C: sum of the points, 3 float64 (the points are float32; the sum has a fixed order)
 *   14     u  n_boxes                                           15    0
 *   16 + 12 i, one block per sub-map i:
 *     +0..2 f  centre, +3..5 f length of localMLP_expand_rule(box_i, surface box, max_len_i)
 *     +6    u  lattice A points with depth > 0 strictly inside box_i with its lengths clamped below by min_cr_len
 *     +7    u  lattice A points with depth > 0 strictly inside the expanded box
 *     +8    u  lattice B points (NO depth mask: a zero-depth pixel counts as the camera centre) strictly inside box_i
 *     +9    u  the expand rule's case per axis, axis a in bits 8a..8a+7 (0 contained, 1 full, 2 free, 3 positive, 4 negative, 5 both)
 *     +10,11   0
 */
typedef struct mipsf_submap_frame_stats_args {
    uint32_t struct_size;
    uint32_t H, W;
    uint32_t n_boxes;                   /* 1 .. MIPSF_SUBMAP_MAX_BOXES */
    uint32_t lat_a_h, lat_a_w;          /* containing ratios (upstream 150 x 200) */
    uint32_t lat_b_h, lat_b_w;          /* most-overlapping score (15 x 20) */
    uint32_t lat_c_h, lat_c_w;          /* mapping.overlapping.n_rays_h x n_rays_w */
    float near, far;
    float min_cr_len[3];
    uint32_t reserved;
    const float* rows;                  /* [H*W,7] */
    const float* pose;                  /* [4,4] row major */
    const float* boxes;                 /* [n_boxes,6] centre, length */
    const float* max_len;               /* [n_boxes,3] */
    uint32_t* record;                   /* MIPSF_SUBMAP_RECORD_WORDS; words of sub-maps >= n_boxes are not written */
    void* workspace;                    /* MIPSF_SUBMAP_WORKSPACE_BYTES, 8-byte aligned; needs no initialisation */
} mipsf_submap_frame_stats_args;

int mipsf_submap_frame_stats(const mipsf_submap_frame_stats_args* a, void* stream);

/* find_overlapping_region (Manager.py:261-337).  Two phases, either may be empty (n_related = 0 or k = 0) but not both; the host
 * ranks the distances of phase (a) between two calls.
 *  (a) for each related keyframe j: c = mean over its rows_per_slot rows of direction*depth (float32 products, float64 sum, fixed
 *      order), moved with its camera -> world pose as keyframeSet.sort_center_dist_kf does; dist[j] = |c_world - centre of the
 *      frame's lattice points| in float64.  A slot outside [0, n_slots) gives NaN and is not read.
 *  (b) for each chosen keyframe: the lattice points through the rigid inverse of its pose in float64, projected as
 *      project_to_pixel does (x negated, z + 1e-5); seen = edge < u < cam_W - edge, edge < v < cam_H - edge, z_cam < 0.
 *      mask_final = seen by any & strictly inside target_box.
 */
typedef struct mipsf_submap_overlap_args {
    uint32_t struct_size;
    uint32_t H, W;
    uint32_t lat_h, lat_w;              /* P = lat_h * lat_w */
    uint32_t n_related;                 /* phase (a) */
    uint32_t k;                         /* phase (b), <= MIPSF_SUBMAP_MAX_TOP_KF */
    uint32_t n_slots, rows_per_slot;
    uint32_t reserved;
    double fx, fy, cx, cy, cam_W, cam_H, edge;
    float target_box[6];                /* centre, length of the sub-map switched to */
    const float* rows;                  /* [H*W,7] */
    const float* pose;                  /* [4,4] */
    const float* table;                 /* [n_slots, rows_per_slot, 7]        (a) */
    const int32_t* related_slots;       /* [n_related]                        (a) */
    const float* related_poses;         /* [n_related,4,4] camera -> world    (a) */
    double* dist;                       /* [n_related]                        (a) */
    const float* top_poses;             /* [k,4,4] camera -> world            (b) */
    uint8_t* top_kf_masks;              /* [k,P]                              (b) */
    uint8_t* mask_final;                /* [P]                                (b) */
    uint32_t* count;                    /* [1] count of mask_final            (b) */
    float* target_d;                    /* [P]                                (b) */
    float* rays_d_cam;                  /* [P,3]                              (b) */
} mipsf_submap_overlap_args;

int mipsf_submap_overlap(const mipsf_submap_overlap_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SUBMAP_H */
