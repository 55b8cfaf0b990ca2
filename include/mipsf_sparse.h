/*
 * mipsf_sparse.h -- the volume of mipsf_tsdf.h kept only where a depth pixel put a surface: a VIRTUAL grid of bricks of
 * MIPSF_TSDF_BRICK_X x _Y x _Z voxels, an index grid with one word per brick, and a pool of brick-sized slots.  A brick-sparse volume
 * is a dense volume in which a voxel is updated only while its brick is allocated: every output below is the output of the dense rule
 * (mipsf_tsdf.h, mipsf_track.h) on "the masked dense state", the dense state with the voxels of unallocated bricks left at zero.
 * The virtual grid may hold 2^31 voxels and more; a linear voxel index is never formed, addressing is (slot, voxel in brick).
 * DESIGN.md 4.24; mipsfusion_amd/sparse_tsdf.py.
 *
 * Same conventions as mipsf_tsdf.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation, no host round trip.
 * Nothing here uses a floating-point atomic: the marks are an integer atomic minimum (a set, whatever the order of work), the counts
 * integer sums; a voxel is owned by one lane for the whole call; the same call gives the same bytes.  Every floating-point operation
 * named below is one IEEE float64 operation rounded on its own (no contraction, no reciprocal), fp32 inputs widened first, so a
 * float64 restatement on the host (tests/sparse_cpu.py) gives the same words.
 */
#ifndef MIPSF_SPARSE_H
#define MIPSF_SPARSE_H

#include <stdint.h>

#include "mipsf_track.h"
#include "mipsf_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_SPARSE_BRICK_VOXELS 1024u          /* MIPSF_TSDF_BRICK_X * _Y * _Z: the words of a slot                            */
#define MIPSF_SPARSE_MAX_BRICKS 0x7fffffffu      /* bricks of the virtual grid: below 2^31                                       */
#define MIPSF_SPARSE_MAX_CAPACITY 0x100000u      /* slots of a pool: 2^31 / 2048, so a word offset into tsdf or weight is below 2^30 */
#define MIPSF_SPARSE_MAX_STEPS 4096u             /* ceil(band / voxel)                                                           */
#define MIPSF_SPARSE_MAX_VIEWS 65535u            /* views of one call (the second grid dimension)                                */
#define MIPSF_SPARSE_SCAN_TILE 1024u             /* bricks of a tile of the allocation's prefix sum                              */

/* mipsf_sparse_raycast_args.flags */
#define MIPSF_SPARSE_NO_SKIP 1u                  /* a sample whose base brick is unallocated is evaluated like any other          */

/* The state of a volume is the caller's, all of it on the device:
 *   the virtual grid X, Y, Z: voxel (i,j,k) sits at origin + voxel*(i,j,k) in float64 (ticks[a][i], the three float64 tick arrays of
 *     mipsf_tsdf.h, hold exactly these values); bricks BX x BY x BZ = ceil(X/8) x ceil(Y/8) x ceil(Z/16), z fastest
 *   table      int32 [BX,BY,BZ]: the slot of a brick, or -1 (all -1 before the first call)
 *   slot_brick int32 [capacity]: the brick of a slot in use
 *   birth      uint32 [capacity]: the call's scratch; after mipsf_sparse_allocate the first view of THIS call a slot takes
 *   count      uint32 [1]: slots in use (0 before the first call); slots 0 .. count-1 are the ones in use
 *   tsdf, weight fp32 [capacity,8,8,16], optionally color fp32 [capacity,8,8,16,3]: voxel (i,j,k) of an allocated brick is word
 *     ((i%8)*8 + j%8)*16 + k%16 of its slot; all zero before the first call.  Words of a slot that lie outside the grid stay zero. */
typedef struct mipsf_sparse_volume {
    uint32_t X, Y, Z;
    uint32_t capacity;
    double origin[3], voxel;
    const double* ticks[3];             /* [X], [Y], [Z]                                                                       */
    int32_t* table;
    int32_t* slot_brick;
    uint32_t* birth;
    uint32_t* count;
    float* tsdf;
    float* weight;
    float* color;                       /* or null                                                                             */
} mipsf_sparse_volume;

typedef struct mipsf_sparse_alloc_record {
    uint64_t marked;                    /* bricks this call's views marked                                                     */
    uint64_t created;                   /* of those, bricks that had no slot and got one ("new")                               */
    uint64_t dropped;                   /* of those, bricks that had no slot and got none: the pool was full                   */
    uint64_t in_use;                    /* slots in use after the call                                                         */
} mipsf_sparse_alloc_record;

/* words of the `scan` scratch of mipsf_sparse_allocate for a virtual grid; 0: a side is 0 or the grid has more than
 * MIPSF_SPARSE_MAX_BRICKS bricks */
uint64_t mipsf_sparse_scan_words(uint32_t X, uint32_t Y, uint32_t Z);

/* mipsf_sparse_allocate: the bricks near the surfaces of n views get slots.  depth fp32 [n,H,W], poses fp32 [n,4,4] as in
 * mipsf_tsdf_integrate; steps = the host's ceil(band/voxel).  mark uint32 [BX,BY,BZ] is the call's scratch (set to 0xffffffff
 * first, by a kernel: a call is kernels only and replays from a captured graph).  Per view k and pixel (row, col), with d = (double)D[k][row][col] and usable = d > 0 && d < inf && d <= depth_max, for
 * j = -steps .. steps, in float64, parentheses give the order:
 *   z      = d + (double)j*voxel;  skipped unless z > 0
 *   p_c    = (z*((col - cx)/fx), -(z*((row - cy)/fy)), -z)
 *   p[r]   = ((R[r][0]*p_c.x + R[r][1]*p_c.y) + R[r][2]*p_c.z) + t[r]
 *   g[a]   = (p[a] - origin[a])/voxel;  i0[a] = floor(g[a])          (compared as doubles; a NaN fails every comparison, so a NaN
 *                                                                     pose marks nothing)
 *   each of the eight corners c[a] in {i0[a] - 1, i0[a] + 2} with 0 <= c[a] <= D_a - 1 on every axis marks the brick
 *   (c[0]/8, c[1]/8, c[2]/16):  mark = min(mark, k)
 * Then the marked bricks without a slot get the slots count, count + 1, .. in ascending brick index (a prefix sum over tiles of
 * MIPSF_SPARSE_SCAN_TILE bricks: tile sums, one block over the sums, the tiles again): table and slot_brick are written and
 * birth[slot] = mark, the first view that marked the brick; slots in use before the call have birth 0.  When the pool runs out the
 * first bricks in that order get the remaining slots and the rest stay unallocated (`dropped`); nothing is written beyond `capacity`
 * slots.  n = 0 marks nothing.
 * Refused on the host, with nothing launched: what mipsf_tsdf_integrate refuses of X, Y, Z (zero), H, W, the intrinsics and
 * depth_max; more than MIPSF_SPARSE_MAX_BRICKS bricks; capacity 0 or above MIPSF_SPARSE_MAX_CAPACITY; voxel not positive and finite,
 * an origin not finite; band negative, infinite or NaN; steps above MIPSF_SPARSE_MAX_STEPS; n above MIPSF_SPARSE_MAX_VIEWS; a null
 * pointer (depth and poses are not looked at when n is 0). */
typedef struct mipsf_sparse_allocate_args {
    uint32_t struct_size;
    uint32_t n, H, W;
    uint32_t steps;
    uint32_t reserved;
    double fx, fy, cx, cy, depth_max, band;
    mipsf_sparse_volume vol;
    const float* depth;                 /* [n,H,W]                                                                             */
    const float* poses;                 /* [n,4,4]                                                                             */
    uint32_t* mark;                     /* [BX,BY,BZ]                                                                          */
    uint32_t* scan;                     /* [mipsf_sparse_scan_words(X, Y, Z)]                                                  */
    mipsf_sparse_alloc_record* record;
} mipsf_sparse_allocate_args;

int mipsf_sparse_allocate(const mipsf_sparse_allocate_args* a, void* stream);

/* mipsf_sparse_integrate: the per-voxel rule of mipsf_tsdf_integrate, word for word (the projection, the running mean, the fp32
 * rounding after every view, max_weight), for every voxel of a brick with a slot and the views k >= birth[slot] of the call in
 * ascending order; voxel (i,j,k) sits at ((float)ticks[0][i], (float)ticks[1][j], (float)ticks[2][k]).  Because a brick takes the
 * views from the one that first marked it, cutting the views into (allocate, integrate) calls does not reach a byte of any brick as
 * long as nothing is dropped; only the numbering of the slots depends on the cut.  One workgroup per slot (`capacity` are launched;
 * those at or beyond `count` return); the per-brick view culling of tsdf.hip is restated and, as there, never leaves out a pair the
 * rule updates.  record: the two counts of mipsf_tsdf_integrate over the voxels of the slots in use.
 * Refused: what mipsf_tsdf_integrate refuses (the voxel limit aside), and what mipsf_sparse_allocate refuses of the volume. */
typedef struct mipsf_sparse_integrate_args {
    uint32_t struct_size;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_TSDF_NO_CULL                                                                  */
    uint32_t reserved;
    double fx, fy, cx, cy, trunc, depth_max, max_weight;
    mipsf_sparse_volume vol;
    const float* depth;                 /* [n,H,W]                                                                             */
    const float* rgb;                   /* [n,H,W,3] or null; there exactly when vol.color is                                  */
    const float* poses;                 /* [n,4,4]                                                                             */
    mipsf_tsdf_record* record;
} mipsf_sparse_integrate_args;

int mipsf_sparse_integrate(const mipsf_sparse_integrate_args* a, void* stream);

/* mipsf_sparse_gather: the window lo[a] <= index < hi[a] of the masked dense state as dense arrays tsdf, weight fp32
 * [hi-lo], color fp32 [hi-lo, 3] (when given), zeros where no brick is allocated: the input of mipsf_mesh_* and mipsf_tsdf_sample.
 * Refused: lo[a] >= hi[a] or hi[a] > D_a, a window above MIPSF_TSDF_MAX_VOXELS voxels, color without vol.color, a null pointer. */
typedef struct mipsf_sparse_gather_args {
    uint32_t struct_size;
    uint32_t lo[3], hi[3];
    uint32_t reserved;
    mipsf_sparse_volume vol;
    float* tsdf;
    float* weight;
    float* color;                       /* or null                                                                             */
} mipsf_sparse_gather_args;

int mipsf_sparse_gather(const mipsf_sparse_gather_args* a, void* stream);

/* mipsf_sparse_raycast: the rule of mipsf_track_raycast, word for word, over the masked dense state: D_a and the box are the
 * virtual grid's, a voxel of an unallocated brick has weight 0 and tsdf 0.  With min_weight > 0 a sample whose base voxel i0 lies in
 * an unallocated brick has a corner of weight 0 and is unknown: it costs one word of the table.  MIPSF_SPARSE_NO_SKIP looks at all
 * eight corners of such a sample too; the words are the same either way.  Outputs as mipsf_track_raycast; record.marked is 0 (there
 * is no marking pass: allocated bricks are walked sample by sample).  mipsf_track_register and mipsf_track_register_color take
 * these images.  Refused: what mipsf_track_raycast refuses (the voxel and brick limits aside, no workspace), and what
 * mipsf_sparse_allocate refuses of the volume. */
typedef struct mipsf_sparse_raycast_args {
    uint32_t struct_size;
    uint32_t n, H, W;
    uint32_t flags;                     /* MIPSF_SPARSE_NO_SKIP                                                                */
    uint32_t reserved;
    double trunc, fx, fy, cx, cy, near, far, step, min_weight;
    mipsf_sparse_volume vol;
    const float* poses;                 /* [n,4,4]                                                                             */
    float* depth;                       /* [n,H,W]                                                                             */
    float* normals;                     /* [n,H,W,3] or null                                                                   */
    float* color_out;                   /* [n,H,W,3] or null                                                                   */
    mipsf_track_record* record;
} mipsf_sparse_raycast_args;

int mipsf_sparse_raycast(const mipsf_sparse_raycast_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SPARSE_H */
