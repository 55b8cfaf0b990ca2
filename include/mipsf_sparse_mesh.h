/*
 * mipsf_sparse_mesh.h -- the mesh of a brick-sparse volume (mipsf_sparse.h) marched brick by brick: no dense window is formed, and the
 * virtual grid may hold 2^31 voxels and more in one call.  DESIGN.md 4.25; mipsfusion_amd/sparse_tsdf.py: extract_mesh_bricks.
 *
 * Same conventions as mipsf_sparse.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation; sizes of the caller's
 * buffers come from mipsf_sparse_mesh_scan_words() and mipsf_buffer_size(MIPSF_SIZE_MCUBES_WELD_WORDS, T); every refusal happens on
 * the host with a message and nothing launched.  No floating-point atomic; no atomic decides an order.
 *
 * The rule.  The marching volume M[i,j,k] over the virtual grid is tsdf where the voxel's brick has a slot and weight >= min_weight
 * (compared in fp32), and -inf everywhere else: unallocated brick, low weight, outside the grid, the words of a slot past the grid's
 * edge.  Isovalue 0, truncation 1, as TSDFVolume.extract_mesh.  Cell (i,j,k) of the dual grid (mipsf_mesh.h) reads voxels i-1 .. i+1
 * on each axis and always its own voxel, so a cell whose own brick is unallocated emits nothing and every emitting cell belongs to
 * exactly one allocated brick.  For the brick b = (bx,by,bz) of a slot in use, base = (8bx-1, 8by-1, 16bz-1) (never clipped, may be
 * -1) and the block B = M[base .. base + (10,10,18)) is the brick plus one voxel on every side.  The soup of the brick is the soup of
 * mipsf_mcubes_count / _emit on B, word for word (dual sums in their order, the `thresh` rejections, the patterns that emit nothing,
 * the snaps, p1 + mu (p2 - p1) in fp32 without contraction, table order within a cell, cells in (i,j,k) order, k fastest): the cells
 * 1..8, 1..8, 1..16 of the block are the brick's own, every other cell of the block has an invalid corner.  Vertices are BLOCK-LOCAL
 * fp32 (a brick's cells give coordinates in [0.5, 8.5] x [0.5, 8.5] x [0.5, 16.5]); the whole soup is the concatenation over the
 * slots 0 .. count-1 in slot order.
 *
 * The weld is the relation of mipsf_mcubes_weld on the GLOBAL 1e-5 grid: soup vertex v of a triangle of brick b has the integer cell
 * q[a] = base[a]*100000 + trunc(v[a]/1e-5f + 0.5f) (the second term is the dense weld's quantisation of the local coordinate);
 * vertices whose cells are equal or adjacent on every axis are one vertex (connected components, by rounds to a fixed point with the
 * caller's retry); the first in soup order survives, numbering by first appearance.  The fixed coordinates of a vertex are exact
 * half-integers and the running coordinate has the same base in every brick that shares the edge, so two bricks give a shared vertex
 * the same q.  A surviving vertex is written in index units of the virtual grid as float64: (double)base + (double)v, which is exact.
 *
 * q IS KEPT IN 32 BITS: mipsf_sparse_mesh_weld refuses a virtual grid with a side above MIPSF_SPARSE_MESH_MAX_SIDE voxels (the
 * largest q is below (side - 1.5) * 100000 < 2^31 then).  Count, emit and sample take any grid the sparse volume takes.
 */
#ifndef MIPSF_SPARSE_MESH_H
#define MIPSF_SPARSE_MESH_H

#include <stdint.h>

#include "mipsf_mesh.h"
#include "mipsf_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_SPARSE_MESH_MAX_SIDE 21474u        /* voxels a side of the virtual grid in mipsf_sparse_mesh_weld                    */
#define MIPSF_SPARSE_MESH_SCAN_TILE 1024u        /* slots of a tile of the prefix sum over the slots' triangle counts               */

/* uint32 words of the `scan` scratch of mipsf_sparse_mesh_count for a pool of `capacity` slots (8-byte aligned); 0: capacity is 0 or
 * above MIPSF_SPARSE_MAX_CAPACITY */
uint64_t mipsf_sparse_mesh_scan_words(uint32_t capacity);

/* One block for count and emit.
 * mipsf_sparse_mesh_count: one workgroup per slot (`capacity` are launched; those at or beyond `count` return, `count` is not read
 *   back).  A workgroup reads the 27 table words of the brick's neighbourhood once, stages the block in LDS with invalid voxels as
 *   NaN, then the 9 x 9 x 17 dual values, and writes one case byte per cell, cases[slot][cell] with cell = ((i%8)*8 + j%8)*16 + k%16
 *   (own corner numbering as mipsf_mcubes_args.cases; 0 = emits nothing), and the slot's triangle count.  A prefix sum over the slots
 *   (tile sums, one block over the sums, the tiles again) leaves offsets[s] = triangles of the slots before s for s < capacity (slots
 *   at or beyond `count` hold none) and offsets[capacity] = T, 0xffffffff when the soup has 2^32 triangles or more.
 * mipsf_sparse_mesh_emit: per slot, the triangles go to offsets[slot] .. in the order above: soup (block-local), tri_slot, and
 *   optionally cell_ids, the cell within the brick.  Triangles at or beyond capacity_tris are not written; the host refuses
 *   capacity_tris == 0 with nothing to do (returns 0) and cannot see T, so the caller passes the T it read.
 * Refused: what mipsf_sparse_allocate refuses of the volume, a min_weight that is not a number, a null pointer, cases or scan not
 * 8-byte aligned. */
typedef struct mipsf_sparse_mesh_args {
    uint32_t struct_size;
    float min_weight;
    mipsf_sparse_volume vol;
    uint8_t* cases;                     /* [capacity,1024]                                                                     */
    uint32_t* offsets;                  /* [capacity + 1]                                                                      */
    uint32_t* scan;                     /* [mipsf_sparse_mesh_scan_words(capacity)]; count only                                */
    /* mipsf_sparse_mesh_emit only */
    float* soup;                        /* [capacity_tris,3,3]                                                                 */
    int32_t* tri_slot;                  /* [capacity_tris]                                                                     */
    int32_t* cell_ids;                  /* optional [capacity_tris]                                                            */
    uint32_t capacity_tris;
    uint32_t reserved;
} mipsf_sparse_mesh_args;

int mipsf_sparse_mesh_count(const mipsf_sparse_mesh_args* a, void* stream);
int mipsf_sparse_mesh_emit(const mipsf_sparse_mesh_args* a, void* stream);

/* mipsf_sparse_mesh_weld: the weld of mipsf_mcubes_weld over the cells q above; scratch, faces, counts and max_rounds are that entry
 * point's (scratch: mipsf_buffer_size(MIPSF_SIZE_MCUBES_WELD_WORDS, T) words).  vertices float64 [3T,3] capacity, index units of the
 * virtual grid; the first counts[0] rows are written.  A soup vertex whose tri_slot is not a slot of the pool, or whose q is negative,
 * counts as unplaced (counts[2], must be 0).
 * Refused: what mipsf_sparse_allocate refuses of the volume; a side above MIPSF_SPARSE_MESH_MAX_SIDE, named in the message; a T beyond
 * what the weld table can hold, capacity_tris below T, max_rounds outside 1..64, a null pointer, a scratch not 8-byte aligned. */
typedef struct mipsf_sparse_mesh_weld_args {
    uint32_t struct_size;
    uint32_t T;                         /* triangles of the soup                                                               */
    uint32_t capacity_tris;             /* triangles soup, tri_slot and faces have room for, 3 * capacity_tris rows of vertices */
    uint32_t max_rounds;
    mipsf_sparse_volume vol;
    const float* soup;                  /* [T,3,3] block-local                                                                 */
    const int32_t* tri_slot;            /* [T]                                                                                 */
    uint32_t* scratch;
    double* vertices;                   /* [3T,3]                                                                              */
    int32_t* faces;                     /* [T,3]                                                                               */
    uint32_t* counts;                   /* [4] as mipsf_mcubes_weld                                                            */
} mipsf_sparse_mesh_weld_args;

int mipsf_sparse_mesh_weld(const mipsf_sparse_mesh_weld_args* a, void* stream);

/* mipsf_sparse_sample: the colour of m points given in index units of the virtual grid, by the rule of mipsf_tsdf_sample, word for
 * word, over the masked dense state: corners are read through the table, a corner of an unallocated brick has weight 0.
 * points float64 [m,3] -> out fp32 [m,3].  Refused: what mipsf_sparse_allocate refuses of the volume, a volume without colour, a null
 * pointer with m > 0. */
typedef struct mipsf_sparse_sample_args {
    uint32_t struct_size;
    uint32_t m;
    mipsf_sparse_volume vol;
    const double* points;
    float* out;
} mipsf_sparse_sample_args;

int mipsf_sparse_sample(const mipsf_sparse_sample_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SPARSE_MESH_H */
