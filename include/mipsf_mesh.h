/*
 * mipsf_mesh.h -- the mesh extractor of libmipsf_hip.so: marching cubes on a device-resident SDF volume with the semantics of
 * the upstream extractor (external/NumpyMarchingCubes, called from utils/utils.py: extract_mesh / extract_mesh2).
 *
 * Same conventions as mipsf.h (which this header extends; it is a header of its own because mipsf.h is held to 45 entry
 * points): int return code, message through mipsf_last_error(), one argument block per entry point with `struct_size`
 * first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Sizes of the buffers the
 * caller provides come from mipsf_buffer_size(MIPSF_SIZE_MCUBES_*, ...).
 *
 * The call sequence:
 *   mipsf_mcubes_count  volume -> one case byte per cell (0 = emits nothing) and the exclusive triangle offset of every block
 *                       of MIPSF_MCUBES_BLOCK_CELLS cells; block_offsets[n_blocks] is the triangle count T
 *   (the caller reads T and provides soup [T,3,3])
 *   mipsf_mcubes_emit   -> the triangle soup in cell order (i, j, k), k fastest, table order within a cell
 *   mipsf_mcubes_weld   soup -> vertices welded on the 1e-5 grid and numbered by first appearance, faces [T,3] as vertex numbers
 * Faces with a repeated vertex and repeated faces are still in `faces`; dropping them is index plumbing left to the caller.
 *
 * Semantics: the DUAL grid is marched.  The corner of cell (i,j,k) at offset (dx,dy,dz) has the value
 * sum of 0.125f * volume[i-1+dx+a][j-1+dy+b][k-1+dz+c] over (a,b,c) in the order 000 100 010 001 110 011 101 111, and is
 * invalid when one of the eight voxels is -inf, has |d| >= truncation or lies outside the volume.  A cell with an invalid
 * corner emits nothing, so cells 1..X-2 can emit and vertices lie in [0.5, X-1.5] (voxel units).
 */
#ifndef MIPSF_MESH_H
#define MIPSF_MESH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cells per block of the triangle-offset table (a block = 256 threads x 16 consecutive cells in C order) */
#define MIPSF_MCUBES_BLOCK_CELLS 4096u
/* the per-cell rejection threshold of the upstream extractor (dead for truncation <= 5) */
#define MIPSF_MCUBES_THRESH 10.0f
/* weld grid: vertices whose quantised cells trunc(v / 1e-5 + 0.5 sgn v) are equal or adjacent are one vertex */
#define MIPSF_MCUBES_WELD_GRID 0.00001f

/* mipsf_buffer_size() ids: n = X, a = Y, b = Z for the first, n = T (triangles) for the other two */
#define MIPSF_SIZE_MCUBES_OFFSET_WORDS 20   /* uint32 words of block_offsets (n_blocks + 1)                       */
#define MIPSF_SIZE_MCUBES_WELD_SLOTS 21     /* slots of the weld hash table: a power of two >= 6 T                  */
#define MIPSF_SIZE_MCUBES_WELD_WORDS 22     /* uint32 words of the weld scratch (table + three words per soup vertex) */

typedef struct mipsf_mcubes_args {
    uint32_t struct_size;
    uint32_t X, Y, Z;               /* volume [X,Y,Z], C order; X*Y*Z < 2^31                                        */
    float isovalue, truncation;
    const float* volume;
    uint8_t* cases;                 /* [X*Y*Z] own corner numbering (bit 4dx+2dy+dz set when value < isovalue); 0 = nothing */
    uint32_t* block_offsets;        /* [MIPSF_SIZE_MCUBES_OFFSET_WORDS]                                              */
    /* mipsf_mcubes_emit only */
    float* soup;                    /* [capacity_tris,3,3]                                                           */
    int32_t* cell_ids;              /* optional [capacity_tris]: (i*Y + j)*Z + k of the cell a triangle came from     */
    uint32_t capacity_tris;         /* triangles beyond it are not written (pass T read from block_offsets)           */
} mipsf_mcubes_args;

int mipsf_mcubes_count(const mipsf_mcubes_args* a, void* stream);
int mipsf_mcubes_emit(const mipsf_mcubes_args* a, void* stream);

typedef struct mipsf_mcubes_weld_args {
    uint32_t struct_size;
    uint32_t T;                     /* triangles of the soup; 3T soup vertices, coordinates >= 0                      */
    const float* soup;              /* [T,3,3]                                                                       */
    uint32_t* scratch;              /* [MIPSF_SIZE_MCUBES_WELD_WORDS], 8-byte aligned                                 */
    float* vertices;                /* [3T,3] capacity; the first counts[0] rows are written                          */
    int32_t* faces;                 /* [T,3]                                                                         */
    uint32_t* counts;               /* [4]: V, rounds in which a label still moved (== max_rounds: not converged,     */
                                    /* call again with more), soup vertices that could not be placed (must be 0), 0   */
    uint32_t max_rounds;            /* label-propagation rounds; 2 suffice when every cluster is a clique             */
} mipsf_mcubes_weld_args;

int mipsf_mcubes_weld(const mipsf_mcubes_weld_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_MESH_H */
