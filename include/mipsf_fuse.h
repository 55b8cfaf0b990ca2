/*
 * mipsf_fuse.h -- the scene as one mesh: visibility of points from keyframes, fusion of the sub-maps' SDFs on one grid, and
 * labelling of the connected components of a mesh (upstream: model/Mesher.py extract_mesh_jointly, vis/math_helper.py).
 *
 * Same conventions as mipsf.h and mipsf_mesh.h (a header of its own because mipsf.h is held to 45 entry points): int return
 * code, message through mipsf_last_error(), one argument block per entry point with `struct_size` first, DEVICE pointers,
 * everything enqueued on `stream`, no allocation and no synchronisation.
 *
 * Points are described in one of two ways (mipsf_fuse_points):
 *   a list    points fp32 [n,3];
 *   a grid    three float64 tick arrays and an index sub-box lo[3], size[3]: item q in 0 .. size[0]*size[1]*size[2] stands for
 *             the grid point (lo[0] + ix, lo[1] + iy, lo[2] + iz) with q = (ix*size[1] + iy)*size[2] + iz, at the world
 *             position (float)ticks[axis][index] (the upstream builds the grid in float64 and narrows it to fp32).  Its row in
 *             a per-voxel array of the whole grid is (gx*dims[1] + gy)*dims[2] + gz.  Grid points are never stored.
 * A call covers the items first .. first + n - 1 (chunks of a sub-box), item `first + p` uses row p of the per-call arrays.
 *
 * The visibility test (Mesher.py:247-281), fp32, no contraction: with a keyframe record (R 3x3 and t of world->camera, and
 * max_depth), c = (x*r0 + y*r1 + z*r2) + t per row, den = c.z + 1e-5f, u = (fx*(-c.x) + cx*c.z) / den,
 * v = (fy*c.y + cy*c.z) / den; seen by it when edge < u < W - edge, edge < v < H - edge, c.z < 0, 0 < |c.z| < max_depth.
 * A point is seen when one keyframe sees it.
 *
 * The fusion (Mesher.py:456-527): per voxel num, den (fp32) and flag bits.  For every sub-map in turn, over its sub-box,
 *   w = expf(-10 clip(entropy, 0, 1e4)) * gauss_k * expf(-0.5 (dist/sigma)^2),   dist = |p - centroid| (fp32),
 *   num += w * value, den += w   where the point is inside the oriented box AND seen by one of THIS sub-map's keyframes.
 * Every voxel is owned by one lane and sub-maps follow each other on the stream: no float atomics, bit-reproducible.
 */
#ifndef MIPSF_FUSE_H
#define MIPSF_FUSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_FUSE_KF_FLOATS 16u        /* one keyframe record: r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2 max_depth 0 0 0 */
#define MIPSF_FUSE_IN_BOX 1u            /* flag bit: the voxel lies in some sub-map's axis-aligned box                      */
#define MIPSF_FUSE_SEEN 2u              /* flag bit: inside some sub-map's oriented box and seen by one of ITS keyframes     */

typedef struct mipsf_fuse_points {
    const float* points;                /* list: fp32 [>= first + n, 3]; NULL = the grid description below                 */
    const double* ticks[3];             /* grid: the tick arrays of the whole grid                                         */
    uint32_t dims[3];                   /* grid: ticks per axis; dims[0]*dims[1]*dims[2] < 2^31                             */
    uint32_t lo[3], size[3];            /* grid: the index sub-box, lo + size <= dims                                       */
    uint32_t first, n;                  /* items first .. first + n - 1 of the list / the sub-box                           */
} mipsf_fuse_points;

typedef struct mipsf_fuse_camera {
    float fx, fy, cx, cy;
    float W, H, edge;
    uint32_t k;                         /* keyframes                                                                       */
    const float* keyframes;             /* [k, MIPSF_FUSE_KF_FLOATS], 64-byte aligned                                       */
} mipsf_fuse_camera;

typedef struct mipsf_fuse_visibility_args {
    uint32_t struct_size;
    mipsf_fuse_points pts;
    mipsf_fuse_camera cam;
    uint8_t* seen;                      /* [n] 0 / 1                                                                       */
} mipsf_fuse_visibility_args;

int mipsf_fuse_visibility(const mipsf_fuse_visibility_args* a, void* stream);

/* normalised local coordinates of the items, float64 [n,3]: local = (x*r0 + y*r1 + z*r2) + t in fp32 with the fp32
 * world->local transform w2l (3x4, row major, passed by value), then ((double)local - sub) / div  (Mesher.py:476-484: the
 * upstream's bounding box is a float64 tensor, so the normalisation promotes). */
typedef struct mipsf_fuse_local_args {
    uint32_t struct_size;
    mipsf_fuse_points pts;
    float w2l[12];
    double sub[3], div[3];
    double* out;                        /* [n,3]                                                                           */
} mipsf_fuse_local_args;

int mipsf_fuse_local_points(const mipsf_fuse_local_args* a, void* stream);

typedef struct mipsf_fuse_accumulate_args {
    uint32_t struct_size;
    mipsf_fuse_points pts;
    mipsf_fuse_camera cam;              /* THIS sub-map's keyframes                                                         */
    const int32_t* rows;                /* list only, optional [n]: the state row of item first + p (NULL: first + p)        */
    uint32_t n_rows;                    /* rows of the state arrays; an item whose row is not below it is left out           */
    uint32_t channels;                  /* 1 (SDF) or 3 (colour)                                                            */
    uint32_t sigmoid;                   /* 1: value = 1 / (1 + expf(-raw))                                                   */
    const float* values;                /* value c of row p at values[p*value_stride + c]                                    */
    const float* entropy;               /* entropy of row p at entropy[p*entropy_stride]                                     */
    uint32_t value_stride, entropy_stride;
    uint32_t use_obb;                   /* 1: the point must satisfy |(p - centre) . axis_i| <= half[i] (float64)            */
    double obb_centre[3], obb_axes[9] /* axis i = column i: obb_axes[3*r + i] */, obb_half[3];
    float centroid[3];
    float sigma, gauss_k;               /* max_dist / 3 and 1 / (sigma sqrt(2 pi)), rounded to fp32 by the caller            */
    float* num;                         /* [rows, channels]                                                                 */
    float* den;                         /* [rows]                                                                           */
    uint8_t* flags;                     /* [rows] MIPSF_FUSE_* bits                                                          */
} mipsf_fuse_accumulate_args;

int mipsf_fuse_accumulate(const mipsf_fuse_accumulate_args* a, void* stream);

/* out[r,c] = den[r] > 0 ? num[r,c] / den[r] : 0.  With `flags`: a row without MIPSF_FUSE_SEEN gives -1 in `out`, and `volume`
 * (optional, channels == 1) holds `out` where both bits are set and -inf elsewhere: the marching-cubes input
 * (mipsf_mesh.h: an -inf voxel switches its cells off). */
typedef struct mipsf_fuse_finalize_args {
    uint32_t struct_size;
    uint32_t n, channels;
    const float* num;
    const float* den;
    const uint8_t* flags;               /* optional                                                                        */
    float* out;                         /* [n, channels]; may be NULL when `volume` is given                                */
    float* volume;                      /* optional [n]                                                                    */
} mipsf_fuse_finalize_args;

int mipsf_fuse_finalize(const mipsf_fuse_finalize_args* a, void* stream);

/* Connected components of F items joined by E pairs (faces that share an edge): labels[i] = the smallest item of i's
 * component.  Hooking on roots + pointer jumping, `max_rounds` rounds enqueued; counts[1] = rounds in which a label still moved
 * (== max_rounds: possibly not converged, call again with resume = 1, which keeps `labels`). */
typedef struct mipsf_fuse_label_args {
    uint32_t struct_size;
    uint32_t F, E;
    const int32_t* pairs;               /* [E,2]                                                                           */
    int32_t* labels;                    /* [F]                                                                             */
    uint32_t* counts;                   /* [4]: 0, moved rounds, scratch, 0                                                  */
    uint32_t max_rounds, resume;
} mipsf_fuse_label_args;

int mipsf_fuse_label_components(const mipsf_fuse_label_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_FUSE_H */
