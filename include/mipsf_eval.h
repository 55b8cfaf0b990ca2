/*
 * mipsf_eval.h -- scoring a mesh against ground truth the way the NICE-SLAM / Co-SLAM evaluation does: area-uniform samples
 * of each mesh, the distance of every sample to the nearest sample of the other mesh, means and the share below a threshold
 * (accuracy, completion, completion ratio).  DESIGN.md 4.17; mipsfusion_amd/evaluate.py.
 *
 * Same conventions as mipsf_icp.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Workspaces are
 * the caller's; mipsf_eval_workspace_bytes() gives their sizes.  Nothing here uses a floating-point atomic; the same call gives
 * the same bytes.  Every floating-point operation named below is one IEEE float64 operation rounded on its own (no
 * contraction), so a float64 restatement on the host (tests/eval_cpu.py) gives the same words.
 */
#ifndef MIPSF_EVAL_H
#define MIPSF_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_EVAL_MAX_FACES (1u << 30)
#define MIPSF_EVAL_MAX_SAMPLES (1u << 27)        /* = MIPSF_ICP_MAX_POINTS: the samples are binned by mipsf_icp_bin           */
#define MIPSF_EVAL_AREA_UNIT_LOG2 (-40)          /* areas are counted in units of 2^-40 m^2                                    */

/* mipsf_eval_workspace_bytes(which, n): bytes of a workspace; 0 = out of range */
#define MIPSF_EVAL_WS_SAMPLE 1                   /* mipsf_eval_sample for a mesh of n faces                                    */
#define MIPSF_EVAL_WS_STATS 2                    /* mipsf_eval_stats for n distances                                           */
uint64_t mipsf_eval_workspace_bytes(int which, uint32_t n);

/* status word of mipsf_eval_sample_record */
#define MIPSF_EVAL_OK 0u
#define MIPSF_EVAL_NO_AREA 1u                    /* every face has area 0: nothing was drawn                                   */
#define MIPSF_EVAL_AREA_OVERFLOW 2u              /* the total is 2^63 units (2^23 m^2) or more: nothing was drawn              */

typedef struct mipsf_eval_sample_record {
    double area;                                 /* (double)total_units * 2^-40                                                */
    uint64_t total_units;                        /* sum of the faces' units (wraps when status is AREA_OVERFLOW)                */
    uint32_t status;
    uint32_t reserved[3];
} mipsf_eval_sample_record;

/* n area-uniform, stratified, reproducible samples of a triangle mesh.
 *   area of face f   A, B, C = its vertices widened to float64; e1 = B - A, e2 = C - A;
 *                    c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x);
 *                    area = 0.5 * sqrt((c.x*c.x + c.y*c.y) + c.z*c.z); a face with an index outside [0, V) or an area that is
 *                    not finite counts as area 0
 *   units of face f  t = area * 2^40; t >= 2^63 ? 2^63 : (uint64)floor(t)
 *   cum[f]           the inclusive prefix sum of the units (integers: the same in any order); total = cum[F-1]
 *   word(k, which)   h = seed*0x9e3779b9 + k*3 + which; h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b;
 *                    h ^= h >> 16 (uint32 arithmetic); u = (h >> 8) * 2^-24
 *   sample k         u0, u1, u2 = word(k, 0..2); pos = min((uint64)((((double)k + u0) / (double)n) * (double)total), total - 1);
 *                    face_of[k] = the first f with cum[f] > pos (never a face of area 0);
 *                    r = sqrt(u1); a = 1 - r; b = r * (1 - u2); c = r * u2;
 *                    points[k][d] = (float)((a*A[d] + b*B[d]) + c*C[d])
 * Returns an error, and launches nothing, for F = 0.  A mesh without area or with too much of it is found on the device: the
 * record's status says so and the drawing kernel returns without writing points or face_of. */
typedef struct mipsf_eval_sample_args {
    uint32_t struct_size;
    uint32_t V, F, n, seed;
    const float* vertices;              /* [V,3]                                                                           */
    const int32_t* faces;               /* [F,3]                                                                           */
    float* points;                      /* [n,3]                                                                           */
    int32_t* face_of;                   /* [n]                                                                             */
    mipsf_eval_sample_record* record;   /* [1]                                                                             */
    void* workspace;                    /* MIPSF_EVAL_WS_SAMPLE bytes for F, 16-byte aligned                                */
} mipsf_eval_sample_args;

int mipsf_eval_sample(const mipsf_eval_sample_args* a, void* stream);

/* index[i] = the original index of the target point nearest to source point i, d2[i] = its squared distance: the float64 value
 * and the (distance, index) order of mipsf_icp.h, whatever the distance is.  The grid is one mipsf_icp_bin made of the target,
 * with any edge; no result depends on it.  -1 and inf when the target is empty or the source point has a coordinate that is not
 * finite.  The walk visits O(R^3) cells for a point R cells away from its nearest target point. */
typedef struct mipsf_eval_nearest_args {
    uint32_t struct_size;
    uint32_t n_source, n_target, max_cells;
    const float* source;                /* [n_source,3]                                                                    */
    const void* grid;                   /* of the target: MIPSF_ICP_WS_GRID bytes for (n_target, max_cells)                  */
    int32_t* index;                     /* [n_source]                                                                      */
    double* d2;                         /* [n_source]                                                                      */
} mipsf_eval_nearest_args;

int mipsf_eval_nearest(const mipsf_eval_nearest_args* a, void* stream);

/* Squared distances [n] -> one record.  Entries that are not finite (inf, NaN) are counted out: they enter neither the sums,
 * nor the maximum, nor `within`.  The sums are added in a fixed two-stage order (lane -> wave -> block partial; one finishing
 * wave), `within` counts d2 <= threshold*threshold (the product formed once, in float64, on the host). */
typedef struct mipsf_eval_stats_record {
    double sum_d;                       /* sum of sqrt(d2)                                                                 */
    double sum_d2;
    double max_d2;                      /* 0 when no entry is finite                                                       */
    uint64_t within;
    uint64_t finite;
    uint64_t reserved[3];
} mipsf_eval_stats_record;

typedef struct mipsf_eval_stats_args {
    uint32_t struct_size;
    uint32_t n;
    const double* d2;                   /* [n]                                                                             */
    double threshold;
    mipsf_eval_stats_record* record;    /* [1]                                                                             */
    void* workspace;                    /* MIPSF_EVAL_WS_STATS bytes for n, 16-byte aligned                                 */
} mipsf_eval_stats_args;

int mipsf_eval_stats(const mipsf_eval_stats_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_EVAL_H */
