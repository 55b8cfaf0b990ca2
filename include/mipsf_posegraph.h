/*
 * mipsf_posegraph.h -- closing a loop: Levenberg-Marquardt over the first-keyframe ("anchor") poses of all sub-maps (upstream:
 * PoseCorrector.py pose_graph_optimize + model/poseGraph.py, run through pypose's LM / Cholesky / TrustRegion / StopOnPlateau on
 * the host).  DESIGN.md 4.15 states what is computed; tests/posegraph_cpu.py restates it in numpy.
 *
 * Same conventions as mipsf.h and mipsf_icp.h: int return code, message through mipsf_last_error(), one argument block with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation; the workspace is
 * the caller's.  ONE EXCEPTION to "refused with a message": the edge table is on the device and the call reads nothing back, so
 * an edge with a == b or an index outside [0, n_nodes) cannot be refused on the host.  The call then returns 0,
 * mipsf_last_error() stays empty, and the refusal is MIPSF_POSEGRAPH_BAD_EDGE in result[6]: nothing was optimised.  A caller
 * that has the edges on the host checks them before the upload (mipsfusion_amd/pose_graph.py: check_graph).  ONE launch of one workgroup runs the whole optimisation -- projection, every step, every rejection, the stop --
 * so the call can sit between captured graphs or inside one.  All arithmetic is float64; nothing uses a floating-point atomic and
 * every sum has a fixed order: the same call gives the same bytes.
 */
#ifndef MIPSF_POSEGRAPH_H
#define MIPSF_POSEGRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_POSEGRAPH_MAX_NODES 64u
#define MIPSF_POSEGRAPH_MAX_EDGES 1024u
#define MIPSF_POSEGRAPH_LDS_NODES 20u      /* up to here the packed triangle of J^T J lives in LDS, above in the workspace     */
#define MIPSF_POSEGRAPH_RESULT_DOUBLES 8u  /* first loss, last loss, steps done, solves, rejections, final radius, status, 0   */

/* status bits of result[6] */
#define MIPSF_POSEGRAPH_FACTORISATION_FAILED 1u /* a Cholesky pivot was not positive and finite, or the solved step was not
                                                   finite: that step ended without an update                                    */
#define MIPSF_POSEGRAPH_NAN_QUALITY 2u          /* a step's quality was 0/0 (an exact fixed point); it shrank the radius        */
#define MIPSF_POSEGRAPH_BAD_EDGE 4u             /* an edge with a == b or an index outside [0, n_nodes): nothing was optimised,
                                                   the anchors come back as projected                                           */

/* bytes of the workspace for a graph of that size; 0 = out of range */
uint64_t mipsf_posegraph_workspace_bytes(uint32_t n_nodes, uint32_t n_edges);

/* Nodes X_0..X_{N-1} (camera -> world, X_0 is never updated), edges (a, b) with observation P and weight w, residual
 * r = w * Log(P X_a^-1 X_b) in R^6 (translation first), loss = sum r^2.  Rotations of anchors and observations are first
 * projected through their unit quaternion. */
typedef struct mipsf_posegraph_args {
    uint32_t struct_size;
    uint32_t n_nodes, n_edges;          /* 2 .. MIPSF_POSEGRAPH_MAX_NODES, 1 .. MIPSF_POSEGRAPH_MAX_EDGES                      */
    uint32_t input_f64;                 /* 0: anchors and observations are float32, 1: float64                                */
    const void* anchors;                /* [n_nodes,4,4] row major                                                            */
    const int32_t* edges;               /* [n_edges,2]                                                                        */
    const void* observations;           /* [n_edges,4,4]                                                                      */
    const double* weights;              /* [n_edges]                                                                          */
    uint32_t steps, patience, max_rejects, reserved;
    double decreasing, radius, min_diag;
    double* anchors_out;                /* [n_nodes,4,4] float64                                                              */
    float* anchors_out32;               /* [n_nodes,4,4] the same, rounded                                                    */
    double* result;                     /* MIPSF_POSEGRAPH_RESULT_DOUBLES                                                     */
    void* workspace;                    /* mipsf_posegraph_workspace_bytes(n_nodes, n_edges), 16-byte aligned                 */
} mipsf_posegraph_args;

int mipsf_posegraph_optimize(const mipsf_posegraph_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_POSEGRAPH_H */
