/*
 * mipsf_icp.h -- rectifying the pose of a switch back to an earlier sub-map: point clouds from ray rows, a uniform grid over a
 * cloud, exact nearest neighbours, normals from the 30 nearest neighbours, and point-to-plane ICP (upstream: PoseCorrector.py
 * switch_pose_rectifying, which calls open3d's estimate_normals() and registration_icp()).  DESIGN.md 4.14.
 *
 * Same conventions as mipsf.h, mipsf_mesh.h and mipsf_fuse.h: int return code, message through mipsf_last_error(), one argument
 * block per entry point with `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no
 * synchronisation.  Workspaces are the caller's; mipsf_icp_workspace_bytes() gives their sizes.  Coordinates must be finite.
 *
 * Every distance is the float64 value ((dx*dx + dy*dy) + dz*dz) of the float64-widened coordinates (no contraction), and
 * candidates are ordered by (that value, original index): the neighbour sets equal those of a float64 computation on the host.
 * Nothing here uses a floating-point atomic; the same call gives the same bytes.
 */
#ifndef MIPSF_ICP_H
#define MIPSF_ICP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_ICP_KNN 30u               /* neighbours of a normal (open3d's default KDTreeSearchParamKNN), the point included  */
#define MIPSF_ICP_RESULT_DOUBLES 20u    /* result block: T[16] row major, correspondences, fitness, inlier rmse, iterations   */
#define MIPSF_ICP_MAX_POINTS (1u << 27)
#define MIPSF_ICP_MAX_CELLS (1u << 26)

/* mipsf_icp_workspace_bytes(which, n, cells): bytes of a workspace; 0 = out of range */
#define MIPSF_ICP_WS_CLOUD 1            /* mipsf_icp_cloud for n rows                                                          */
#define MIPSF_ICP_WS_GRID 2             /* a grid over n points with at most `cells` cells                                     */
#define MIPSF_ICP_WS_REGISTER 3         /* mipsf_icp_register for n source points                                              */
uint64_t mipsf_icp_workspace_bytes(int which, uint32_t n, uint32_t cells);

/* Points of ray rows (PoseCorrector.py:42-56, 70-87).  rows [n,7] = direction 3, rgb 3, depth 1; row i belongs to pose
 * owner[i], or to pose i / rows_per_owner when owner is NULL.  fp32, no contraction:
 *   d_w[r] = (d.x*R[r][0] + d.y*R[r][1]) + d.z*R[r][2],   p[r] = t[r] + d_w[r]*depth.
 * Rows with depth > 0 (and an owner below k) are kept in their original order; *count = how many. */
typedef struct mipsf_icp_cloud_args {
    uint32_t struct_size;
    uint32_t n, k, rows_per_owner;
    const float* rows;                  /* [n,7]                                                                           */
    const int32_t* owner;               /* optional [n]                                                                    */
    const float* poses;                 /* [k,4,4] camera -> world                                                         */
    float* points;                      /* [n,3]; the first *count rows are written                                         */
    uint32_t* count;                    /* [1]                                                                             */
    void* workspace;                    /* MIPSF_ICP_WS_CLOUD bytes, 16-byte aligned                                        */
} mipsf_icp_cloud_args;

int mipsf_icp_cloud(const mipsf_icp_cloud_args* a, void* stream);

/* Sort a cloud into a uniform grid over its bounding box (counting sort; the original indices are kept).  The cell edge is
 * min_edge when that is positive, else chosen from the cloud's density (about 8 points per occupied cell of a surface); it grows
 * by steps of 1.25 until the grid has at most max_cells cells.  No result of a search depends on the edge. */
typedef struct mipsf_icp_bin_args {
    uint32_t struct_size;
    uint32_t n, max_cells;
    const float* points;                /* [n,3]                                                                           */
    double min_edge;
    void* grid;                         /* MIPSF_ICP_WS_GRID bytes for (n, max_cells), 16-byte aligned                      */
} mipsf_icp_bin_args;

int mipsf_icp_bin(const mipsf_icp_bin_args* a, void* stream);

/* partner[i] = the original index of the target point nearest to source point i when its squared distance is <=
 * max_dist*max_dist, else -1.  The grid must have been binned with min_edge >= max_dist * (1 + 1e-6).  A source point outside
 * the grid's box is clamped for the cell look-up only. */
typedef struct mipsf_icp_nearest_args {
    uint32_t struct_size;
    uint32_t n_source, n_target, max_cells;
    const float* source;                /* [n_source,3]                                                                    */
    const void* grid;                   /* of the target                                                                   */
    double max_dist;
    int32_t* partner;                   /* [n_source]                                                                      */
    double* d2;                         /* optional [n_source]: the squared distance (inf where partner is -1)              */
} mipsf_icp_nearest_args;

int mipsf_icp_nearest(const mipsf_icp_nearest_args* a, void* stream);

/* normals[i] = the unit eigenvector of the smallest eigenvalue of the covariance (about the mean, float64) of the
 * min(n, MIPSF_ICP_KNN) points nearest to point i; (0,0,1) when n < 3 or no direction exists.  Its sign is arbitrary.  The grid
 * is one of the same points (any edge). */
typedef struct mipsf_icp_normals_args {
    uint32_t struct_size;
    uint32_t n, max_cells;
    const float* points;                /* [n,3]                                                                           */
    const void* grid;
    double* normals;                    /* [n,3]                                                                           */
    int32_t* neighbours;                /* optional [n, MIPSF_ICP_KNN]: the neighbours of point i, nearest first, -1 padded  */
} mipsf_icp_normals_args;

int mipsf_icp_normals(const mipsf_icp_normals_args* a, void* stream);

/* open3d's registration_icp(source, target, max_dist, identity, TransformationEstimationPointToPlane(),
 * ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)); max_iteration + 1 evaluations are enqueued, a `done`
 * word on the device makes the ones after the stop return at once.  result: MIPSF_ICP_RESULT_DOUBLES doubles. */
typedef struct mipsf_icp_register_args {
    uint32_t struct_size;
    uint32_t n_source, n_target, max_cells, max_iteration;
    const float* source;                /* [n_source,3]                                                                    */
    const void* grid;                   /* of the target, binned with min_edge >= max_dist * (1 + 1e-6)                     */
    const double* target_normals;       /* [n_target,3]                                                                    */
    double max_dist, relative_fitness, relative_rmse;
    double* result;
    int32_t* partner;                   /* optional [n_source]: the pairs of the last evaluation (-1: none)                  */
    void* workspace;                    /* MIPSF_ICP_WS_REGISTER bytes for n_source, 16-byte aligned                        */
} mipsf_icp_register_args;

int mipsf_icp_register(const mipsf_icp_register_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_ICP_H */
