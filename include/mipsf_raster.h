/*
 * mipsf_raster.h -- a triangle mesh as per-pixel depth from a batch of camera poses, and the two uses the NICE-SLAM / Co-SLAM
 * evaluation has for it: depth L1 between the rendered reconstruction and the rendered ground truth, and the occlusion test of
 * the culling (a face behind the rendered depth is dropped).  DESIGN.md 4.18; mipsfusion_amd/mesh_render.py.
 *
 * Same conventions as mipsf_eval.h: int return code, message through mipsf_last_error(), one argument block per entry point with
 * `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Workspaces are
 * the caller's; mipsf_raster_workspace_bytes() gives their sizes.  Nothing here uses a floating-point atomic and no kernel waits
 * on another workgroup; the same call gives the same bytes.  Every floating-point operation named below is one IEEE float64
 * operation rounded on its own (no contraction), fp32 inputs widened first, so a float64 restatement on the host
 * (tests/raster_cpu.py) gives the same words.
 */
#ifndef MIPSF_RASTER_H
#define MIPSF_RASTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_RASTER_TILE 8u                     /* a tile is 8 x 8 pixels: one wavefront, one lane per pixel                  */
#define MIPSF_RASTER_MAX_FACES (1u << 30)        /* the face index is the low word of a key and -1 must stay free              */
#define MIPSF_RASTER_MAX_SIDE 8192u              /* H and W of an image: at most 2^20 tiles per image                          */
#define MIPSF_RASTER_MAX_PIXELS (1u << 30)       /* n * H * W of one call                                                       */
#define MIPSF_RASTER_MAX_ITEMS 0x7fffffffu       /* n * F of one call: one (view, face) pair per lane of the count kernel.  The */
                                                 /* tiles of one call are counted in uint64: at most 2^31 * 2^20, never wrapping */

/* mipsf_raster_workspace_bytes(which, n, F, H, W): bytes of a workspace; 0 = out of range */
#define MIPSF_RASTER_WS_DEPTH 1                  /* mipsf_raster_depth for n views of F faces at H x W                         */
#define MIPSF_RASTER_WS_L1 2                     /* mipsf_raster_l1 for n views at H x W (F is ignored)                        */
uint64_t mipsf_raster_workspace_bytes(int which, uint32_t n, uint32_t F, uint32_t H, uint32_t W);

/* The depth of a mesh from n poses (camera to world, row-major 4 x 4, the OpenGL convention of the datasets: the camera looks
 * along its -z, +y is up; R = pose[:3,:3], t = pose[:3,3]).  Homogeneous ray-triangle rasterisation in the WORLD frame: nothing
 * is clipped at a near plane and the pose is never inverted.  All values float64, parentheses give the order:
 *   pixel (row j, col i)   dx = (i - cx)/fx;  dy = -((j - cy)/fy);
 *                          dw[k] = (R[k][0]*dx + R[k][1]*dy) + R[k][2]*(-1.0),  k = 0..2
 *   face (a, b, c)         A = v[a] - t, B = v[b] - t, C = v[c] - t;
 *                          cross(P,Q) = (P.y*Q.z - P.z*Q.y, P.z*Q.x - P.x*Q.z, P.x*Q.y - P.y*Q.x);
 *                          nAB = cross(A,B), nBC = cross(B,C), nCA = cross(C,A)
 *   dot(d,n)             = (d.x*n.x + d.y*n.y) + d.z*n.z;   e0 = dot(dw,nAB), e1 = dot(dw,nBC), e2 = dot(dw,nCA)
 *   inside               = (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0)
 *   den = (e0 + e1) + e2;  num = dot(A, nBC);  tt = num / den;  d32 = (float)tt
 *   hit                  = inside && den != 0 && tt > near && tt < far && 2^-126 <= d32 < inf
 *   key                  = ((uint64)bits(d32) << 32) | face index;  the pixel keeps the SMALLEST key over the faces
 * tt is the z-depth (the camera-frame direction has z = -1).  The mesh is two-sided.  A face with an index outside [0, V) or a
 * vertex that is not finite hits nothing.  The edge rule is inclusive and cross(B,A) = -cross(A,B) exactly, so two faces that
 * share an edge never both reject a pixel between them; a tie in d32 goes to the lower face index.  The smallest key is an
 * integer minimum: the image does not depend on the order of work.
 *   depth[v][j][i] = d32 of the kept key, 0 for a pixel nothing hits (the datasets' value for a missing depth)
 *   face[v][j][i]  = its face index, -1 for a pixel nothing hits
 * Kernels: the number of 8 x 8 tiles in each (view, face)'s conservative screen box (none for a face wholly behind the camera or
 * with a repeated vertex; the box of the part in front of the camera for a face that crosses the camera plane; the whole image
 * for a face with a vertex in the camera plane or whose plane passes through the camera) ->
 * 64-bit prefix sum -> one wavefront per tile, found by binary search in the sum, 64-bit atomicMin of the key -> keys to depth
 * and face.  The box is found in arithmetic of its own; it never leaves out a pixel the rule above hits.
 * Refused on the host, with nothing launched: n = 0, F = 0, H * W = 0, H or W above MIPSF_RASTER_MAX_SIDE, F above
 * MIPSF_RASTER_MAX_FACES, n * H * W above MIPSF_RASTER_MAX_PIXELS, n * F above MIPSF_RASTER_MAX_ITEMS, fx or fy not positive and
 * finite, cx or cy not finite, near or far NaN, a null pointer, a workspace that is not 16-byte aligned. */
#define MIPSF_RASTER_STAGE_COUNT 1u              /* clear the keys, count the tiles of every (view, face)                      */
#define MIPSF_RASTER_STAGE_SCAN 2u               /* prefix sum of the counts                                                   */
#define MIPSF_RASTER_STAGE_RASTER 4u             /* the tiles                                                                  */
#define MIPSF_RASTER_STAGE_RESOLVE 8u            /* keys -> depth, face                                                        */

typedef struct mipsf_raster_depth_args {
    uint32_t struct_size;
    uint32_t V, F, n, H, W;
    uint32_t stages;                    /* 0 = all four.  A subset repeats those stages on a workspace that a full call with the
                                           same arguments has filled (tools/raster_time.py times them one by one)            */
    uint32_t reserved;
    double fx, fy, cx, cy, near, far;
    const float* vertices;              /* [V,3]                                                                           */
    const int32_t* faces;               /* [F,3]                                                                           */
    const float* poses;                 /* [n,4,4]                                                                         */
    float* depth;                       /* [n,H,W]                                                                         */
    int32_t* face;                      /* [n,H,W]                                                                         */
    void* workspace;                    /* MIPSF_RASTER_WS_DEPTH bytes for (n, F, H, W), 16-byte aligned                     */
} mipsf_raster_depth_args;

int mipsf_raster_depth(const mipsf_raster_depth_args* a, void* stream);

/* Two depth stacks [n,H,W] -> one record per view.  A pixel is hit in an image when its value is not 0; a miss counts as depth 0,
 * as published.  Every term is |(double)a - (double)b|.  The sums are added in a fixed order (lane -> wave butterfly -> waves
 * ascending -> block partial; one finishing wave per view). */
typedef struct mipsf_raster_l1_record {
    double sum_all;                     /* over all H*W pixels                                                             */
    double sum_both;                    /* over the pixels both images hit                                                 */
    uint64_t both, rec_only, gt_only, neither;      /* a = rec, b = gt; the four add up to H*W                             */
    uint64_t reserved[2];
} mipsf_raster_l1_record;

typedef struct mipsf_raster_l1_args {
    uint32_t struct_size;
    uint32_t n, H, W;
    const float* a;                     /* [n,H,W]: the reconstruction's depth                                             */
    const float* b;                     /* [n,H,W]: the ground truth's                                                     */
    mipsf_raster_l1_record* records;    /* [n]                                                                             */
    void* workspace;                    /* MIPSF_RASTER_WS_L1 bytes for (n, H, W), 16-byte aligned                           */
} mipsf_raster_l1_args;

int mipsf_raster_l1(const mipsf_raster_l1_args* a, void* stream);

/* seen[p] = 1 when some view sees point p, else 0.  The pose is taken as rigid: the transpose of R stands for its inverse.
 * In float64, for view k with depth image D[k]:
 *   q = p - t;  cam[c] = (R[0][c]*q.x + R[1][c]*q.y) + R[2][c]*q.z;  z = -cam.z;
 *   u = cx + fx*(cam.x/z);  v = cy - fy*(cam.y/z);  col = floor(u + 0.5), row = floor(v + 0.5)
 *   seen by k = z > 0 && z < (double)max_depth[k] && edge < u && u < (double)W - edge && edge < v && v < (double)H - edge
 *               && 0 <= col < W && 0 <= row < H && (D[k][row][col] == 0 || z <= (double)D[k][row][col] + eps)
 * (the bounds on col and row matter only for an edge below one half).  A pixel without depth occludes nothing. */
typedef struct mipsf_raster_visible_args {
    uint32_t struct_size;
    uint32_t m, n, H, W;
    uint32_t reserved;
    double fx, fy, cx, cy, edge, eps;
    const float* points;                /* [m,3]                                                                           */
    const float* depth;                 /* [n,H,W]                                                                         */
    const float* poses;                 /* [n,4,4]                                                                         */
    const float* max_depth;             /* [n]                                                                             */
    uint8_t* seen;                      /* [m]                                                                             */
} mipsf_raster_visible_args;

int mipsf_raster_visible(const mipsf_raster_visible_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_RASTER_H */
