/*
 * mipsf_shade.h -- what a rendered mesh looks like: per-vertex normals of a triangle mesh, and the attribute pass that turns the
 * face image of mipsf_raster_depth into colour, normal and head-lit "shaded geometry" images.  DESIGN.md 4.22;
 * mipsfusion_amd/mesh_render.py.
 *
 * Same conventions as mipsf_raster.h: int return code, message through mipsf_last_error(), one argument block per entry point
 * with `struct_size` first, DEVICE pointers, everything enqueued on `stream`, no allocation and no synchronisation.  Workspaces
 * are the caller's; mipsf_shade_workspace_bytes() gives their sizes.  Nothing here uses a floating-point atomic and no kernel
 * waits on another workgroup; the same call gives the same bytes.  Every floating-point operation named below is one IEEE float64
 * operation rounded on its own (no contraction), fp32 inputs widened first, and the only operations are + - * / sqrt, so a
 * float64 restatement on the host (tests/shade_cpu.py) gives the same words.
 *
 * Shared by both entry points, all values float64, parentheses give the order:
 *   cross(P,Q) = (P.y*Q.z - P.z*Q.y, P.z*Q.x - P.x*Q.z, P.x*Q.y - P.y*Q.x)      (mipsf_raster.h's)
 *   dot(d,n)   = (d.x*n.x + d.y*n.y) + d.z*n.z                                   (mipsf_raster.h's)
 *   len(P)     = sqrt(dot(P,P))
 *   unit(P)    = (P.x/L, P.y/L, P.z/L) with L = len(P) when L > 0 and L < inf; otherwise NONE
 *   face (a, b, c) is VALID when a, b, c lie in [0, V) and its nine fp32 coordinates are finite (the rasteriser's rule for a face
 *                that can hit);  N_f = cross(v[b] - v[a], v[c] - v[a]): its length is twice the area
 */
#ifndef MIPSF_SHADE_H
#define MIPSF_SHADE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPSF_SHADE_TILE 8u                      /* a wavefront shades 8 x 8 pixels of one view, one lane per pixel             */
#define MIPSF_SHADE_MAX_FACES (1u << 30)         /* MIPSF_RASTER_MAX_FACES; 3 F corners stay below 2^32                          */
#define MIPSF_SHADE_MAX_VERTICES 0x7fffffffu     /* an index is an int32                                                        */
#define MIPSF_SHADE_MAX_SIDE 8192u               /* MIPSF_RASTER_MAX_SIDE                                                       */
#define MIPSF_SHADE_MAX_PIXELS (1u << 30)        /* MIPSF_RASTER_MAX_PIXELS: n * H * W of one call                               */
#define MIPSF_SHADE_MAX_ITEMS 0x7fffffffu        /* MIPSF_RASTER_MAX_ITEMS: n * F of one call, refused as the rasteriser does    */
#define MIPSF_SHADE_SHORT_SEGMENT 32u            /* corners of a vertex one lane orders on its own (below)                      */

/* mipsf_shade_workspace_bytes(which, V, F): bytes of a workspace; 0 = out of range.  mipsf_shade_pixels needs none. */
#define MIPSF_SHADE_WS_VERTEX_NORMALS 1          /* mipsf_shade_vertex_normals for V vertices and F faces                       */
uint64_t mipsf_shade_workspace_bytes(int which, uint32_t V, uint32_t F);

/* Area-weighted vertex normals.  For vertex i, S starts at +0.0 per component and adds N_f over the VALID faces that name i, in
 * ASCENDING face index, once per corner that names it (a face that names i twice has a repeated vertex and N_f = 0);
 *   normal[i] = (float)unit(S), or 0 0 0 when unit(S) is NONE: an isolated vertex, a fan whose faces cancel, no valid face at all.
 * The order of the sum is part of the rule; the result does not depend on the order of work.
 * Kernels: the corners of every vertex are counted (integer atomics), the counts become a prefix sum (block_dev.h's device-wide
 * scan), every valid face writes its index into the segment of each of its corners (integer atomics: the segment's order is
 * not fixed yet), then every segment is put in ascending order and summed.  A segment of at most MIPSF_SHADE_SHORT_SEGMENT
 * corners is ordered by ONE lane (insertion sort in place).  A longer one is queued and taken by a whole workgroup: a bitonic
 * network whose comparators all point the same way, so that the segment needs no padding to a power of two, in place in the
 * workspace, log2^2 passes; then 256 corners at a time have their N_f computed side by side and one lane adds them in order.  A
 * vertex named by every face (a fan's apex of valence F) therefore takes O(F log^2 F / 256) comparisons and F additions in a
 * row, which the rule itself demands; it finishes.
 * V = 0 is a no-op.  F = 0 writes zeros.  Refused on the host, with nothing launched: V above MIPSF_SHADE_MAX_VERTICES, F above
 * MIPSF_SHADE_MAX_FACES, a null pointer (vertices and normals when V > 0, faces when F > 0, the workspace), a workspace that is
 * not 16-byte aligned. */
typedef struct mipsf_shade_vertex_normals_args {
    uint32_t struct_size;
    uint32_t V, F;
    uint32_t reserved;
    const float* vertices;              /* [V,3]                                                                           */
    const int32_t* faces;               /* [F,3]                                                                           */
    float* normals;                     /* [V,3]                                                                           */
    void* workspace;                    /* MIPSF_SHADE_WS_VERTEX_NORMALS bytes for (V, F), 16-byte aligned                   */
} mipsf_shade_vertex_normals_args;

int mipsf_shade_vertex_normals(const mipsf_shade_vertex_normals_args* a, void* stream);

/* The attribute pass over the face image of mipsf_raster_depth, given the same vertices, faces, poses and intrinsics.  Per view and pixel
 * (row j, col i) with f = face[view][j][i]:
 *   MISS when f < 0, f >= F or face f is not VALID.
 *   dx, dy, dw, R, t, A, B, C, nAB, nBC, nCA, e0, e1, e2 and den = (e0 + e1) + e2 are exactly mipsf_raster.h's.
 *   MISS also when den == 0 or den is not finite.
 *   wA = e1/den, wB = e2/den, wC = e0/den      the barycentric weights of the hit point: P = tt*dw = wA*A + wB*B + wC*C and
 *                                               tt = dot(A,nBC)/den, so dotting P with cross(B,C) gives wA, and so on round
 *   color[ch]  = (float)((wA*cA[ch] + wB*cB[ch]) + wC*cC[ch])                     cA = colors[a] widened, ...
 *   n          = unit(N_f)                                                        MIPSF_SHADE_FLAT
 *              = unit(m), m[k] = (wA*nA[k] + wB*nB[k]) + wC*nC[k]                 MIPSF_SHADE_SMOOTH; nA = vertex_normals[a] widened
 *   s          = dot(n, dw);  when s > 0 every component of n is negated (the mesh is two-sided; s == 0 leaves n as it is)
 *   normals[k] = (float)n[k]                                                      in the world frame, towards the camera
 *   shaded     = (float)(|s| / len(dw))                                           the head-light Lambert term, 0 .. 1
 * A MISS has color = background, normals = 0 0 0, shaded = 0.  A pixel whose n is NONE keeps its colour and has normals 0 0 0 and
 * shaded 0.  n is computed only when `normals` or `shaded` is an output.
 * record[0] = the number of pixels that are no MISS, record[1] = the number of those with an n (0 when n is not computed); both
 * uint64, cleared first, added with integer atomics.
 * Kernel: one lane per pixel, a wavefront per 8 x 8 tile, four of them per workgroup (16 x 16 pixels of one view), so that
 * neighbouring lanes gather the same faces; a workgroup strides over such blocks of pixels and adds its two counts to the record
 * once, at its end; no workspace.
 * n = 0 writes a zero record and nothing else.  Refused on the host, with nothing launched: what mipsf_raster_depth refuses for
 * the same fields (F = 0, H * W = 0, H or W above MIPSF_SHADE_MAX_SIDE, F above MIPSF_SHADE_MAX_FACES, n * H * W above
 * MIPSF_SHADE_MAX_PIXELS, n * F above MIPSF_SHADE_MAX_ITEMS, fx or fy not positive and finite, cx or cy not finite, a null
 * vertices (with V > 0), faces, poses or face pointer); flags other than exactly MIPSF_SHADE_FLAT or MIPSF_SHADE_SMOOTH;
 * MIPSF_SHADE_SMOOTH without vertex_normals while `normals` or `shaded` is an output; `color` without colors; a null record. */
#define MIPSF_SHADE_FLAT 1u
#define MIPSF_SHADE_SMOOTH 2u
#define MIPSF_SHADE_RECORD_WORDS 2u              /* uint64 hits, shaded                                                         */

typedef struct mipsf_shade_pixels_args {
    uint32_t struct_size;
    uint32_t V, F, n, H, W;
    uint32_t flags;                     /* MIPSF_SHADE_FLAT or MIPSF_SHADE_SMOOTH                                          */
    uint32_t reserved;
    double fx, fy, cx, cy;
    float background[3];
    float reserved2;
    const float* vertices;              /* [V,3]                                                                           */
    const int32_t* faces;               /* [F,3]                                                                           */
    const float* poses;                 /* [n,4,4]                                                                         */
    const int32_t* face;                /* [n,H,W]: the face image of mipsf_raster_depth                                   */
    const float* colors;                /* [V,3] or null                                                                   */
    const float* vertex_normals;        /* [V,3] or null                                                                   */
    float* color;                       /* [n,H,W,3] or null                                                               */
    float* normals;                     /* [n,H,W,3] or null                                                               */
    float* shaded;                      /* [n,H,W] or null                                                                 */
    uint64_t* record;                   /* [MIPSF_SHADE_RECORD_WORDS]                                                      */
} mipsf_shade_pixels_args;

int mipsf_shade_pixels(const mipsf_shade_pixels_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIPSF_SHADE_H */
