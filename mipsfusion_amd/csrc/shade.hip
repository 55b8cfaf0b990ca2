// What a rendered mesh looks like (include/mipsf_shade.h): area-weighted vertex normals with the order of every sum fixed, and the
// attribute pass that turns the rasteriser's face image into colour, normal and head-lit images.  Upstream renders its meshes with
// a host library; the rules here are the header's, float64 operation by operation, restated in tests/shade_cpu.py.  DESIGN.md 4.22.
//
// Shape of the kernels.  Vertex normals: a lane per face counts the corners of every vertex; the counts become an inclusive prefix
// sum (block_dev.h's device-wide scan); a lane per face claims a slot in the segment of each of its corners by counting the
// segment's end down, so that the end becomes the start; a lane per vertex orders a short segment and sums it, a workgroup per
// queued vertex a long one.  Pixels: a lane per pixel, a wavefront per 8 x 8 tile, a gather of the winner's face, its three
// vertices and what hangs on them, and the stores.
#include "block_dev.h"
#include "../../include/mipsf_shade.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr int SCAN_TILE = TPB * SCAN_ITEMS;     // items one block scans
constexpr uint32_t TILE = MIPSF_SHADE_TILE;
constexpr uint32_t BLOCK_SIDE = 2 * TILE;       // a workgroup: 2 x 2 tiles
constexpr uint32_t SHORT = MIPSF_SHADE_SHORT_SEGMENT;
static_assert(TILE * TILE == MIPSF_WAVE, "one lane per pixel of a tile");
static_assert(WAVES == 4, "2 x 2 tiles per workgroup");

__device__ __forceinline__ void cross3(const double P[3], const double Q[3], double out[3]) {
    out[0] = P[1] * Q[2] - P[2] * Q[1];
    out[1] = P[2] * Q[0] - P[0] * Q[2];
    out[2] = P[0] * Q[1] - P[1] * Q[0];
}
__device__ __forceinline__ double dot3(const double d[3], const double n[3]) { return (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]; }

// the header's unit(P): false = NONE
__device__ __forceinline__ bool unit3(const double P[3], double out[3]) {
    const double L = sqrt(dot3(P, P));
    if (!(L > 0.0 && L < INFINITY)) return false;
    out[0] = P[0] / L, out[1] = P[1] / L, out[2] = P[2] / L;
    return true;
}

// face f -> its indices and its widened vertices; whether it is VALID
__device__ __forceinline__ bool load_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t V, uint32_t f,
                                          int32_t idx[3], double P[3][3]) {
    idx[0] = faces[(size_t)f * 3], idx[1] = faces[(size_t)f * 3 + 1], idx[2] = faces[(size_t)f * 3 + 2];
    if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0 || (uint32_t)idx[0] >= V || (uint32_t)idx[1] >= V || (uint32_t)idx[2] >= V) return false;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float x = vertices[(size_t)idx[c] * 3 + d];
            finite = finite && fabsf(x) < INFINITY;
            P[c][d] = (double)x;
        }
    return finite;
}

// N_f = cross(v[b] - v[a], v[c] - v[a])
__device__ __forceinline__ void face_normal(const double P[3][3], double N[3]) {
    const double E1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const double E2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    cross3(E1, E2, N);
}

// ------------------------------------------------------------------------------------------------ vertex normals
struct NormalsLayout {
    uint64_t count, pos, list, sums, queue, n_long, bytes;    // count, pos: uint32 [V]; list: uint32 [3F]; sums: uint32 [nb]; queue: uint32 [cap]
    uint32_t nb;
};
NormalsLayout normals_layout(uint32_t V, uint32_t F) {
    NormalsLayout L;
    L.nb = blocks_for(V, SCAN_TILE);
    L.count = 0;
    L.pos = align16((uint64_t)V * 4);
    L.list = align16(L.pos + (uint64_t)V * 4);
    L.sums = align16(L.list + (uint64_t)F * 12);
    L.queue = align16(L.sums + (uint64_t)L.nb * 4);
    L.n_long = align16(L.queue + ((uint64_t)F * 3 / (SHORT + 1) + 1) * 4);       // a queued vertex has more than SHORT of the 3F corners
    L.bytes = L.n_long + 16;
    return L;
}
bool normals_in_range(uint32_t V, uint32_t F) { return V <= MIPSF_SHADE_MAX_VERTICES && F <= MIPSF_SHADE_MAX_FACES; }

__global__ void __launch_bounds__(TPB) shade_clear_kernel(uint32_t* __restrict__ count, uint32_t V, uint32_t* __restrict__ n_long) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x; p < V; p += stride) count[p] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_long = 0u;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) shade_count_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                            uint32_t V, uint32_t F, uint32_t* __restrict__ count) {
    const uint32_t f = blockIdx.x * TPB + threadIdx.x;
    if (f >= F) return;
    int32_t idx[3];
    double P[3][3];
    if (!load_face(vertices, faces, V, f, idx, P)) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(count + idx[c], 1u);
}

__global__ void __launch_bounds__(TPB) shade_tile_sum_kernel(const uint32_t* __restrict__ count, uint32_t V, uint32_t* __restrict__ sums) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t s = scan_tile_sum<WAVES>(count, V, sm);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

__global__ void __launch_bounds__(TPB) shade_scan_top_kernel(uint32_t* sums, uint32_t nb) {
    __shared__ uint32_t sm[WAVES];
    scan_top<WAVES>(sums, nb, sm);
}

// pos[i] = the END of vertex i's segment of the list
__global__ void __launch_bounds__(TPB) shade_scan_apply_kernel(const uint32_t* __restrict__ count, uint32_t V, const uint32_t* __restrict__ sums,
                                                               uint32_t* __restrict__ pos) {
    __shared__ uint32_t sm[WAVES];
    scan_apply<WAVES, true>(count, V, sums, pos, sm);
}

// every corner of a valid face counts its vertex's end down by one and owns that slot: afterwards pos[i] is the segment's START
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) shade_fill_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                           uint32_t V, uint32_t F, uint32_t* __restrict__ pos,
                                                                           uint32_t* __restrict__ list) {
    const uint32_t f = blockIdx.x * TPB + threadIdx.x;
    if (f >= F) return;
    int32_t idx[3];
    double P[3][3];
    if (!load_face(vertices, faces, V, f, idx, P)) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) list[atomicSub(pos + idx[c], 1u) - 1u] = f;
}

// N_f of a face the list holds (so a valid one)
__device__ __forceinline__ void listed_normal(const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t V, uint32_t f,
                                              double N[3]) {
    int32_t idx[3];
    double P[3][3];
    load_face(vertices, faces, V, f, idx, P);
    face_normal(P, N);
}

__device__ __forceinline__ void store_normal(const double S[3], float* __restrict__ out) {
    double u[3];
    const bool ok = unit3(S, u);
    out[0] = ok ? (float)u[0] : 0.0f, out[1] = ok ? (float)u[1] : 0.0f, out[2] = ok ? (float)u[2] : 0.0f;
}

// a lane per vertex: a short segment is ordered in place and summed, a long one queued
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) shade_sum_short_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                                uint32_t V, const uint32_t* __restrict__ count,
                                                                                const uint32_t* __restrict__ pos, uint32_t* __restrict__ list,
                                                                                uint32_t* __restrict__ queue, uint32_t* __restrict__ n_long,
                                                                                float* __restrict__ normals) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= V) return;
    const uint32_t k = count[i];
    if (k > SHORT) {
        queue[atomicAdd(n_long, 1u)] = i;
        return;
    }
    uint32_t* seg = list + pos[i];
    for (uint32_t a = 1; a < k; ++a) {
        const uint32_t x = seg[a];
        uint32_t b = a;
        for (; b > 0 && seg[b - 1] > x; --b) seg[b] = seg[b - 1];
        seg[b] = x;
    }
    double S[3] = {0.0, 0.0, 0.0};
    for (uint32_t a = 0; a < k; ++a) {
        double N[3];
        listed_normal(vertices, faces, V, seg[a], N);
        S[0] = S[0] + N[0], S[1] = S[1] + N[1], S[2] = S[2] + N[2];
    }
    store_normal(S, normals + (size_t)i * 3);
}

// A workgroup per queued vertex.  The network: merges of 2, 4, 8, ... ; the first pass of a merge pairs position j of a run with
// the run's position from the other end, the passes after it pair positions half a sub-run apart; the smaller value always goes to
// the lower position, so positions past the segment's end, which would hold +infinity, never take part.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) shade_sum_long_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                               uint32_t V, const uint32_t* __restrict__ count,
                                                                               const uint32_t* __restrict__ pos, uint32_t* __restrict__ list,
                                                                               const uint32_t* __restrict__ queue, const uint32_t* __restrict__ n_long,
                                                                               float* __restrict__ normals) {
    __shared__ double sN[3][TPB];
    const uint32_t todo = *n_long;
    for (uint32_t q = blockIdx.x; q < todo; q += gridDim.x) {
        const uint32_t i = queue[q];
        const uint64_t k = count[i];
        uint32_t* seg = list + pos[i];
        uint64_t padded = 1;
        while (padded < k) padded <<= 1;
        for (uint64_t run = 2; run <= padded; run <<= 1) {
            for (uint64_t half = run >> 1; half > 0; half >>= 1) {
                const bool flip = half == run >> 1;
                for (uint64_t c = threadIdx.x; c < padded >> 1; c += TPB) {
                    const uint64_t lo = (c / half) * (half << 1) + c % half;
                    const uint64_t hi = flip ? (c / half) * (half << 1) + (half << 1) - 1 - c % half : lo + half;
                    if (hi < k) {
                        const uint32_t x = seg[lo], y = seg[hi];
                        if (x > y) seg[lo] = y, seg[hi] = x;
                    }
                }
                __syncthreads();
            }
        }
        double S[3] = {0.0, 0.0, 0.0};
        for (uint64_t base = 0; base < k; base += TPB) {
            if (base + threadIdx.x < k) {
                double N[3];
                listed_normal(vertices, faces, V, seg[base + threadIdx.x], N);
                sN[0][threadIdx.x] = N[0], sN[1][threadIdx.x] = N[1], sN[2][threadIdx.x] = N[2];
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t m = (uint32_t)(k - base < TPB ? k - base : TPB);
                for (uint32_t a = 0; a < m; ++a) S[0] = S[0] + sN[0][a], S[1] = S[1] + sN[1][a], S[2] = S[2] + sN[2][a];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) store_normal(S, normals + (size_t)i * 3);
    }
}

// ------------------------------------------------------------------------------------------------ the attribute pass
struct Shade {
    const float* vertices;
    const int32_t* faces;
    const float* poses;
    const int32_t* face;
    const float* colors;
    const float* vertex_normals;
    float* color;
    float* normals;
    float* shaded;
    unsigned long long* record;
    uint32_t V, F, n, H, W, flags, bx, by;       // bx * by blocks of 16 x 16 pixels per view
    double fx, fy, cx, cy;
    float background[3];
};

__global__ void shade_record_clear_kernel(unsigned long long* record) {
    if (threadIdx.x < MIPSF_SHADE_RECORD_WORDS) record[threadIdx.x] = 0ull;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) shade_pixels_kernel(Shade s) {
    __shared__ uint32_t counts[2];
    if (threadIdx.x < 2) counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t per_view = s.bx * s.by;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t hits = 0, with_n = 0;                // of this wavefront, in every lane
    for (uint32_t b = blockIdx.x; b < s.n * per_view; b += gridDim.x) {
        const uint32_t view = b / per_view, r = b % per_view;
        const uint32_t i = (r % s.bx) * BLOCK_SIDE + (wave & 1u) * TILE + (lane & 7u);
        const uint32_t j = (r / s.bx) * BLOCK_SIDE + (wave >> 1) * TILE + (lane >> 3);
        const bool in = i < s.W && j < s.H;
        bool hit = false, has_n = false;
        if (in) {
            const size_t p = ((size_t)view * s.H + j) * s.W + i;
            const int32_t f = s.face[p];
            int32_t idx[3];
            double P[3][3], w[3] = {0.0, 0.0, 0.0}, dw[3] = {0.0, 0.0, 0.0};
            if (f >= 0 && (uint32_t)f < s.F && load_face(s.vertices, s.faces, s.V, (uint32_t)f, idx, P)) {
                const float* M = s.poses + (size_t)view * 16;
                const double dx = ((double)i - s.cx) / s.fx;
                const double dy = -(((double)j - s.cy) / s.fy);
                double A[3], B[3], C[3], nAB[3], nBC[3], nCA[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    dw[k] = ((double)M[k * 4] * dx + (double)M[k * 4 + 1] * dy) + (double)M[k * 4 + 2] * (-1.0);
                    const double t = (double)M[k * 4 + 3];
                    A[k] = P[0][k] - t, B[k] = P[1][k] - t, C[k] = P[2][k] - t;
                }
                cross3(A, B, nAB), cross3(B, C, nBC), cross3(C, A, nCA);
                const double e0 = dot3(dw, nAB), e1 = dot3(dw, nBC), e2 = dot3(dw, nCA);
                const double den = (e0 + e1) + e2;
                if (den != 0.0 && fabs(den) < INFINITY) {
                    hit = true;
                    w[0] = e1 / den, w[1] = e2 / den, w[2] = e0 / den;
                }
            }
            float rgb[3] = {s.background[0], s.background[1], s.background[2]};
            float n32[3] = {0.0f, 0.0f, 0.0f}, lambert = 0.0f;
            if (hit) {
                if (s.color) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const double cA = (double)s.colors[(size_t)idx[0] * 3 + ch], cB = (double)s.colors[(size_t)idx[1] * 3 + ch],
                                     cC = (double)s.colors[(size_t)idx[2] * 3 + ch];
                        rgb[ch] = (float)((w[0] * cA + w[1] * cB) + w[2] * cC);
                    }
                }
                if (s.normals || s.shaded) {
                    double m[3], n[3];
                    if (s.flags == MIPSF_SHADE_SMOOTH) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const double nA = (double)s.vertex_normals[(size_t)idx[0] * 3 + k], nB = (double)s.vertex_normals[(size_t)idx[1] * 3 + k],
                                         nC = (double)s.vertex_normals[(size_t)idx[2] * 3 + k];
                            m[k] = (w[0] * nA + w[1] * nB) + w[2] * nC;
                        }
                    } else {
                        face_normal(P, m);
                    }
                    has_n = unit3(m, n);
                    if (has_n) {
                        const double sd = dot3(n, dw);
                        if (sd > 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
                        n32[0] = (float)n[0], n32[1] = (float)n[1], n32[2] = (float)n[2];
                        lambert = (float)(fabs(sd) / sqrt(dot3(dw, dw)));
                    }
                }
            }
            if (s.color) s.color[p * 3] = rgb[0], s.color[p * 3 + 1] = rgb[1], s.color[p * 3 + 2] = rgb[2];
            if (s.normals) s.normals[p * 3] = n32[0], s.normals[p * 3 + 1] = n32[1], s.normals[p * 3 + 2] = n32[2];
            if (s.shaded) s.shaded[p] = lambert;
        }
        hits += (uint32_t)__popcll(__ballot(hit)), with_n += (uint32_t)__popcll(__ballot(has_n));
    }
    if (lane == 0) {
        if (hits) atomicAdd(&counts[0], hits);
        if (with_n) atomicAdd(&counts[1], with_n);
    }
    __syncthreads();
    if (threadIdx.x < 2 && counts[threadIdx.x]) atomicAdd(s.record + threadIdx.x, (unsigned long long)counts[threadIdx.x]);
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_shade_workspace_bytes(int which, uint32_t V, uint32_t F) {
    if (which != MIPSF_SHADE_WS_VERTEX_NORMALS || !normals_in_range(V, F)) return 0;
    return normals_layout(V, F).bytes;
}

extern "C" int mipsf_shade_vertex_normals(const mipsf_shade_vertex_normals_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_shade_vertex_normals_args, "mipsf_shade_vertex_normals");
    MIPSF_REQUIRE(a->V <= MIPSF_SHADE_MAX_VERTICES, "mipsf_shade_vertex_normals: %u vertices, at most %u", a->V, MIPSF_SHADE_MAX_VERTICES);
    MIPSF_REQUIRE(a->F <= MIPSF_SHADE_MAX_FACES, "mipsf_shade_vertex_normals: %u faces, at most %u", a->F, MIPSF_SHADE_MAX_FACES);
    MIPSF_REQUIRE(a->workspace && (a->V == 0 || (a->vertices && a->normals)) && (a->F == 0 || a->faces), "mipsf_shade_vertex_normals: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_shade_vertex_normals: workspace not 16-byte aligned");
    if (a->V == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const NormalsLayout L = normals_layout(a->V, a->F);
    char* ws = (char*)a->workspace;
    uint32_t* count = (uint32_t*)(ws + L.count);
    uint32_t* pos = (uint32_t*)(ws + L.pos);
    uint32_t* list = (uint32_t*)(ws + L.list);
    uint32_t* sums = (uint32_t*)(ws + L.sums);
    uint32_t* queue = (uint32_t*)(ws + L.queue);
    uint32_t* n_long = (uint32_t*)(ws + L.n_long);
    const int cus = device_cus();
    const uint32_t wide = (uint32_t)(cus > 0 ? cus : 64) * 8u;      // blocks of a kernel that strides over its work
    const uint32_t vertex_blocks = blocks_for(a->V, TPB), face_blocks = blocks_for(a->F, TPB);
    hipLaunchKernelGGL(shade_clear_kernel, dim3(min(vertex_blocks, wide * 4u)), dim3(TPB), 0, st, count, a->V, n_long);
    if (a->F) hipLaunchKernelGGL(shade_count_kernel, dim3(face_blocks), dim3(TPB), 0, st, a->vertices, a->faces, a->V, a->F, count);
    hipLaunchKernelGGL(shade_tile_sum_kernel, dim3(L.nb), dim3(TPB), 0, st, (const uint32_t*)count, a->V, sums);
    hipLaunchKernelGGL(shade_scan_top_kernel, dim3(1), dim3(TPB), 0, st, sums, L.nb);
    hipLaunchKernelGGL(shade_scan_apply_kernel, dim3(L.nb), dim3(TPB), 0, st, (const uint32_t*)count, a->V, (const uint32_t*)sums, pos);
    if (a->F) hipLaunchKernelGGL(shade_fill_kernel, dim3(face_blocks), dim3(TPB), 0, st, a->vertices, a->faces, a->V, a->F, pos, list);
    hipLaunchKernelGGL(shade_sum_short_kernel, dim3(vertex_blocks), dim3(TPB), 0, st, a->vertices, a->faces, a->V, (const uint32_t*)count,
                       (const uint32_t*)pos, list, queue, n_long, a->normals);
    if (a->F > SHORT / 3)                                           // fewer faces cannot give a vertex more than SHORT corners
        hipLaunchKernelGGL(shade_sum_long_kernel, dim3(wide), dim3(TPB), 0, st, a->vertices, a->faces, a->V, (const uint32_t*)count,
                           (const uint32_t*)pos, list, (const uint32_t*)queue, (const uint32_t*)n_long, a->normals);
    return check_launch("shade_vertex_normals");
}

extern "C" int mipsf_shade_pixels(const mipsf_shade_pixels_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_shade_pixels_args, "mipsf_shade_pixels");
    MIPSF_REQUIRE(a->flags == MIPSF_SHADE_FLAT || a->flags == MIPSF_SHADE_SMOOTH, "mipsf_shade_pixels: flags %u: MIPSF_SHADE_FLAT or MIPSF_SHADE_SMOOTH",
                  a->flags);
    MIPSF_REQUIRE(a->record, "mipsf_shade_pixels: null pointer (record)");
    hipStream_t st = (hipStream_t)stream;
    if (a->n == 0) {
        hipLaunchKernelGGL(shade_record_clear_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, (unsigned long long*)a->record);
        return check_launch("shade_pixels");
    }
    MIPSF_REQUIRE(a->F > 0, "mipsf_shade_pixels: a mesh without faces has nothing to shade");
    MIPSF_REQUIRE(a->H > 0 && a->W > 0, "mipsf_shade_pixels: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_SHADE_MAX_SIDE && a->W <= MIPSF_SHADE_MAX_SIDE, "mipsf_shade_pixels: image %u x %u, at most %u a side", a->H, a->W,
                  MIPSF_SHADE_MAX_SIDE);
    MIPSF_REQUIRE(a->F <= MIPSF_SHADE_MAX_FACES, "mipsf_shade_pixels: %u faces, at most %u", a->F, MIPSF_SHADE_MAX_FACES);
    MIPSF_REQUIRE((uint64_t)a->n * a->H * a->W <= MIPSF_SHADE_MAX_PIXELS, "mipsf_shade_pixels: %u views of %u x %u pixels, at most %u pixels a call", a->n,
                  a->H, a->W, MIPSF_SHADE_MAX_PIXELS);
    MIPSF_REQUIRE((uint64_t)a->n * a->F <= MIPSF_SHADE_MAX_ITEMS, "mipsf_shade_pixels: %u views of %u faces, at most %u pairs a call", a->n, a->F,
                  MIPSF_SHADE_MAX_ITEMS);
    MIPSF_REQUIRE(a->fx > 0.0 && a->fx < INFINITY && a->fy > 0.0 && a->fy < INFINITY && fabs(a->cx) < INFINITY && fabs(a->cy) < INFINITY,
                  "mipsf_shade_pixels: intrinsics %g %g %g %g", a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->faces && a->poses && a->face && (a->vertices || a->V == 0), "mipsf_shade_pixels: null pointer");
    MIPSF_REQUIRE(!a->color || a->colors, "mipsf_shade_pixels: color asked for without vertex colours");
    MIPSF_REQUIRE(a->flags != MIPSF_SHADE_SMOOTH || a->vertex_normals || !(a->normals || a->shaded),
                  "mipsf_shade_pixels: MIPSF_SHADE_SMOOTH without vertex_normals");
    Shade s;
    s.vertices = a->vertices, s.faces = a->faces, s.poses = a->poses, s.face = a->face, s.colors = a->colors, s.vertex_normals = a->vertex_normals;
    s.color = a->color, s.normals = a->normals, s.shaded = a->shaded, s.record = (unsigned long long*)a->record;
    s.V = a->V, s.F = a->F, s.n = a->n, s.H = a->H, s.W = a->W, s.flags = a->flags;
    s.bx = blocks_for(a->W, BLOCK_SIDE), s.by = blocks_for(a->H, BLOCK_SIDE);
    s.fx = a->fx, s.fy = a->fy, s.cx = a->cx, s.cy = a->cy;
    s.background[0] = a->background[0], s.background[1] = a->background[1], s.background[2] = a->background[2];
    // n * H * W <= 2^30, so there are at most 2^30 blocks of pixels.  A workgroup strides over them and adds its two counts to
    // the record once at its end: with a workgroup per block of pixels the 2 x 71 300 additions to one address of 64 views at
    // 460 x 620 took 0.89 ms, whatever the outputs
    const int cus = device_cus();
    const uint32_t wide = (uint32_t)(cus > 0 ? cus : 64) * 16u;
    hipLaunchKernelGGL(shade_record_clear_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, s.record);
    hipLaunchKernelGGL(shade_pixels_kernel, dim3(min(a->n * s.bx * s.by, wide)), dim3(TPB), 0, st, s);
    return check_launch("shade_pixels");
}
