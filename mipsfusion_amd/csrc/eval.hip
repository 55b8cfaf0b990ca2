// Scoring a mesh against ground truth (include/mipsf_eval.h): area-uniform stratified samples of a triangle mesh, the exact
// nearest neighbour without a radius over the grid of icp.hip, and the reduction of the distances.  Upstream has no evaluation
// code; the protocol is the published one of the NICE-SLAM / Co-SLAM evaluation (cloud to cloud).  DESIGN.md 4.17.
//
// Shape of the kernels: one face, one sample, one source point or one distance per lane.  Areas are integers (units of 2^-40 m^2),
// so their prefix sum is the same in any order; everything else a result depends on is float64, one operation at a time (the
// library is built with -ffp-contract=off), which tests/eval_cpu.py restates word for word.  Sums are added in a fixed order: lane
// -> wave (cross-lane moves) -> block partials in a buffer -> one finishing wave.
#include "block_dev.h"
#include "icp_grid.h"
#include "../../include/mipsf_eval.h"
#include "../../include/mipsf_icp.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr int SCAN_TILE = TPB * SCAN_ITEMS;  // faces one block scans
constexpr uint32_t STATS_MAX_BLOCKS = 1024;
constexpr uint64_t UNITS_CAP = 1ull << 63;   // a total of this many units or more is refused

// ------------------------------------------------------------------------------------------------ sampler
struct MeshView {
    const float* vertices;
    const int32_t* faces;
    uint32_t V, F;
};

struct SampleLayout {
    uint64_t cum, tiles, bytes;      // cum: uint64 [F]; tiles: uint64 [3][nb] = sum, sum of high halves, sum of low halves
    uint32_t nb;
};
SampleLayout sample_layout(uint32_t F) {
    SampleLayout L;
    L.nb = blocks_for(F ? F : 1, SCAN_TILE);
    L.cum = 0;
    L.tiles = align16((uint64_t)(F ? F : 1) * 8);
    L.bytes = L.tiles + (uint64_t)L.nb * 3 * 8;
    return L;
}

__device__ __forceinline__ bool face_vertices(const MeshView& m, uint32_t f, double A[3], double B[3], double C[3]) {
    const int32_t ia = m.faces[(size_t)f * 3], ib = m.faces[(size_t)f * 3 + 1], ic = m.faces[(size_t)f * 3 + 2];
    if (ia < 0 || ib < 0 || ic < 0 || (uint32_t)ia >= m.V || (uint32_t)ib >= m.V || (uint32_t)ic >= m.V) return false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        A[d] = (double)m.vertices[(size_t)ia * 3 + d];
        B[d] = (double)m.vertices[(size_t)ib * 3 + d];
        C[d] = (double)m.vertices[(size_t)ic * 3 + d];
    }
    return true;
}

__device__ __forceinline__ uint64_t face_units(const MeshView& m, uint32_t f) {
    double A[3], B[3], C[3];
    if (!face_vertices(m, f, A, B, C)) return 0;
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area < INFINITY)) return 0;       // NaN too
    const double t = area * 0x1p40;
    return t >= 0x1p63 ? UNITS_CAP : (uint64_t)floor(t);
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) eval_units_kernel(MeshView m, uint64_t* __restrict__ cum, uint64_t* __restrict__ tiles,
                                                                           uint32_t nb) {
    __shared__ uint64_t sm[WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint64_t s = 0, hi = 0, lo = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < m.F) {
            const uint64_t u = face_units(m, (uint32_t)(base + k));
            cum[base + k] = u;
            s += u, hi += u >> 32, lo += u & 0xffffffffull;
        }
    s = block_reduce<WAVES>(s, sm, Add()), hi = block_reduce<WAVES>(hi, sm, Add()), lo = block_reduce<WAVES>(lo, sm, Add());
    if (threadIdx.x == 0) tiles[blockIdx.x] = s, tiles[nb + blockIdx.x] = hi, tiles[2 * (size_t)nb + blockIdx.x] = lo;
}

// one block: tiles[0..nb) becomes its exclusive scan; the record is written.  The halves cannot wrap (F < 2^32 terms below 2^32
// each), so hi + (lo >> 32) is the true total >> 32.
__global__ void __launch_bounds__(TPB) eval_scan_top_kernel(uint64_t* tiles, uint32_t nb, mipsf_eval_sample_record* rec) {
    __shared__ uint64_t sm[WAVES];
    uint32_t lo_i, hi_i;
    scan_top_range<WAVES>(nb, lo_i, hi_i);
    uint64_t hi = 0, lo = 0;
    for (uint32_t i = lo_i; i < hi_i; ++i) hi += tiles[nb + i], lo += tiles[2 * (size_t)nb + i];
    const uint64_t total = scan_top<WAVES>(tiles, nb, sm);
    hi = block_reduce<WAVES>(hi, sm, Add()), lo = block_reduce<WAVES>(lo, sm, Add());
    if (threadIdx.x == 0) {
        const bool over = hi + (lo >> 32) >= (UNITS_CAP >> 32);
        rec->total_units = total;
        rec->area = (double)total * 0x1p-40;
        rec->status = over ? MIPSF_EVAL_AREA_OVERFLOW : (total == 0 ? MIPSF_EVAL_NO_AREA : MIPSF_EVAL_OK);
        rec->reserved[0] = rec->reserved[1] = rec->reserved[2] = 0u;
    }
}

// cum: the faces' units in, their inclusive prefix sum out
__global__ void __launch_bounds__(TPB) eval_scan_apply_kernel(uint64_t* cum, uint32_t F, const uint64_t* __restrict__ tiles) {
    __shared__ uint64_t sm[WAVES];
    scan_apply<WAVES, true>(cum, F, tiles, cum, sm);
}

__device__ __forceinline__ double uniform24(uint32_t seed, uint32_t k, uint32_t which) {
    uint32_t h = seed * 0x9e3779b9u + k * 3u + which;
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return (double)(h >> 8) * 0x1p-24;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) eval_draw_kernel(MeshView m, const uint64_t* __restrict__ cum,
                                                                          const mipsf_eval_sample_record* rec, uint32_t n, uint32_t seed,
                                                                          float* __restrict__ points, int32_t* __restrict__ face_of) {
    const uint32_t k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n || rec->status != MIPSF_EVAL_OK) return;
    const uint64_t total = rec->total_units;            // 0 < total < 2^63
    const double u0 = uniform24(seed, k, 0u), u1 = uniform24(seed, k, 1u), u2 = uniform24(seed, k, 2u);
    const double x = (((double)k + u0) / (double)n) * (double)total;
    uint64_t pos = (uint64_t)x;
    if (pos > total - 1) pos = total - 1;
    uint32_t lo = 0, hi = m.F - 1;                       // the first f with cum[f] > pos; cum[F-1] = total > pos
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cum[mid] > pos) hi = mid;
        else lo = mid + 1;
    }
    double A[3], B[3], C[3];
    const bool ok = face_vertices(m, lo, A, B, C);      // a face with units has its indices in range
    const double r = sqrt(u1), a = 1.0 - r, b = r * (1.0 - u2), c = r * u2;
    face_of[k] = (int32_t)lo;
#pragma unroll
    for (int d = 0; d < 3; ++d) points[(size_t)k * 3 + d] = ok ? (float)((a * A[d] + b * B[d]) + c * C[d]) : 0.0f;
}

// ------------------------------------------------------------------------------------------------ nearest neighbour, no radius
__device__ __forceinline__ void nearest_run(const Grid& g, uint32_t n, uint32_t c0, uint32_t c1, double qx, double qy, double qz,
                                            double& bd, uint32_t& bj) {
    const uint32_t s = g.start[c0], e = min(g.start[c1 + 1], n);
    for (uint32_t p = s; p < e; ++p) {
        const float4 v = g.sorted[p];
        const double d2 = dist2(qx, qy, qz, v);
        const uint32_t j = __float_as_uint(v.w);
        if (d2 < bd || (d2 == bd && j < bj)) bd = d2, bj = j;
    }
}

// One source point per lane; rings of cells around the point's clamped cell, the best candidate in registers.  The point need
// not lie in that cell (a reconstruction has surface where the ground truth has none), so what the scanned block covers is
// measured from the point itself: an unscanned target point lies beyond one of the block's face planes that still have cells
// behind them, at least the point's distance to that plane away.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) eval_nearest_kernel(const float* __restrict__ src, uint32_t n_source, uint32_t n_target,
                                                                             Grid g, int32_t* __restrict__ index, double* __restrict__ d2_out) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n_source) return;
    const double q[3] = {(double)src[(size_t)i * 3], (double)src[(size_t)i * 3 + 1], (double)src[(size_t)i * 3 + 2]};
    double bd = INFINITY;
    uint32_t bj = 0xffffffffu;
    const bool finite = fabs(q[0]) < INFINITY && fabs(q[1]) < INFINITY && fabs(q[2]) < INFINITY;      // NaN: false
    if (n_target > 0 && finite) {
        const GridHdr h = *g.hdr;
        const int dim[3] = {(int)h.dims[0], (int)h.dims[1], (int)h.dims[2]};
        int c[3];
        double span = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            c[d] = (int)cell_of(q[d], h.origin[d], h.edge, h.dims[d]);
            span = fmax(span, fabs(h.origin[d]) + (double)dim[d] * h.edge);
        }
        const double slack = 16.0 * 2.220446049250313e-16 * span;      // rounding of a plane's position and of the binning's quotient
        for (int r = 0;; ++r) {
            int lo[3], hi[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) lo[d] = max(c[d] - r, 0), hi[d] = min(c[d] + r, dim[d] - 1);
            for (int x = lo[0]; x <= hi[0]; ++x)
                for (int y = lo[1]; y <= hi[1]; ++y) {
                    const uint32_t row = ((uint32_t)x * h.dims[1] + (uint32_t)y) * h.dims[2];
                    if (x - c[0] == r || c[0] - x == r || y - c[1] == r || c[1] - y == r) {
                        nearest_run(g, n_target, row + lo[2], row + hi[2], q[0], q[1], q[2], bd, bj);
                    } else {
                        if (c[2] - r >= 0) nearest_run(g, n_target, row + (c[2] - r), row + (c[2] - r), q[0], q[1], q[2], bd, bj);
                        if (c[2] + r <= dim[2] - 1)
                            nearest_run(g, n_target, row + (c[2] + r), row + (c[2] + r), q[0], q[1], q[2], bd, bj);
                    }
                }
            double bound = INFINITY;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (lo[d] > 0) bound = fmin(bound, fmax(q[d] - (h.origin[d] + (double)lo[d] * h.edge), 0.0));
                if (hi[d] < dim[d] - 1) bound = fmin(bound, fmax((h.origin[d] + (double)(hi[d] + 1) * h.edge) - q[d], 0.0));
            }
            if (!(bound < INFINITY)) break;       // the block is the grid
            const double covered = fmax(bound * (1.0 - 1.0e-6) - slack, 0.0);
            if (bd <= covered * covered) break;
        }
    }
    const bool found = bj < n_target;
    index[i] = found ? (int32_t)bj : -1;
    d2_out[i] = found ? bd : (double)INFINITY;
}

// ------------------------------------------------------------------------------------------------ statistics
struct StatsPartial {
    double sum_d, sum_d2, max_d2;
    uint64_t within, finite;
    uint64_t pad[3];
};
static_assert(sizeof(StatsPartial) == 64 && sizeof(mipsf_eval_stats_record) == 64, "stats records");
static_assert(sizeof(mipsf_eval_sample_record) == 32, "sample record");

__device__ __forceinline__ double wave_max_d(double v) {
    return wave_reduce(v, [](double a, double b) { return fmax(a, b); });
}

// block b, thread t takes entries (b*TPB + t) + j * (blocks*TPB); butterfly over the wave; waves in ascending order
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) eval_stats_partial_kernel(const double* __restrict__ d2, uint32_t n, double thr2,
                                                                                   StatsPartial* __restrict__ part) {
    __shared__ StatsPartial sm[WAVES];
    double sd = 0.0, s2 = 0.0, mx = 0.0;
    uint64_t within = 0, fin = 0;
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        const double v = d2[i];
        if (v >= 0.0 && v < INFINITY) {
            sd += sqrt(v), s2 += v, mx = fmax(mx, v);
            within += v <= thr2 ? 1u : 0u;
            ++fin;
        }
    }
    sd = wave_sum_d(sd), s2 = wave_sum_d(s2), mx = wave_max_d(mx);
    within = wave_sum_u64(within), fin = wave_sum_u64(fin);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = StatsPartial{sd, s2, mx, within, fin, {0, 0, 0}};
    __syncthreads();
    if (threadIdx.x == 0) {
        StatsPartial p = sm[0];
        for (int w = 1; w < WAVES; ++w)
            p.sum_d += sm[w].sum_d, p.sum_d2 += sm[w].sum_d2, p.max_d2 = fmax(p.max_d2, sm[w].max_d2), p.within += sm[w].within,
                p.finite += sm[w].finite;
        part[blockIdx.x] = p;
    }
}

// one wave: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) eval_stats_finish_kernel(const StatsPartial* __restrict__ part, uint32_t nb,
                                                                                         mipsf_eval_stats_record* rec) {
    double sd = 0.0, s2 = 0.0, mx = 0.0;
    uint64_t within = 0, fin = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += MIPSF_WAVE) {
        const StatsPartial p = part[b];
        sd += p.sum_d, s2 += p.sum_d2, mx = fmax(mx, p.max_d2), within += p.within, fin += p.finite;
    }
    sd = wave_sum_d(sd), s2 = wave_sum_d(s2), mx = wave_max_d(mx);
    within = wave_sum_u64(within), fin = wave_sum_u64(fin);
    if (threadIdx.x == 0) *rec = mipsf_eval_stats_record{sd, s2, mx, within, fin, {0, 0, 0}};
}

inline uint32_t stats_blocks(uint32_t n) { return n ? min(blocks_for(n, TPB), STATS_MAX_BLOCKS) : 0u; }

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_eval_workspace_bytes(int which, uint32_t n) {
    switch (which) {
        case MIPSF_EVAL_WS_SAMPLE:
            return n <= MIPSF_EVAL_MAX_FACES ? sample_layout(n).bytes : 0;
        case MIPSF_EVAL_WS_STATS:
            return (uint64_t)(stats_blocks(n) ? stats_blocks(n) : 1u) * sizeof(StatsPartial);
        default:
            return 0;
    }
}

extern "C" int mipsf_eval_sample(const mipsf_eval_sample_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_eval_sample_args, "mipsf_eval_sample");
    MIPSF_REQUIRE(a->F > 0, "mipsf_eval_sample: a mesh without faces has no surface to sample");
    MIPSF_REQUIRE(a->F <= MIPSF_EVAL_MAX_FACES, "mipsf_eval_sample: %u faces, at most %u", a->F, MIPSF_EVAL_MAX_FACES);
    MIPSF_REQUIRE(a->n <= MIPSF_EVAL_MAX_SAMPLES, "mipsf_eval_sample: %u samples, at most %u", a->n, MIPSF_EVAL_MAX_SAMPLES);
    MIPSF_REQUIRE(a->faces && a->record && a->workspace && (a->vertices || a->V == 0), "mipsf_eval_sample: null pointer");
    MIPSF_REQUIRE((a->points && a->face_of) || a->n == 0, "mipsf_eval_sample: null output");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_eval_sample: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const SampleLayout L = sample_layout(a->F);
    uint64_t* cum = (uint64_t*)((char*)a->workspace + L.cum);
    uint64_t* tiles = (uint64_t*)((char*)a->workspace + L.tiles);
    const MeshView m = {a->vertices, a->faces, a->V, a->F};
    hipLaunchKernelGGL(eval_units_kernel, dim3(L.nb), dim3(TPB), 0, s, m, cum, tiles, L.nb);
    hipLaunchKernelGGL(eval_scan_top_kernel, dim3(1), dim3(TPB), 0, s, tiles, L.nb, a->record);
    hipLaunchKernelGGL(eval_scan_apply_kernel, dim3(L.nb), dim3(TPB), 0, s, cum, a->F, (const uint64_t*)tiles);
    if (a->n)
        hipLaunchKernelGGL(eval_draw_kernel, dim3(blocks_for(a->n, TPB)), dim3(TPB), 0, s, m, (const uint64_t*)cum,
                           (const mipsf_eval_sample_record*)a->record, a->n, a->seed, a->points, a->face_of);
    return check_launch("eval_sample");
}

extern "C" int mipsf_eval_nearest(const mipsf_eval_nearest_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_eval_nearest_args, "mipsf_eval_nearest");
    if (a->n_source == 0) return 0;
    MIPSF_REQUIRE(a->source && a->grid && a->index && a->d2, "mipsf_eval_nearest: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->grid & 15u) == 0, "mipsf_eval_nearest: grid not 16-byte aligned");
    MIPSF_REQUIRE(a->n_source <= MIPSF_ICP_MAX_POINTS && a->n_target <= MIPSF_ICP_MAX_POINTS, "mipsf_eval_nearest: too many points");
    MIPSF_REQUIRE(a->max_cells >= 1 && a->max_cells <= MIPSF_ICP_MAX_CELLS, "mipsf_eval_nearest: max_cells %u", a->max_cells);
    hipLaunchKernelGGL(eval_nearest_kernel, dim3(blocks_for(a->n_source, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->source, a->n_source,
                       a->n_target, grid_view(a->grid, a->n_target, a->max_cells), a->index, a->d2);
    return check_launch("eval_nearest");
}

extern "C" int mipsf_eval_stats(const mipsf_eval_stats_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_eval_stats_args, "mipsf_eval_stats");
    MIPSF_REQUIRE(a->record && a->workspace && (a->d2 || a->n == 0), "mipsf_eval_stats: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_eval_stats: workspace not 16-byte aligned");
    MIPSF_REQUIRE(a->threshold >= 0.0 && a->threshold < INFINITY, "mipsf_eval_stats: threshold %g", a->threshold);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nb = stats_blocks(a->n);
    StatsPartial* part = (StatsPartial*)a->workspace;
    if (nb) hipLaunchKernelGGL(eval_stats_partial_kernel, dim3(nb), dim3(TPB), 0, s, a->d2, a->n, a->threshold * a->threshold, part);
    hipLaunchKernelGGL(eval_stats_finish_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, (const StatsPartial*)part, nb, a->record);
    return check_launch("eval_stats");
}
