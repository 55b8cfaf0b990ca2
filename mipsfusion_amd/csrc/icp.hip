// Rectifying the pose of a switch back to an earlier sub-map (include/mipsf_icp.h): clouds from ray rows, a uniform grid over a
// cloud, exact nearest neighbours, normals from the 30 nearest neighbours, point-to-plane ICP.  Upstream: PoseCorrector.py, which
// calls open3d's estimate_normals() and registration_icp().  DESIGN.md 4.14.
//
// Shape of the kernels: one point per lane.  A cloud is sorted into cells of a uniform grid (count, scan, scatter; 16 bytes per
// sorted point: x, y, z and the original index), z runs fastest, so the cells (x, y, z0..z1) hold one contiguous run of points.
// Every comparison is on float64 squared distances ordered by (distance, original index): neither the edge of the cells nor the
// order of the points inside a cell (the scatter's integer atomics decide it) reaches a result.  Sums that feed a result are
// added in a fixed order: lane -> wave (cross-lane moves) -> block partials in a buffer -> one finishing wave.  The library is
// built with -ffp-contract=off.
#include "block_dev.h"
#include "icp_dev.h"
#include "icp_grid.h"
#include "../../include/mipsf_icp.h"

namespace mipsf {
namespace {

constexpr int TPB = GRID_TPB;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr int SCAN_TILE = GRID_SCAN_TILE; // entries one block scans
static_assert(SCAN_TILE == TPB * SCAN_ITEMS, "the grid's layout counts the tiles of block_dev.h's scan");
constexpr int KNN = MIPSF_ICP_KNN;

// ------------------------------------------------------------------------------------------------ exclusive scan of uint32
__global__ void __launch_bounds__(TPB) scan_sums_kernel(const uint32_t* in, uint32_t n, uint32_t* bsum) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t total = scan_tile_sum<WAVES>(in, n, sm);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum[0..nb) becomes its exclusive scan, *total_out the sum
__global__ void __launch_bounds__(TPB) scan_top_kernel(uint32_t* bsum, uint32_t nb, uint32_t* total_out) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t total = scan_top<WAVES>(bsum, nb, sm);
    if (threadIdx.x == 0 && total_out) *total_out = total;
}

// out may be in
__global__ void __launch_bounds__(TPB) scan_apply_kernel(const uint32_t* in, uint32_t n, const uint32_t* bsum, uint32_t* out) {
    __shared__ uint32_t sm[WAVES];
    scan_apply<WAVES, false>(in, n, bsum, out, sm);
}

// exclusive scan of in[0..n) into out (may alias), the sum into *total_out (optional); bsum: blocks_for(n, SCAN_TILE) words
void enqueue_scan(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* bsum, uint32_t* total_out, hipStream_t s) {
    const uint32_t nb = blocks_for(n, SCAN_TILE);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(TPB), 0, s, in, n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(TPB), 0, s, bsum, nb, total_out);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(TPB), 0, s, in, n, (const uint32_t*)bsum, out);
}

// ------------------------------------------------------------------------------------------------ cloud
struct CloudCfg {
    const float* rows;
    const int32_t* owner;
    const float* poses;
    uint32_t n, k, rows_per_owner;
};

__device__ __forceinline__ bool cloud_keep(const CloudCfg& c, uint32_t i, uint32_t& o) {
    o = c.owner ? (uint32_t)c.owner[i] : i / c.rows_per_owner;
    return c.rows[(size_t)i * 7 + 6] > 0.0f && o < c.k;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) cloud_flag_kernel(CloudCfg c, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= c.n) return;
    uint32_t o;
    flags[i] = cloud_keep(c, i, o) ? 1u : 0u;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) cloud_emit_kernel(CloudCfg c, const uint32_t* __restrict__ offsets,
                                                                           float* __restrict__ points) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= c.n) return;
    uint32_t o;
    if (!cloud_keep(c, i, o)) return;
    const float* r = c.rows + (size_t)i * 7;
    const float* P = c.poses + (size_t)o * 16;
    const float dx = r[0], dy = r[1], dz = r[2], depth = r[6];
    float* out = points + (size_t)offsets[i] * 3;      // offsets[i] <= i < n
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float dw = (dx * P[4 * d] + dy * P[4 * d + 1]) + dz * P[4 * d + 2];
        out[d] = P[4 * d + 3] + dw * depth;
    }
}

// ------------------------------------------------------------------------------------------------ grid (its layout: icp_grid.h)
// a box {min x y z, max x y z} over the wave, in every lane
__device__ __forceinline__ void box_wave_reduce(float v[6]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        v[d] = wave_reduce(v[d], [](float a, float b) { return fminf(a, b); });
        v[3 + d] = wave_reduce(v[3 + d], [](float a, float b) { return fmaxf(a, b); });
    }
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) bbox_partial_kernel(const float* __restrict__ pts, uint32_t n,
                                                                             float* __restrict__ part) {
    __shared__ float sm[WAVES][6];
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = v[3 + d] = pts[(size_t)i * 3 + d];
    }
    box_wave_reduce(v);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int d = 0; d < 6; ++d) sm[threadIdx.x >> 6][d] = v[d];
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = sm[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) r = threadIdx.x < 3 ? fminf(r, sm[w][threadIdx.x]) : fmaxf(r, sm[w][threadIdx.x]);
        part[(size_t)blockIdx.x * 6 + threadIdx.x] = r;
    }
}

// one wave: the box of the cloud and the grid over it
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) bbox_finish_kernel(const float* __restrict__ part, uint32_t nb, uint32_t n,
                                                                                   double min_edge, uint32_t max_cells, GridHdr* h) {
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t b = threadIdx.x; b < nb; b += MIPSF_WAVE)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            v[d] = fminf(v[d], part[(size_t)b * 6 + d]);
            v[3 + d] = fmaxf(v[3 + d], part[(size_t)b * 6 + 3 + d]);
        }
    box_wave_reduce(v);
    if (threadIdx.x != 0) return;
    double ext[3] = {0.0, 0.0, 0.0};
    if (n > 0)
        for (int d = 0; d < 3; ++d) ext[d] = (double)v[3 + d] - (double)v[d];
    double e = min_edge;
    if (!(e > 0.0)) {
        // points of a surface: about 8 per occupied cell when the surface is as large as the box's
        const double area = 2.0 * ((ext[0] * ext[1] + ext[1] * ext[2]) + ext[2] * ext[0]);
        const double longest = fmax(ext[0], fmax(ext[1], ext[2]));
        e = sqrt(8.0 * area / (double)(n ? n : 1));
        if (!(e > longest / 1024.0)) e = longest / 1024.0;
        if (!(e > 0.0) || !(e < INFINITY)) e = 1.0;
    }
    uint32_t dims[3] = {1, 1, 1};
    bool fits = false;
    for (int it = 0; it < 4096 && !fits; ++it) {
        double prod = 1.0;
        for (int d = 0; d < 3; ++d) {
            const double c = floor(ext[d] / e);
            dims[d] = c < 1.0e9 ? (uint32_t)c + 1u : 1000000000u;      // NaN -> the cap, which never fits
            prod *= (double)dims[d];
        }
        fits = prod <= (double)max_cells;
        if (!fits) e *= 1.25;
    }
    if (!fits) dims[0] = dims[1] = dims[2] = 1;
    for (int d = 0; d < 3; ++d) {
        h->origin[d] = n > 0 ? (double)v[d] : 0.0;
        h->dims[d] = dims[d];
    }
    h->edge = e;
    h->ncells = dims[0] * dims[1] * dims[2];
}

__device__ __forceinline__ uint32_t cell_index(const GridHdr& h, double x, double y, double z) {
    const uint32_t cx = cell_of(x, h.origin[0], h.edge, h.dims[0]), cy = cell_of(y, h.origin[1], h.edge, h.dims[1]),
                   cz = cell_of(z, h.origin[2], h.edge, h.dims[2]);
    return (cx * h.dims[1] + cy) * h.dims[2] + cz;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) bin_count_kernel(const float* __restrict__ pts, uint32_t n, const GridHdr* hp,
                                                                          uint32_t* cnt) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const GridHdr h = *hp;
    atomicAdd(&cnt[cell_index(h, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2])], 1u);
}

// cnt goes back to zero; start[c] + (what was left of cnt[c]) - 1 < start[c + 1] <= n
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) bin_scatter_kernel(const float* __restrict__ pts, uint32_t n, const GridHdr* hp,
                                                                            const uint32_t* __restrict__ start, uint32_t* cnt,
                                                                            float4* __restrict__ sorted) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const GridHdr h = *hp;
    const float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    const uint32_t c = cell_index(h, x, y, z);
    const uint32_t slot = start[c] + (atomicSub(&cnt[c], 1u) - 1u);
    if (slot < n) sorted[slot] = make_float4(x, y, z, __uint_as_float(i));
}

struct Best {
    double d2;
    uint32_t j;
    float x, y, z;
};

// The nearest target point among the cells within one cell of q's own (unclamped) cell: with an edge above max_dist that is every
// point within max_dist.  Cells outside the grid hold nothing.
__device__ __forceinline__ Best nearest_in_reach(const GridHdr& h, const Grid& g, uint32_t n_target, double qx, double qy, double qz) {
    Best b = {INFINITY, 0xffffffffu, 0.f, 0.f, 0.f};
    const double q[3] = {qx, qy, qz};
    int lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double f = floor((q[d] - h.origin[d]) / h.edge), top = (double)h.dims[d] + 1.0;
        const int t = f > -2.0 ? (f < top ? (int)f : (int)h.dims[d] + 1) : -2;      // NaN -> -2: an empty range
        lo[d] = t - 1 > 0 ? t - 1 : 0;
        hi[d] = t + 1 < (int)h.dims[d] - 1 ? t + 1 : (int)h.dims[d] - 1;
    }
    if (lo[2] > hi[2]) return b;
    for (int x = lo[0]; x <= hi[0]; ++x)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            const uint32_t row = ((uint32_t)x * h.dims[1] + (uint32_t)y) * h.dims[2];
            const uint32_t s = g.start[row + lo[2]], e = min(g.start[row + hi[2] + 1], n_target);
            for (uint32_t p = s; p < e; ++p) {
                const float4 v = g.sorted[p];
                const double d2 = dist2(qx, qy, qz, v);
                const uint32_t j = __float_as_uint(v.w);
                if (d2 < b.d2 || (d2 == b.d2 && j < b.j)) b = Best{d2, j, v.x, v.y, v.z};
            }
        }
    return b;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) nearest_kernel(const float* __restrict__ src, uint32_t n_source, uint32_t n_target,
                                                                        Grid g, double maxd2, int32_t* __restrict__ partner,
                                                                        double* __restrict__ d2_out) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n_source) return;
    const GridHdr h = *g.hdr;
    const Best b = nearest_in_reach(h, g, n_target, src[(size_t)i * 3], src[(size_t)i * 3 + 1], src[(size_t)i * 3 + 2]);
    const bool pair = b.j < n_target && b.d2 <= maxd2;
    partner[i] = pair ? (int32_t)b.j : -1;
    if (d2_out) d2_out[i] = pair ? b.d2 : (double)INFINITY;
}

// ------------------------------------------------------------------------------------------------ normals
// The unit eigenvector of the smallest eigenvalue of a symmetric 3x3 matrix, closed form in float64 (the non-iterative scheme of
// D. Eberly, "A Robust Eigensolver for 3x3 Symmetric Matrices": eigenvalues by the trigonometric formula on the scaled matrix, the
// vector of the better separated end of the spectrum from the largest cross product of two rows of A - l I, the others in the
// plane orthogonal to it).  false: no direction (zero matrix, or A - l I of rank below 2 where a direction was needed).
struct Vec3 {
    double x, y, z;
};
__device__ __forceinline__ Vec3 cross3(const Vec3& a, const Vec3& b) { return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot3(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ bool eigvec_by_rows(double a00, double a01, double a02, double a11, double a12, double a22, double l, Vec3& out) {
    const Vec3 r0 = {a00 - l, a01, a02}, r1 = {a01, a11 - l, a12}, r2 = {a02, a12, a22 - l};
    const Vec3 c01 = cross3(r0, r1), c02 = cross3(r0, r2), c12 = cross3(r1, r2);
    const double d01 = dot3(c01, c01), d02 = dot3(c02, c02), d12 = dot3(c12, c12);
    double dm = d01;
    Vec3 c = c01;
    if (d02 > dm) dm = d02, c = c02;
    if (d12 > dm) dm = d12, c = c12;
    if (!(dm > 0.0)) return false;
    const double inv = 1.0 / sqrt(dm);
    out = Vec3{c.x * inv, c.y * inv, c.z * inv};
    return true;
}

// the eigenvector of eigenvalue l in the plane orthogonal to the unit eigenvector w
__device__ __forceinline__ Vec3 eigvec_in_complement(double a00, double a01, double a02, double a11, double a12, double a22, const Vec3& w,
                                                     double l, Vec3& u_out) {
    Vec3 u;
    if (fabs(w.x) > fabs(w.y)) {
        const double inv = 1.0 / sqrt(w.x * w.x + w.z * w.z);
        u = Vec3{-w.z * inv, 0.0, w.x * inv};
    } else {
        const double inv = 1.0 / sqrt(w.y * w.y + w.z * w.z);
        u = Vec3{0.0, w.z * inv, -w.y * inv};
    }
    const Vec3 v = cross3(w, u);
    const Vec3 au = {(a00 * u.x + a01 * u.y) + a02 * u.z, (a01 * u.x + a11 * u.y) + a12 * u.z, (a02 * u.x + a12 * u.y) + a22 * u.z};
    const Vec3 av = {(a00 * v.x + a01 * v.y) + a02 * v.z, (a01 * v.x + a11 * v.y) + a12 * v.z, (a02 * v.x + a12 * v.y) + a22 * v.z};
    double m00 = dot3(u, au) - l, m01 = dot3(u, av), m11 = dot3(v, av) - l;
    const double b00 = fabs(m00), b01 = fabs(m01), b11 = fabs(m11);
    u_out = u;
    if (b00 >= b11) {
        if (!(fmax(b00, b01) > 0.0)) return u;
        if (b00 >= b01) {
            m01 /= m00;
            m00 = 1.0 / sqrt(1.0 + m01 * m01);
            m01 *= m00;
        } else {
            m00 /= m01;
            m01 = 1.0 / sqrt(1.0 + m00 * m00);
            m00 *= m01;
        }
        return Vec3{m01 * u.x - m00 * v.x, m01 * u.y - m00 * v.y, m01 * u.z - m00 * v.z};
    }
    if (!(fmax(b11, b01) > 0.0)) return u;
    if (b11 >= b01) {
        m01 /= m11;
        m11 = 1.0 / sqrt(1.0 + m01 * m01);
        m01 *= m11;
    } else {
        m11 /= m01;
        m01 = 1.0 / sqrt(1.0 + m11 * m11);
        m11 *= m01;
    }
    return Vec3{m11 * u.x - m01 * v.x, m11 * u.y - m01 * v.y, m11 * u.z - m01 * v.z};
}

__device__ __forceinline__ bool smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, Vec3& out) {
    const double big = fmax(fmax(fabs(a00), fmax(fabs(a01), fabs(a02))), fmax(fabs(a11), fmax(fabs(a12), fabs(a22))));
    if (!(big > 0.0) || !(big < INFINITY)) return false;
    const double s = 1.0 / big;
    a00 *= s, a01 *= s, a02 *= s, a11 *= s, a12 *= s, a22 *= s;
    const double norm = (a01 * a01 + a02 * a02) + a12 * a12;
    if (!(norm > 0.0)) {       // diagonal: the axis of the smallest entry, z first among equals
        if (a22 <= a00 && a22 <= a11) out = Vec3{0.0, 0.0, 1.0};
        else if (a11 <= a00) out = Vec3{0.0, 1.0, 0.0};
        else out = Vec3{1.0, 0.0, 0.0};
        return true;
    }
    const double q = ((a00 + a11) + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p = sqrt((((b00 * b00 + b11 * b11) + b22 * b22) + 2.0 * norm) / 6.0);
    const double c00 = b11 * b22 - a12 * a12, c01 = a01 * b22 - a12 * a02, c02 = a01 * a12 - b11 * a02;
    const double det = ((b00 * c00 - a01 * c01) + a02 * c02) / (p * p * p);
    const double half = fmin(fmax(0.5 * det, -1.0), 1.0);
    const double angle = acos(half) / 3.0;
    const double beta2 = 2.0 * cos(angle), beta0 = 2.0 * cos(angle + 2.0943951023931954923), beta1 = -(beta0 + beta2);
    const double l0 = q + p * beta0, l1 = q + p * beta1, l2 = q + p * beta2;
    if (half < 0.0) return eigvec_by_rows(a00, a01, a02, a11, a12, a22, l0, out);      // l0 is the better separated end
    Vec3 w2, u;
    if (!eigvec_by_rows(a00, a01, a02, a11, a12, a22, l2, w2)) return false;
    const Vec3 w1 = eigvec_in_complement(a00, a01, a02, a11, a12, a22, w2, l1, u);
    out = cross3(w1, w2);
    return true;
}

struct Knn {        // a lane's sorted candidate list in LDS, lane-minor
    double* d2;
    uint32_t* id;
    int cnt, cap;
    __device__ __forceinline__ double& D(int j) { return d2[j * MIPSF_WAVE]; }
    __device__ __forceinline__ uint32_t& I(int j) { return id[j * MIPSF_WAVE]; }
    __device__ __forceinline__ void offer(double d, uint32_t i) {
        if (cnt == cap) {
            const double dk = D(cap - 1);
            if (d > dk || (d == dk && i > I(cap - 1))) return;
        }
        int j = cnt < cap ? cnt : cap - 1;       // the slot that opens
        while (j > 0 && (D(j - 1) > d || (D(j - 1) == d && I(j - 1) > i))) {
            D(j) = D(j - 1);
            I(j) = I(j - 1);
            --j;
        }
        D(j) = d;
        I(j) = i;
        if (cnt < cap) ++cnt;
    }
};

__device__ __forceinline__ void knn_run(Knn& k, const Grid& g, uint32_t n, uint32_t c0, uint32_t c1, double qx, double qy, double qz) {
    const uint32_t s = g.start[c0], e = min(g.start[c1 + 1], n);
    for (uint32_t p = s; p < e; ++p) {
        const float4 v = g.sorted[p];
        k.offer(dist2(qx, qy, qz, v), __float_as_uint(v.w));
    }
}

// Lanes take the points in the grid's order (neighbours in space share cells).  Rings of cells around the point's own are scanned
// until the list is full and its last distance lies within the scanned cube, whose faces are at least ring * edge away.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) normals_kernel(const float* __restrict__ pts, uint32_t n, Grid g,
                                                                               double* __restrict__ normals,
                                                                               int32_t* __restrict__ neighbours) {
    __shared__ double s_d2[KNN * MIPSF_WAVE];
    __shared__ uint32_t s_id[KNN * MIPSF_WAVE];
    const uint32_t sidx = blockIdx.x * MIPSF_WAVE + threadIdx.x;
    if (sidx >= n) return;
    const GridHdr h = *g.hdr;
    const float4 me = g.sorted[sidx];
    const uint32_t self = __float_as_uint(me.w);
    if (self >= n) return;
    double* out = normals + (size_t)self * 3;
    out[0] = 0.0, out[1] = 0.0, out[2] = 1.0;
    const double qx = me.x, qy = me.y, qz = me.z;
    Knn k = {s_d2 + threadIdx.x, s_id + threadIdx.x, 0, (int)(n < (uint32_t)KNN ? n : (uint32_t)KNN)};
    const int dx = (int)h.dims[0], dy = (int)h.dims[1], dz = (int)h.dims[2];
    const int cx = (int)cell_of(qx, h.origin[0], h.edge, h.dims[0]), cy = (int)cell_of(qy, h.origin[1], h.edge, h.dims[1]),
              cz = (int)cell_of(qz, h.origin[2], h.edge, h.dims[2]);
    const int reach = max(max(max(cx, dx - 1 - cx), max(cy, dy - 1 - cy)), max(cz, dz - 1 - cz));
    for (int r = 0;; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
        for (int x = x0; x <= x1; ++x)
            for (int y = y0; y <= y1; ++y) {
                const uint32_t row = ((uint32_t)x * h.dims[1] + (uint32_t)y) * h.dims[2];
                if (x - cx == r || cx - x == r || y - cy == r || cy - y == r) {
                    knn_run(k, g, n, row + z0, row + z1, qx, qy, qz);
                } else {
                    if (cz - r >= 0) knn_run(k, g, n, row + (cz - r), row + (cz - r), qx, qy, qz);
                    if (cz + r <= dz - 1) knn_run(k, g, n, row + (cz + r), row + (cz + r), qx, qy, qz);
                }
            }
        if (r >= reach) break;
        const double covered = (double)r * h.edge * (1.0 - 1.0e-6);
        if (k.cnt == k.cap && k.D(k.cap - 1) <= covered * covered) break;
    }
    if (neighbours)
        for (int j = 0; j < KNN; ++j) neighbours[(size_t)self * KNN + j] = j < k.cnt ? (int32_t)k.I(j) : -1;
    if (k.cnt < 3) return;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int j = 0; j < k.cnt; ++j) {
        const float* p = pts + (size_t)min(k.I(j), n - 1) * 3;
        mx += (double)p[0], my += (double)p[1], mz += (double)p[2];
    }
    const double inv = 1.0 / (double)k.cnt;
    mx *= inv, my *= inv, mz *= inv;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int j = 0; j < k.cnt; ++j) {
        const float* p = pts + (size_t)min(k.I(j), n - 1) * 3;
        const double ex = (double)p[0] - mx, ey = (double)p[1] - my, ez = (double)p[2] - mz;
        a00 += ex * ex, a01 += ex * ey, a02 += ex * ez, a11 += ey * ey, a12 += ey * ez, a22 += ez * ez;
    }
    Vec3 v;
    if (!smallest_eigvec(a00 * inv, a01 * inv, a02 * inv, a11 * inv, a12 * inv, a22 * inv, v)) return;
    const double len = sqrt(dot3(v, v));
    if (!(len > 0.0) || !(len < INFINITY)) return;
    out[0] = v.x / len, out[1] = v.y / len, out[2] = v.z / len;
}

// ------------------------------------------------------------------------------------------------ registration
// IcpState, the sum layout and the finish step: icp_dev.h
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) icp_init_kernel(const float* __restrict__ src, uint32_t n3, double* __restrict__ P,
                                                                         IcpState* st, double* __restrict__ result) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < n3) P[i] = (double)src[i];
    if (i == 0) {
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) st->T[4 * r + c] = r == c ? 1.0 : 0.0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) st->U[4 * r + c] = r == c ? 1.0 : 0.0;
        st->prev_fitness = st->prev_rmse = 0.0;
        st->done = 0u, st->iter = 0u;
        for (int j = 0; j < (int)MIPSF_ICP_RESULT_DOUBLES; ++j) result[j] = 0.0;
    }
}

// One evaluation: move the points by the last update, pair each with its nearest target point within max_dist, and leave the
// block's sums of the normal equations in partial[block][NSUM_PAD].
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) icp_pair_kernel(double* __restrict__ P, uint32_t n_source, uint32_t n_target, Grid g,
                                                                         const double* __restrict__ normals, double maxd2,
                                                                         const IcpState* st, int apply, double* __restrict__ partial,
                                                                         int32_t* __restrict__ partner) {
    if (st->done) return;
    __shared__ double sm[WAVES][NSUM_PAD];
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    double c[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) c[k] = 0.0;
    if (i < n_source) {
        double px = P[(size_t)i * 3], py = P[(size_t)i * 3 + 1], pz = P[(size_t)i * 3 + 2];
        if (apply) {
            const double* U = st->U;
            const double nx = ((U[0] * px + U[1] * py) + U[2] * pz) + U[3];
            const double ny = ((U[4] * px + U[5] * py) + U[6] * pz) + U[7];
            const double nz = ((U[8] * px + U[9] * py) + U[10] * pz) + U[11];
            px = nx, py = ny, pz = nz;
            P[(size_t)i * 3] = px, P[(size_t)i * 3 + 1] = py, P[(size_t)i * 3 + 2] = pz;
        }
        const GridHdr h = *g.hdr;
        const Best b = nearest_in_reach(h, g, n_target, px, py, pz);
        const bool pair = b.j < n_target && b.d2 <= maxd2;
        if (partner) partner[i] = pair ? (int32_t)b.j : -1;
        if (pair) {
            const double* nn = normals + (size_t)b.j * 3;
            const double nx = nn[0], ny = nn[1], nz = nn[2];
            const double r = (((px - (double)b.x) * nx + (py - (double)b.y) * ny) + (pz - (double)b.z) * nz);
            icp_pair_sums(c, px, py, pz, nx, ny, nz, r, b.d2);
        }
    }
    icp_block_sums<WAVES, NSUM>(c, sm, partial);
}

// One wave: add the partials in index order, judge the evaluation, and -- unless it was the last -- solve for the next update.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) icp_finish_kernel(const double* __restrict__ partial, uint32_t nb, uint32_t n_source,
                                                                                  IcpState* st, uint32_t max_iteration, double rel_fitness,
                                                                                  double rel_rmse, double* __restrict__ result) {
    if (st->done) return;
    icp_finish<NSUM>(partial, nb, n_source, st, max_iteration, rel_fitness, rel_rmse, result);
}

struct RegLayout {
    uint64_t state, P, partial, bytes;
};
RegLayout reg_layout(uint32_t n_source) {
    RegLayout L;
    L.state = 0;
    L.P = 256;
    L.partial = align16(L.P + (uint64_t)(n_source ? n_source : 1) * 3 * sizeof(double));
    L.bytes = L.partial + (uint64_t)blocks_for(n_source ? n_source : 1, TPB) * NSUM_PAD * sizeof(double);
    return L;
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_icp_workspace_bytes(int which, uint32_t n, uint32_t cells) {
    if (n > MIPSF_ICP_MAX_POINTS) return 0;
    switch (which) {
        case MIPSF_ICP_WS_CLOUD:
            return align16((uint64_t)(n ? n : 1) * 4) + align16((uint64_t)blocks_for(n ? n : 1, SCAN_TILE) * 4);
        case MIPSF_ICP_WS_GRID:
            if (cells == 0 || cells > MIPSF_ICP_MAX_CELLS) return 0;
            return grid_layout(n, cells).bytes;
        case MIPSF_ICP_WS_REGISTER:
            return reg_layout(n).bytes;
        default:
            return 0;
    }
}

extern "C" int mipsf_icp_cloud(const mipsf_icp_cloud_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_icp_cloud_args, "mipsf_icp_cloud");
    MIPSF_REQUIRE(a->count != nullptr, "mipsf_icp_cloud: null count");
    MIPSF_REQUIRE(a->n <= MIPSF_ICP_MAX_POINTS, "mipsf_icp_cloud: %u rows, at most %u", a->n, MIPSF_ICP_MAX_POINTS);
    hipStream_t s = (hipStream_t)stream;
    if (a->n == 0) {
        if (hipMemsetAsync(a->count, 0, sizeof(uint32_t), s) != hipSuccess) {
            set_error("mipsf_icp_cloud: memset failed");
            return 1;
        }
        return 0;
    }
    MIPSF_REQUIRE(a->rows && a->poses && a->points && a->workspace, "mipsf_icp_cloud: null pointer");
    MIPSF_REQUIRE(a->k > 0, "mipsf_icp_cloud: no poses");
    MIPSF_REQUIRE(a->owner || a->rows_per_owner > 0, "mipsf_icp_cloud: neither owner nor rows_per_owner");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_icp_cloud: workspace not 16-byte aligned");
    uint32_t* flags = (uint32_t*)a->workspace;
    uint32_t* bsum = (uint32_t*)((char*)a->workspace + align16((uint64_t)a->n * 4));
    const CloudCfg c = {a->rows, a->owner, a->poses, a->n, a->k, a->rows_per_owner};
    hipLaunchKernelGGL(cloud_flag_kernel, dim3(blocks_for(a->n, TPB)), dim3(TPB), 0, s, c, flags);
    enqueue_scan(flags, a->n, flags, bsum, a->count, s);
    hipLaunchKernelGGL(cloud_emit_kernel, dim3(blocks_for(a->n, TPB)), dim3(TPB), 0, s, c, (const uint32_t*)flags, a->points);
    return check_launch("icp_cloud");
}

extern "C" int mipsf_icp_bin(const mipsf_icp_bin_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_icp_bin_args, "mipsf_icp_bin");
    MIPSF_REQUIRE(a->grid != nullptr && (a->points != nullptr || a->n == 0), "mipsf_icp_bin: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->grid & 15u) == 0, "mipsf_icp_bin: grid not 16-byte aligned");
    MIPSF_REQUIRE(a->n <= MIPSF_ICP_MAX_POINTS, "mipsf_icp_bin: %u points, at most %u", a->n, MIPSF_ICP_MAX_POINTS);
    MIPSF_REQUIRE(a->max_cells >= 1 && a->max_cells <= MIPSF_ICP_MAX_CELLS, "mipsf_icp_bin: max_cells %u outside 1 .. %u", a->max_cells,
                  MIPSF_ICP_MAX_CELLS);
    MIPSF_REQUIRE(a->min_edge >= 0.0 && a->min_edge < INFINITY, "mipsf_icp_bin: min_edge %g", a->min_edge);
    hipStream_t s = (hipStream_t)stream;
    const GridLayout L = grid_layout(a->n, a->max_cells);
    char* b = (char*)a->grid;
    GridHdr* hdr = (GridHdr*)(b + L.hdr);
    float* part = (float*)(b + L.bbox);
    uint32_t* start = (uint32_t*)(b + L.start);
    uint32_t* cnt = (uint32_t*)(b + L.cnt);
    uint32_t* bsum = (uint32_t*)(b + L.bsum);
    float4* sorted = (float4*)(b + L.sorted);
    const uint32_t nb = a->n ? blocks_for(a->n, TPB) : 0;
    if (hipMemsetAsync(cnt, 0, ((size_t)a->max_cells + 1) * 4, s) != hipSuccess) {
        set_error("mipsf_icp_bin: memset failed");
        return 1;
    }
    if (nb) hipLaunchKernelGGL(bbox_partial_kernel, dim3(nb), dim3(TPB), 0, s, a->points, a->n, part);
    hipLaunchKernelGGL(bbox_finish_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, (const float*)part, nb, a->n, a->min_edge, a->max_cells, hdr);
    if (nb) hipLaunchKernelGGL(bin_count_kernel, dim3(nb), dim3(TPB), 0, s, a->points, a->n, (const GridHdr*)hdr, cnt);
    enqueue_scan(cnt, a->max_cells + 1, start, bsum, nullptr, s);
    if (nb) hipLaunchKernelGGL(bin_scatter_kernel, dim3(nb), dim3(TPB), 0, s, a->points, a->n, (const GridHdr*)hdr, (const uint32_t*)start, cnt, sorted);
    return check_launch("icp_bin");
}

extern "C" int mipsf_icp_nearest(const mipsf_icp_nearest_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_icp_nearest_args, "mipsf_icp_nearest");
    if (a->n_source == 0) return 0;
    MIPSF_REQUIRE(a->source && a->grid && a->partner, "mipsf_icp_nearest: null pointer");
    MIPSF_REQUIRE(a->n_source <= MIPSF_ICP_MAX_POINTS && a->n_target <= MIPSF_ICP_MAX_POINTS, "mipsf_icp_nearest: too many points");
    MIPSF_REQUIRE(a->max_cells >= 1 && a->max_cells <= MIPSF_ICP_MAX_CELLS, "mipsf_icp_nearest: max_cells %u", a->max_cells);
    MIPSF_REQUIRE(a->max_dist >= 0.0 && a->max_dist < INFINITY, "mipsf_icp_nearest: max_dist %g", a->max_dist);
    hipLaunchKernelGGL(nearest_kernel, dim3(blocks_for(a->n_source, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->source, a->n_source, a->n_target,
                       grid_view(a->grid, a->n_target, a->max_cells), a->max_dist * a->max_dist, a->partner, a->d2);
    return check_launch("icp_nearest");
}

extern "C" int mipsf_icp_normals(const mipsf_icp_normals_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_icp_normals_args, "mipsf_icp_normals");
    if (a->n == 0) return 0;
    MIPSF_REQUIRE(a->points && a->grid && a->normals, "mipsf_icp_normals: null pointer");
    MIPSF_REQUIRE(a->n <= MIPSF_ICP_MAX_POINTS, "mipsf_icp_normals: too many points");
    MIPSF_REQUIRE(a->max_cells >= 1 && a->max_cells <= MIPSF_ICP_MAX_CELLS, "mipsf_icp_normals: max_cells %u", a->max_cells);
    hipLaunchKernelGGL(normals_kernel, dim3(blocks_for(a->n, MIPSF_WAVE)), dim3(MIPSF_WAVE), 0, (hipStream_t)stream, a->points, a->n,
                       grid_view(a->grid, a->n, a->max_cells), a->normals, a->neighbours);
    return check_launch("icp_normals");
}

extern "C" int mipsf_icp_register(const mipsf_icp_register_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_icp_register_args, "mipsf_icp_register");
    MIPSF_REQUIRE(a->result && a->workspace && a->grid, "mipsf_icp_register: null pointer");
    MIPSF_REQUIRE((a->source || a->n_source == 0) && (a->target_normals || a->n_target == 0), "mipsf_icp_register: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_icp_register: workspace not 16-byte aligned");
    MIPSF_REQUIRE(a->n_source <= MIPSF_ICP_MAX_POINTS && a->n_target <= MIPSF_ICP_MAX_POINTS, "mipsf_icp_register: too many points");
    MIPSF_REQUIRE(a->max_cells >= 1 && a->max_cells <= MIPSF_ICP_MAX_CELLS, "mipsf_icp_register: max_cells %u", a->max_cells);
    MIPSF_REQUIRE(a->max_dist >= 0.0 && a->max_dist < INFINITY, "mipsf_icp_register: max_dist %g", a->max_dist);
    MIPSF_REQUIRE(a->max_iteration <= 1000, "mipsf_icp_register: max_iteration %u above 1000", a->max_iteration);
    hipStream_t s = (hipStream_t)stream;
    const RegLayout L = reg_layout(a->n_source);
    char* w = (char*)a->workspace;
    IcpState* st = (IcpState*)(w + L.state);
    double* P = (double*)(w + L.P);
    double* partial = (double*)(w + L.partial);
    const Grid g = grid_view(a->grid, a->n_target, a->max_cells);
    const uint32_t nb = a->n_source ? blocks_for(a->n_source, TPB) : 0;
    hipLaunchKernelGGL(icp_init_kernel, dim3(blocks_for(a->n_source ? (uint64_t)a->n_source * 3 : 1, TPB)), dim3(TPB), 0, s, a->source,
                       a->n_source * 3, P, st, a->result);
    for (uint32_t k = 0; k <= a->max_iteration; ++k) {
        if (nb)
            hipLaunchKernelGGL(icp_pair_kernel, dim3(nb), dim3(TPB), 0, s, P, a->n_source, a->n_target, g, a->target_normals,
                               a->max_dist * a->max_dist, (const IcpState*)st, k > 0 ? 1 : 0, partial, a->partner);
        hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, (const double*)partial, nb, a->n_source, st, a->max_iteration,
                           a->relative_fitness, a->relative_rmse, a->result);
    }
    return check_launch("icp_register");
}
