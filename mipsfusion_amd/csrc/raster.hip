// A triangle mesh as per-pixel depth from a batch of poses, the L1 difference of two depth stacks, and the occlusion test of the
// culling (include/mipsf_raster.h).  Upstream has no evaluation code; the protocol is the published one of the NICE-SLAM /
// Co-SLAM evaluation, which renders with a host library.  DESIGN.md 4.18.
//
// Shape of the kernels: one (view, face) pair per lane counts the 8 x 8 tiles of the face's screen box; the counts become a
// 64-bit prefix sum (block_dev.h's device-wide scan); one wavefront takes one tile, one lane one pixel, finds its pair by binary
// search in the sum, recomputes the face's cross products and tests its pixel by the header's float64 rule; the winner of a pixel is the
// integer minimum of (depth bits, face index), so the image is the same in any order of work.  The screen box is the only
// arithmetic here that the header does not fix: it may be generous, it must never leave out a pixel the rule hits.
#include "block_dev.h"
#include "../../include/mipsf_raster.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr int SCAN_TILE = TPB * SCAN_ITEMS;     // items one block scans
constexpr uint32_t TILE = MIPSF_RASTER_TILE;
constexpr uint32_t L1_MAX_BLOCKS = 256;         // partials per view
constexpr uint64_t KEY_EMPTY = ~0ull;
static_assert(TILE * TILE == MIPSF_WAVE, "one lane per pixel of a tile");
static_assert(sizeof(mipsf_raster_l1_record) == 64, "l1 record");

// ------------------------------------------------------------------------------------------------ the face and its screen box
struct Scene {
    const float* vertices;
    const int32_t* faces;
    const float* poses;
    uint32_t V, F, n, H, W;
    double fx, fy, cx, cy, near, far;
};

struct Face {
    double R[9], A[3], nAB[3], nBC[3], nCA[3];
};

struct TileBox {
    uint32_t x0, y0, nx, ny;       // nx * ny tiles from tile (x0, y0); nx = 0: none
};

__host__ __device__ __forceinline__ void cross3(const double P[3], const double Q[3], double out[3]) {
    out[0] = P[1] * Q[2] - P[2] * Q[1];
    out[1] = P[2] * Q[0] - P[0] * Q[2];
    out[2] = P[0] * Q[1] - P[1] * Q[0];
}
__host__ __device__ __forceinline__ double dot3(const double d[3], const double n[3]) { return (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]; }
__host__ __device__ __forceinline__ double norm3(const double p[3]) { return sqrt(dot3(p, p)); }
__host__ __device__ __forceinline__ bool finite3(const double p[3]) { return fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY; }
__host__ __device__ __forceinline__ bool same3(const double p[3], const double q[3]) { return p[0] == q[0] && p[1] == q[1] && p[2] == q[2]; }

// The header's values of face f seen from `view` (R, A = v[a] - t, the three cross products) and the tiles its pixels can lie in.
//   none        an index outside [0, V); a vertex that is not finite (its cross products are not finite, so no edge value and no
//               `den` is); two equal vertices (one cross product is exactly 0 and the other two negate each other, so `inside`
//               needs all three edge values 0 and then den = 0); every vertex behind the camera (tt is negative: below)
//   everything  the plane of the face passes through the camera to 1e-10 of the face's distance (num and den are then both
//               rounding residue and tt may be any number along the line the face is seen as); a pose whose R has no inverse to
//               speak of; a vertex within 1e-6 of the face's extent of the camera plane (which side it is on is not certain)
//   else        the box of what lies in front of the camera, a pixel wider on every side.  That part of the face projects to the
//               convex hull of the front vertices' projections and, for every edge that crosses the camera plane, the point at
//               infinity in the direction (x, y) of the crossing point: the edge from a front vertex V to a crossing point c
//               projects to the straight ray from V's pixel along c.xy.  So the box runs from the front vertices' extremes to
//               the image's border on every side some crossing point lies on.  Most faces that cross the camera plane are 90
//               degrees off the axis and their box misses the image altogether.
// With the plane 1e-10 clear of the camera, den carries a relative error below 3e-6 |d| and every edge plane is turned by less
// than 1e-6 radians, a fraction of a pixel at any focal length below 1e5: tt has the sign of the true depth and the pixels the
// rule hits lie within the widened box.  The camera-frame coordinates come from the true inverse of R (adjugate over determinant),
// not its transpose, because the rule's rays are R d for whatever R the caller gives.
__host__ __device__ __forceinline__ TileBox face_setup(const Scene& s, uint32_t view, uint32_t f, Face& o) {
    const TileBox none = {0u, 0u, 0u, 0u};
    const TileBox all = {0u, 0u, (s.W + TILE - 1) / TILE, (s.H + TILE - 1) / TILE};
    const int32_t ia = s.faces[(size_t)f * 3], ib = s.faces[(size_t)f * 3 + 1], ic = s.faces[(size_t)f * 3 + 2];
    if (ia < 0 || ib < 0 || ic < 0 || (uint32_t)ia >= s.V || (uint32_t)ib >= s.V || (uint32_t)ic >= s.V) return none;
    const float* P = s.poses + (size_t)view * 16;
    double t[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.R[k * 3] = (double)P[k * 4], o.R[k * 3 + 1] = (double)P[k * 4 + 1], o.R[k * 3 + 2] = (double)P[k * 4 + 2];
        t[k] = (double)P[k * 4 + 3];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        o.A[d] = (double)s.vertices[(size_t)ia * 3 + d] - t[d];
        B[d] = (double)s.vertices[(size_t)ib * 3 + d] - t[d];
        C[d] = (double)s.vertices[(size_t)ic * 3 + d] - t[d];
    }
    cross3(o.A, B, o.nAB), cross3(B, C, o.nBC), cross3(C, o.A, o.nCA);
    if (!(finite3(o.A) && finite3(B) && finite3(C))) return none;
    if (same3(o.A, B) || same3(B, C) || same3(C, o.A)) return none;
    const double triple = dot3(o.A, o.nBC);
    if (!(fabs(triple) > 1.0e-10 * (norm3(o.A) * norm3(B) * norm3(C)))) return all;
    const double* r0 = o.R, *r1 = o.R + 3, *r2 = o.R + 6;
    double c0[3], c1[3], c2[3];                       // the columns of det * inverse(R)
    cross3(r1, r2, c0), cross3(r2, r0, c1), cross3(r0, r1, c2);
    const double det = dot3(r0, c0);
    if (!(fabs(det) > 1.0e-6 * (norm3(r0) * norm3(r1) * norm3(r2))) || !(fabs(det) < INFINITY)) return all;
    const double* Q[3] = {o.A, B, C};
    double px[3], py[3], z[3], extent = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = ((c0[0] * Q[k][0] + c1[0] * Q[k][1]) + c2[0] * Q[k][2]) / det;
        const double y = ((c0[1] * Q[k][0] + c1[1] * Q[k][1]) + c2[1] * Q[k][2]) / det;
        z[k] = -(((c0[2] * Q[k][0] + c1[2] * Q[k][1]) + c2[2] * Q[k][2]) / det);
        px[k] = x, py[k] = y;
        extent = fmax(extent, fmax(fabs(x), fmax(fabs(y), fabs(z[k]))));
    }
    const double margin = 1.0e-6 * extent;
    if (fmax(z[0], fmax(z[1], z[2])) < -margin) return none;
    bool front[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(fabs(z[k]) > margin)) return all;       // NaN too
        front[k] = z[k] > 0.0;
    }
    double xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (front[k]) {
            const double u = s.cx + s.fx * (px[k] / z[k]), v = s.cy - s.fy * (py[k] / z[k]);
            xlo = fmin(xlo, u), xhi = fmax(xhi, u), ylo = fmin(ylo, v), yhi = fmax(yhi, v);
        }
    const double tol = margin * extent;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int l = (k + 1) % 3;
        if (front[k] != front[l]) {                   // a crossing: a positive multiple of the point where the edge meets the plane
            const int a = front[k] ? k : l, b = front[k] ? l : k;
            const double du = px[a] * (-z[b]) + px[b] * z[a], dv = -(py[a] * (-z[b]) + py[b] * z[a]);
            if (du > -tol) xhi = INFINITY;
            if (du < tol) xlo = -INFINITY;
            if (dv > -tol) yhi = INFINITY;
            if (dv < tol) ylo = -INFINITY;
        }
    }
    xlo = floor(xlo) - 1.0, xhi = ceil(xhi) + 1.0, ylo = floor(ylo) - 1.0, yhi = ceil(yhi) + 1.0;
    if (!(xlo <= xhi && ylo <= yhi)) return all;      // a projection that is not a number
    xlo = fmax(xlo, 0.0), ylo = fmax(ylo, 0.0);
    xhi = fmin(xhi, (double)(s.W - 1)), yhi = fmin(yhi, (double)(s.H - 1));
    if (!(xlo <= xhi && ylo <= yhi)) return none;     // beside the image
    const uint32_t tx0 = (uint32_t)xlo / TILE, tx1 = (uint32_t)xhi / TILE, ty0 = (uint32_t)ylo / TILE, ty1 = (uint32_t)yhi / TILE;
    return TileBox{tx0, ty0, tx1 - tx0 + 1u, ty1 - ty0 + 1u};
}

// the header's test of pixel (row j, col i) against the face `o` holds the values of -> whether it hits, and its key
__host__ __device__ __forceinline__ bool pixel_key(const Scene& s, const Face& o, uint32_t f, uint32_t i, uint32_t j, uint64_t& key) {
    const double dx = ((double)i - s.cx) / s.fx;
    const double dy = -(((double)j - s.cy) / s.fy);
    double dw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dw[k] = (o.R[k * 3] * dx + o.R[k * 3 + 1] * dy) + o.R[k * 3 + 2] * (-1.0);
    const double e0 = dot3(dw, o.nAB), e1 = dot3(dw, o.nBC), e2 = dot3(dw, o.nCA);
    const bool inside = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    const double den = (e0 + e1) + e2;
    const double num = dot3(o.A, o.nBC);
    const double tt = num / den;
    const float d32 = (float)tt;
    key = ((uint64_t)__builtin_bit_cast(uint32_t, d32) << 32) | (uint64_t)f;
    return inside && den != 0.0 && tt > s.near && tt < s.far && d32 >= 0x1p-126f && d32 < INFINITY;
}

// ------------------------------------------------------------------------------------------------ depth of a mesh
__global__ void __launch_bounds__(TPB) raster_clear_kernel(uint64_t* __restrict__ keys, uint64_t pixels) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x; p < pixels; p += stride) keys[p] = KEY_EMPTY;
}

// item = view * F + face; cum[item] = its number of tiles, tiles[block] = the block's sum
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) raster_count_kernel(Scene s, uint32_t items, uint64_t* __restrict__ cum,
                                                                             uint64_t* __restrict__ tiles) {
    __shared__ uint64_t sm[WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint64_t sum = 0;
#pragma unroll 1
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < items) {
            const uint32_t item = (uint32_t)(base + k);
            Face face;
            const TileBox b = face_setup(s, item / s.F, item % s.F, face);
            const uint64_t c = (uint64_t)b.nx * b.ny;
            cum[item] = c;
            sum += c;
        }
    sum = block_reduce<WAVES>(sum, sm, Add());
    if (threadIdx.x == 0) tiles[blockIdx.x] = sum;
}

// one block: tiles[0..nb) becomes its exclusive scan
__global__ void __launch_bounds__(TPB) raster_scan_top_kernel(uint64_t* tiles, uint32_t nb) {
    __shared__ uint64_t sm[WAVES];
    scan_top<WAVES>(tiles, nb, sm);
}

// cum: the items' counts in, their inclusive prefix sum out
__global__ void __launch_bounds__(TPB) raster_scan_apply_kernel(uint64_t* cum, uint32_t items, const uint64_t* __restrict__ tiles) {
    __shared__ uint64_t sm[WAVES];
    scan_apply<WAVES, true>(cum, items, tiles, cum, sm);
}

// Wave w of the grid takes tiles w, w + waves, ...: tile number -> the first item with cum[item] > number -> the tile of that
// item's box -> lane l tests pixel (l % 8, l / 8) of it.  Reading the key before the atomic only skips keys that cannot win: a
// stale value is never smaller than the current one.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) raster_tiles_kernel(Scene s, uint32_t items, const uint64_t* __restrict__ cum,
                                                                             uint64_t* __restrict__ keys) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t total = cum[items - 1];
    const uint64_t waves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < total; w += waves) {
        uint32_t lo = 0, hi = items - 1;              // cum[items-1] = total > w
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cum[mid] > w) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t local = w - (lo ? cum[lo - 1] : 0ull);
        const uint32_t view = lo / s.F, f = lo % s.F;
        Face o;
        const TileBox b = face_setup(s, view, f, o);
        if (local >= (uint64_t)b.nx * b.ny) continue;
        const uint32_t i = (b.x0 + (uint32_t)(local % b.nx)) * TILE + (lane & 7u);
        const uint32_t j = (b.y0 + (uint32_t)(local / b.nx)) * TILE + (lane >> 3);
        if (i >= s.W || j >= s.H) continue;
        uint64_t key;
        if (pixel_key(s, o, f, i, j, key)) {
            uint64_t* p = keys + ((size_t)view * s.H + j) * s.W + i;
            if (key < *p) atomicMin((unsigned long long*)p, (unsigned long long)key);
        }
    }
}

__global__ void __launch_bounds__(TPB) raster_resolve_kernel(const uint64_t* __restrict__ keys, uint64_t pixels, float* __restrict__ depth,
                                                             int32_t* __restrict__ face) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t p = (uint64_t)blockIdx.x * TPB + threadIdx.x; p < pixels; p += stride) {
        const uint64_t key = keys[p];
        const bool hit = key != KEY_EMPTY;
        depth[p] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        face[p] = hit ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
    }
}

struct DepthLayout {
    uint64_t keys, cum, tiles, bytes;    // keys: uint64 [n*H*W]; cum: uint64 [n*F]; tiles: uint64 [nb]
    uint32_t nb, items;
    uint64_t pixels;
};
DepthLayout depth_layout(uint32_t n, uint32_t F, uint32_t H, uint32_t W) {
    DepthLayout L;
    L.pixels = (uint64_t)n * H * W;
    L.items = (uint32_t)((uint64_t)n * F);
    L.nb = blocks_for(L.items, SCAN_TILE);
    L.keys = 0;
    L.cum = align16(L.pixels * 8);
    L.tiles = align16(L.cum + (uint64_t)L.items * 8);
    L.bytes = L.tiles + (uint64_t)L.nb * 8;
    return L;
}
bool depth_in_range(uint32_t n, uint32_t F, uint32_t H, uint32_t W) {
    return n >= 1 && F >= 1 && H >= 1 && W >= 1 && H <= MIPSF_RASTER_MAX_SIDE && W <= MIPSF_RASTER_MAX_SIDE && F <= MIPSF_RASTER_MAX_FACES &&
           (uint64_t)n * H * W <= MIPSF_RASTER_MAX_PIXELS && (uint64_t)n * F <= MIPSF_RASTER_MAX_ITEMS;
}

// ------------------------------------------------------------------------------------------------ L1 of two depth stacks
struct L1Partial {
    double sum_all, sum_both;
    uint64_t both, rec_only, gt_only, neither;
    uint64_t pad[2];
};
static_assert(sizeof(L1Partial) == 64, "l1 partial");

// block (b, view), thread t takes pixels (b*TPB + t) + j * (blocks*TPB) of the view; butterfly over the wave; waves ascending
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) raster_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                                  uint32_t hw, L1Partial* __restrict__ part) {
    __shared__ L1Partial sm[WAVES];
    const size_t off = (size_t)blockIdx.y * hw;
    double sa = 0.0, sb = 0.0;
    uint64_t both = 0, ro = 0, go = 0, none = 0;
    const uint32_t stride = gridDim.x * TPB;
    for (uint32_t p = blockIdx.x * TPB + threadIdx.x; p < hw; p += stride) {
        const float x = a[off + p], y = b[off + p];
        const double d = fabs((double)x - (double)y);
        const bool hx = x != 0.0f, hy = y != 0.0f;
        sa += d;
        if (hx && hy) sb += d;
        both += (hx && hy) ? 1u : 0u, ro += (hx && !hy) ? 1u : 0u, go += (!hx && hy) ? 1u : 0u, none += (!hx && !hy) ? 1u : 0u;
    }
    sa = wave_sum_d(sa), sb = wave_sum_d(sb);
    both = wave_sum_u64(both), ro = wave_sum_u64(ro), go = wave_sum_u64(go), none = wave_sum_u64(none);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = L1Partial{sa, sb, both, ro, go, none, {0, 0}};
    __syncthreads();
    if (threadIdx.x == 0) {
        L1Partial p = sm[0];
        for (int w = 1; w < WAVES; ++w)
            p.sum_all += sm[w].sum_all, p.sum_both += sm[w].sum_both, p.both += sm[w].both, p.rec_only += sm[w].rec_only,
                p.gt_only += sm[w].gt_only, p.neither += sm[w].neither;
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// one wave per view: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) raster_l1_finish_kernel(const L1Partial* __restrict__ part, uint32_t nb,
                                                                                        mipsf_raster_l1_record* __restrict__ rec) {
    double sa = 0.0, sb = 0.0;
    uint64_t both = 0, ro = 0, go = 0, none = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += MIPSF_WAVE) {
        const L1Partial p = part[(size_t)blockIdx.x * nb + b];
        sa += p.sum_all, sb += p.sum_both, both += p.both, ro += p.rec_only, go += p.gt_only, none += p.neither;
    }
    sa = wave_sum_d(sa), sb = wave_sum_d(sb);
    both = wave_sum_u64(both), ro = wave_sum_u64(ro), go = wave_sum_u64(go), none = wave_sum_u64(none);
    if (threadIdx.x == 0) rec[blockIdx.x] = mipsf_raster_l1_record{sa, sb, both, ro, go, none, {0, 0}};
}

inline uint32_t l1_blocks(uint32_t H, uint32_t W) { return min(blocks_for((uint64_t)H * W, TPB), L1_MAX_BLOCKS); }
bool l1_in_range(uint32_t n, uint32_t H, uint32_t W) {
    return n >= 1 && n <= 65535u && H >= 1 && W >= 1 && H <= MIPSF_RASTER_MAX_SIDE && W <= MIPSF_RASTER_MAX_SIDE &&
           (uint64_t)n * H * W <= MIPSF_RASTER_MAX_PIXELS;
}

// ------------------------------------------------------------------------------------------------ which points some view sees
struct Views {
    const float* depth;
    const float* poses;
    const float* max_depth;
    uint32_t n, H, W;
    double fx, fy, cx, cy, edge, eps;
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) raster_visible_kernel(const float* __restrict__ points, uint32_t m, Views s,
                                                                               uint8_t* __restrict__ seen) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const double p[3] = {(double)points[(size_t)i * 3], (double)points[(size_t)i * 3 + 1], (double)points[(size_t)i * 3 + 2]};
    const double w_hi = (double)s.W - s.edge, h_hi = (double)s.H - s.edge;
    bool any = false;
    for (uint32_t k = 0; k < s.n && !any; ++k) {
        const float* P = s.poses + (size_t)k * 16;
        const double q[3] = {p[0] - (double)P[3], p[1] - (double)P[7], p[2] - (double)P[11]};
        double cam[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) cam[c] = ((double)P[c] * q[0] + (double)P[4 + c] * q[1]) + (double)P[8 + c] * q[2];
        const double z = -cam[2];
        const double u = s.cx + s.fx * (cam[0] / z);
        const double v = s.cy - s.fy * (cam[1] / z);
        if (!(z > 0.0 && z < (double)s.max_depth[k] && s.edge < u && u < w_hi && s.edge < v && v < h_hi)) continue;
        const double col = floor(u + 0.5), row = floor(v + 0.5);
        if (!(col >= 0.0 && col < (double)s.W && row >= 0.0 && row < (double)s.H)) continue;
        const float d = s.depth[((size_t)k * s.H + (uint32_t)row) * s.W + (uint32_t)col];
        any = d == 0.0f || z <= (double)d + s.eps;
    }
    seen[i] = any ? 1u : 0u;
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

static bool intrinsics_ok(double fx, double fy, double cx, double cy) {
    return fx > 0.0 && fx < INFINITY && fy > 0.0 && fy < INFINITY && fabs(cx) < INFINITY && fabs(cy) < INFINITY;
}

extern "C" uint64_t mipsf_raster_workspace_bytes(int which, uint32_t n, uint32_t F, uint32_t H, uint32_t W) {
    switch (which) {
        case MIPSF_RASTER_WS_DEPTH:
            return depth_in_range(n, F, H, W) ? depth_layout(n, F, H, W).bytes : 0;
        case MIPSF_RASTER_WS_L1:
            return l1_in_range(n, H, W) ? (uint64_t)n * l1_blocks(H, W) * sizeof(L1Partial) : 0;
        default:
            return 0;
    }
}

extern "C" int mipsf_raster_depth(const mipsf_raster_depth_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_raster_depth_args, "mipsf_raster_depth");
    MIPSF_REQUIRE(a->F > 0, "mipsf_raster_depth: a mesh without faces has nothing to render");
    MIPSF_REQUIRE(a->n > 0, "mipsf_raster_depth: no views");
    MIPSF_REQUIRE(a->H > 0 && a->W > 0, "mipsf_raster_depth: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_RASTER_MAX_SIDE && a->W <= MIPSF_RASTER_MAX_SIDE, "mipsf_raster_depth: image %u x %u, at most %u a side", a->H,
                  a->W, MIPSF_RASTER_MAX_SIDE);
    MIPSF_REQUIRE(a->F <= MIPSF_RASTER_MAX_FACES, "mipsf_raster_depth: %u faces, at most %u", a->F, MIPSF_RASTER_MAX_FACES);
    MIPSF_REQUIRE((uint64_t)a->n * a->H * a->W <= MIPSF_RASTER_MAX_PIXELS, "mipsf_raster_depth: %u views of %u x %u pixels, at most %u pixels a call",
                  a->n, a->H, a->W, MIPSF_RASTER_MAX_PIXELS);
    MIPSF_REQUIRE((uint64_t)a->n * a->F <= MIPSF_RASTER_MAX_ITEMS, "mipsf_raster_depth: %u views of %u faces, at most %u pairs a call", a->n, a->F,
                  MIPSF_RASTER_MAX_ITEMS);
    MIPSF_REQUIRE(intrinsics_ok(a->fx, a->fy, a->cx, a->cy), "mipsf_raster_depth: intrinsics %g %g %g %g", a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->near == a->near && a->far == a->far, "mipsf_raster_depth: near or far is not a number");
    MIPSF_REQUIRE((a->stages & ~15u) == 0, "mipsf_raster_depth: stages %u", a->stages);
    MIPSF_REQUIRE(a->faces && a->poses && a->depth && a->face && a->workspace && (a->vertices || a->V == 0), "mipsf_raster_depth: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_raster_depth: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const DepthLayout L = depth_layout(a->n, a->F, a->H, a->W);
    uint64_t* keys = (uint64_t*)((char*)a->workspace + L.keys);
    uint64_t* cum = (uint64_t*)((char*)a->workspace + L.cum);
    uint64_t* tiles = (uint64_t*)((char*)a->workspace + L.tiles);
    const Scene s = {a->vertices, a->faces, a->poses, a->V, a->F, a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, a->near, a->far};
    const uint32_t stages = a->stages ? a->stages : 15u;
    const int cus = device_cus();
    const uint32_t wide = (uint32_t)(cus > 0 ? cus : 64) * 8u;      // blocks of a kernel that strides over its work
    const uint32_t pixel_blocks = min(blocks_for(L.pixels, TPB), wide * 4u);
    if (stages & MIPSF_RASTER_STAGE_COUNT) {
        hipLaunchKernelGGL(raster_clear_kernel, dim3(pixel_blocks), dim3(TPB), 0, st, keys, L.pixels);
        hipLaunchKernelGGL(raster_count_kernel, dim3(L.nb), dim3(TPB), 0, st, s, L.items, cum, tiles);
    }
    if (stages & MIPSF_RASTER_STAGE_SCAN) {
        hipLaunchKernelGGL(raster_scan_top_kernel, dim3(1), dim3(TPB), 0, st, tiles, L.nb);
        hipLaunchKernelGGL(raster_scan_apply_kernel, dim3(L.nb), dim3(TPB), 0, st, cum, L.items, (const uint64_t*)tiles);
    }
    if (stages & MIPSF_RASTER_STAGE_RASTER)
        hipLaunchKernelGGL(raster_tiles_kernel, dim3(wide), dim3(TPB), 0, st, s, L.items, (const uint64_t*)cum, keys);
    if (stages & MIPSF_RASTER_STAGE_RESOLVE)
        hipLaunchKernelGGL(raster_resolve_kernel, dim3(pixel_blocks), dim3(TPB), 0, st, (const uint64_t*)keys, L.pixels, a->depth, a->face);
    return check_launch("raster_depth");
}

extern "C" int mipsf_raster_l1(const mipsf_raster_l1_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_raster_l1_args, "mipsf_raster_l1");
    MIPSF_REQUIRE(a->n > 0, "mipsf_raster_l1: no views");
    MIPSF_REQUIRE(a->H > 0 && a->W > 0, "mipsf_raster_l1: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(l1_in_range(a->n, a->H, a->W), "mipsf_raster_l1: %u views of %u x %u: at most 65535 views, %u a side, %u pixels a call", a->n,
                  a->H, a->W, MIPSF_RASTER_MAX_SIDE, MIPSF_RASTER_MAX_PIXELS);
    MIPSF_REQUIRE(a->a && a->b && a->records && a->workspace, "mipsf_raster_l1: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_raster_l1: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = l1_blocks(a->H, a->W);
    L1Partial* part = (L1Partial*)a->workspace;
    hipLaunchKernelGGL(raster_l1_partial_kernel, dim3(nb, a->n), dim3(TPB), 0, st, a->a, a->b, a->H * a->W, part);
    hipLaunchKernelGGL(raster_l1_finish_kernel, dim3(a->n), dim3(MIPSF_WAVE), 0, st, (const L1Partial*)part, nb, a->records);
    return check_launch("raster_l1");
}

extern "C" int mipsf_raster_visible(const mipsf_raster_visible_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_raster_visible_args, "mipsf_raster_visible");
    if (a->m == 0) return 0;
    MIPSF_REQUIRE(a->points && a->seen, "mipsf_raster_visible: null pointer");
    MIPSF_REQUIRE(a->n == 0 || (a->depth && a->poses && a->max_depth), "mipsf_raster_visible: null pointer");
    MIPSF_REQUIRE(a->n == 0 || (a->H > 0 && a->W > 0 && a->H <= MIPSF_RASTER_MAX_SIDE && a->W <= MIPSF_RASTER_MAX_SIDE),
                  "mipsf_raster_visible: image %u x %u, 1 .. %u a side", a->H, a->W, MIPSF_RASTER_MAX_SIDE);
    MIPSF_REQUIRE(intrinsics_ok(a->fx, a->fy, a->cx, a->cy), "mipsf_raster_visible: intrinsics %g %g %g %g", a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->edge == a->edge && a->eps == a->eps, "mipsf_raster_visible: edge or eps is not a number");
    const Views s = {a->depth, a->poses, a->max_depth, a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, a->edge, a->eps};
    hipLaunchKernelGGL(raster_visible_kernel, dim3(blocks_for(a->m, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->points, a->m, s, a->seen);
    return check_launch("raster_visible");
}
