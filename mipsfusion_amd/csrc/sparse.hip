// The TSDF volume kept only where a depth pixel put a surface (include/mipsf_sparse.h): an index grid with one word per brick of
// tsdf.hip's 8 x 8 x 16 voxels over a virtual grid, and a pool of brick-sized slots.  Upstream has no TSDF code; the rules are this
// project's own, and every one of them is the dense rule (mipsf_tsdf.h, mipsf_track.h) read over the dense state with the voxels of
// unallocated bricks left at zero.  DESIGN.md 4.24.
//
// Shape of the kernels.  Allocation: a lane per pixel of a view walks the band around its depth and marks the bricks of the eight
// corners with an integer atomic minimum of the view index (a lane remembers the brick each corner marked last, and reads before it
// writes: most of a band falls into one brick); three launches of block_dev.h's device-wide prefix sum then number the marked bricks
// that have no slot, in brick order, behind the slots in use.  Integration: tsdf.hip's kernel with a workgroup per slot, a lane's
// four voxels contiguous in the slot (the 256 lanes read and write 4 KB in one piece).  Gather: a lane per voxel of the window.  Ray
// cast: tsdf_track.hip's kernel with the corner reads through the table; a base voxel with its eight corners in one brick (7/8 of
// 7/8 of 15/16 of them) costs one word of the table.  The dense kernels are restated here, not shared: their code objects stay as
// they are.
#include "block_dev.h"
#include "sparse_dev.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t BX = BRICK_X, BY = BRICK_Y, BZ = BRICK_Z;
constexpr uint32_t SLOT = BRICK_VOXELS;
constexpr uint32_t RUN = 4;                       // voxels of a lane, along z
constexpr uint32_t CHUNK = MIPSF_TSDF_VIEW_CHUNK;
constexpr uint32_t TILE = MIPSF_TRACK_TILE;
constexpr uint32_t UNMARKED = 0xffffffffu;
static_assert(BX * BY * (BZ / RUN) == TPB, "one lane per run of the brick");
static_assert(CHUNK == TPB, "one lane per view of a chunk");
static_assert(TPB * SCAN_ITEMS == MIPSF_SPARSE_SCAN_TILE, "a tile of the prefix sum");
static_assert(TILE * TILE == TPB && TILE == 16, "a lane per pixel of the tile, a wave per 8 x 8 quarter");
static_assert((uint64_t)MIPSF_SPARSE_MAX_CAPACITY * SLOT <= 0x80000000ull, "a word offset into the pool");
static_assert(sizeof(mipsf_sparse_alloc_record) == 32 && sizeof(mipsf_tsdf_record) == 16 && sizeof(mipsf_track_record) == 16, "records");

// p[0..n) = value.  The clears of a call are launches of this kernel, not memset nodes: a captured graph replays them as it
// replays the kernels around them.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_fill_kernel(uint32_t* __restrict__ p, uint64_t n, uint32_t value) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) p[i] = value;
}

void fill(void* p, uint64_t words, uint32_t value, hipStream_t st) {
    hipLaunchKernelGGL(sparse_fill_kernel, dim3(blocks_for(words, TPB)), dim3(TPB), 0, st, (uint32_t*)p, words, value);
}

// ------------------------------------------------------------------------------------------------ allocation
struct Views {
    const float* depth;
    const float* poses;
    uint32_t n, H, W, steps;
    double fx, fy, cx, cy, depth_max;
};

// grid: (blocks of 256 pixels, n)
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_mark_kernel(Pool v, Views s, uint32_t* __restrict__ mark) {
    const uint32_t pixel = blockIdx.x * TPB + threadIdx.x, k = blockIdx.y;
    if (pixel >= s.H * s.W) return;
    const uint32_t row = pixel / s.W, col = pixel % s.W;
    const double d = (double)s.depth[((size_t)k * s.H + row) * s.W + col];
    if (!(d > 0.0 && d < INFINITY && d <= s.depth_max)) return;
    const float* P = s.poses + (size_t)k * 16;
    const double ux = ((double)col - s.cx) / s.fx, uy = ((double)row - s.cy) / s.fy;
    const double top[3] = {(double)v.X - 1.0, (double)v.Y - 1.0, (double)v.Z - 1.0};
    uint32_t last[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) last[c] = UNMARKED;
    const int32_t steps = (int32_t)s.steps;
    for (int32_t j = -steps; j <= steps; ++j) {
        const double z = d + (double)j * v.voxel;
        if (!(z > 0.0)) continue;
        const double pc[3] = {z * ux, -(z * uy), -z};
        double c0[3], c1[3];
        bool ok0[3], ok1[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double p = (((double)P[4 * a] * pc[0] + (double)P[4 * a + 1] * pc[1]) + (double)P[4 * a + 2] * pc[2]) + (double)P[4 * a + 3];
            const double i0 = floor((p - v.origin[a]) / v.voxel);
            c0[a] = i0 - 1.0, c1[a] = i0 + 2.0;
            ok0[a] = c0[a] >= 0.0 && c0[a] <= top[a];                            // a NaN fails
            ok1[a] = c1[a] >= 0.0 && c1[a] <= top[a];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool ok = (c & 4 ? ok1[0] : ok0[0]) && (c & 2 ? ok1[1] : ok0[1]) && (c & 1 ? ok1[2] : ok0[2]);
            if (!ok) continue;
            const uint32_t b = brick_of(v, (uint32_t)(c & 4 ? c1[0] : c0[0]), (uint32_t)(c & 2 ? c1[1] : c0[1]), (uint32_t)(c & 1 ? c1[2] : c0[2]));
            if (b == last[c]) continue;
            last[c] = b;
            if (mark[b] > k) atomicMin(&mark[b], k);                            // marks only fall: a stale read costs an atomic, never a mark
        }
    }
}

// whether brick b is marked and has no slot
__device__ __forceinline__ uint32_t wants_slot(const Pool& v, const uint32_t* mark, uint64_t b) {
    return b < v.bricks && mark[b] != UNMARKED && v.table[b] < 0 ? 1u : 0u;
}

// grid: tiles of 1024 bricks; sums[tile] = bricks of the tile that want a slot
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_tile_kernel(Pool v, const uint32_t* __restrict__ mark, uint32_t* __restrict__ sums,
                                                                            mipsf_sparse_alloc_record* __restrict__ record) {
    __shared__ uint32_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    uint32_t want = 0, marked = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        want += wants_slot(v, mark, base + e);
        marked += base + e < v.bricks && mark[base + e] != UNMARKED ? 1u : 0u;
    }
    want = block_reduce<WAVES>(want, sm, Add());
    marked = block_reduce<WAVES>(marked, sm, Add());
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = want;
        if (marked) atomicAdd((unsigned long long*)&record->marked, (unsigned long long)marked);
    }
}

// ONE block: the tile sums become their exclusive scan; the count moves on, sums[nb] keeps the count before
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_top_kernel(Pool v, uint32_t* __restrict__ sums, uint32_t nb,
                                                                           mipsf_sparse_alloc_record* __restrict__ record) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t total = scan_top<WAVES>(sums, nb, sm);
    if (threadIdx.x == 0) {
        const uint32_t before = min(*v.count, v.capacity);
        const uint32_t created = min(total, v.capacity - before);
        sums[nb] = before;
        *v.count = before + created;
        record->created = created;
        record->dropped = total - created;
        record->in_use = before + created;
    }
}

// grid: the tiles again; a brick that wants a slot and is the r-th of them gets slot before + r while the pool lasts
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_assign_kernel(Pool v, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ sums,
                                                                              uint32_t nb) {
    __shared__ uint32_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    uint32_t want[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        want[e] = wants_slot(v, mark, base + e);
        mine += want[e];
    }
    uint64_t slot = (uint64_t)block_excl_scan<WAVES>(mine, sm) + sums[blockIdx.x] + sums[nb];
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        if (!want[e]) continue;
        if (slot < v.capacity) {                                                // nothing is written beyond the pool
            v.table[base + e] = (int32_t)slot;
            v.slot_brick[slot] = (int32_t)(base + e);
            v.birth[slot] = mark[base + e];
        }
        ++slot;
    }
}

// ------------------------------------------------------------------------------------------------ integration
struct Frames {
    const float* depth;
    const float* rgb;
    const float* poses;
    uint32_t n, H, W, flags;
    double fx, fy, cx, cy, trunc, depth_max, max_weight;
};

// tsdf.hip's view_can_update, restated: whether view k can update a voxel of the ball (centre c, radius r) that holds the brick.
// The bounds are derived there; the test may be generous and never leaves out a pair the rule updates.
__device__ __forceinline__ bool view_can_update(const Frames& s, uint32_t k, const double c[3], double r) {
    const float* P = s.poses + (size_t)k * 16;
    double R[9], t[3], scale = 1.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        R[i * 3] = (double)P[i * 4], R[i * 3 + 1] = (double)P[i * 4 + 1], R[i * 3 + 2] = (double)P[i * 4 + 2];
        t[i] = (double)P[i * 4 + 3];
        finite = finite && fabs(R[i * 3]) < INFINITY && fabs(R[i * 3 + 1]) < INFINITY && fabs(R[i * 3 + 2]) < INFINITY && fabs(t[i]) < INFINITY;
        scale += fabs(t[i]) + fabs(c[i]);
    }
    if (!finite) return false;
    const double q[3] = {c[0] - t[0], c[1] - t[1], c[2] - t[2]};
    const double rr = r * 1.000001 + 1.0e-9 * scale;
    double cc[3], rc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cc[a] = (R[a] * q[0] + R[3 + a] * q[1]) + R[6 + a] * q[2];
        rc[a] = rr * sqrt((R[a] * R[a] + R[3 + a] * R[3 + a]) + R[6 + a] * R[6 + a]) * 1.000001;
    }
    const double zc = -cc[2];
    bool keep = zc + rc[2] > 0.0 && zc - rc[2] <= s.depth_max + s.trunc;
    const double a0 = (-1.5 - s.cx) / s.fx, a1 = ((double)s.W + 0.5 - s.cx) / s.fx;
    keep = keep && (cc[0] - a0 * zc) + (rc[0] + fabs(a0) * rc[2]) >= 0.0 && (cc[0] - a1 * zc) - (rc[0] + fabs(a1) * rc[2]) <= 0.0;
    const double b0 = (s.cy - (double)s.H - 0.5) / s.fy, b1 = (s.cy + 1.5) / s.fy;
    keep = keep && (cc[1] - b0 * zc) + (rc[1] + fabs(b0) * rc[2]) >= 0.0 && (cc[1] - b1 * zc) - (rc[1] + fabs(b1) * rc[2]) <= 0.0;
    return keep;
}

// grid: one block per slot of the pool; those not in use return
template <bool COLOR>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_integrate_kernel(Pool vol, Frames s, mipsf_tsdf_record* __restrict__ record) {
    __shared__ uint32_t list[CHUNK];
    __shared__ uint32_t wave_count[WAVES];
    __shared__ uint64_t sm[WAVES];
    const uint32_t slot = blockIdx.x;
    if (slot >= min(*vol.count, vol.capacity)) return;                          // the whole block
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t brick = (uint32_t)vol.slot_brick[slot], born = vol.birth[slot];
    const uint32_t bz = brick % vol.bricks_z, by = (brick / vol.bricks_z) % vol.bricks_y, bx = brick / (vol.bricks_z * vol.bricks_y);
    const uint32_t x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;                    // the brick; it holds at least one voxel
    const uint32_t x1 = min(x0 + BX, vol.X), y1 = min(y0 + BY, vol.Y), z1 = min(z0 + BZ, vol.Z);

    // the lane's run: voxels (i, j, k0 .. k0 + 3), words base .. base + 3 of the pool
    const uint32_t i = x0 + (tid >> 5), j = y0 + ((tid >> 2) & 7u), k0 = z0 + (tid & 3u) * RUN;
    const bool row_ok = i < vol.X && j < vol.Y;
    const size_t base = (size_t)slot * SLOT + (size_t)tid * RUN;
    const double px = (double)(float)vol.ticks[0][row_ok ? i : x0], py = (double)(float)vol.ticks[1][row_ok ? j : y0];
    bool ok[RUN];
    double pz[RUN];
    float tsdf[RUN], weight[RUN], color[COLOR ? RUN * 3 : 1];
#pragma unroll
    for (uint32_t r = 0; r < RUN; ++r) {
        ok[r] = row_ok && k0 + r < vol.Z;
        pz[r] = (double)(float)vol.ticks[2][ok[r] ? k0 + r : z0];
        tsdf[r] = ok[r] ? vol.tsdf[base + r] : 0.0f;
        weight[r] = ok[r] ? vol.weight[base + r] : 0.0f;
        if (COLOR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) color[r * 3 + c] = ok[r] ? vol.color[(base + r) * 3 + c] : 0.0f;
        }
    }

    // the ball that holds the brick's voxels (every lane the same)
    double c[3], radius;
    {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t a = x0; a < x1; ++a) lo[0] = fmin(lo[0], (double)(float)vol.ticks[0][a]), hi[0] = fmax(hi[0], (double)(float)vol.ticks[0][a]);
        for (uint32_t a = y0; a < y1; ++a) lo[1] = fmin(lo[1], (double)(float)vol.ticks[1][a]), hi[1] = fmax(hi[1], (double)(float)vol.ticks[1][a]);
        for (uint32_t a = z0; a < z1; ++a) lo[2] = fmin(lo[2], (double)(float)vol.ticks[2][a]), hi[2] = fmax(hi[2], (double)(float)vol.ticks[2][a]);
        double h[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = 0.5 * lo[a] + 0.5 * hi[a], h[a] = fmax(hi[a] - c[a], c[a] - lo[a]);
        radius = sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
    }
    const bool cull = !(s.flags & MIPSF_TSDF_NO_CULL) && fabs(c[0]) < INFINITY && fabs(c[1]) < INFINITY && fabs(c[2]) < INFINITY && radius < INFINITY;

    const double w_lim = (double)s.W, h_lim = (double)s.H;
    const size_t hw = (size_t)s.H * s.W;
    uint64_t updates = 0;
    for (uint32_t first = 0; first < s.n; first += CHUNK) {
        // ---- which views of the chunk the brick takes: from its birth on, those that can reach it, in ascending order
        const uint32_t k = first + tid;
        const bool keep = k < s.n && k >= born && (!cull || view_can_update(s, k, c, radius));
        const uint64_t mask = __ballot(keep);
        __syncthreads();                                                        // the list of the chunk before is read no more
        if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
            if (w < wave) before += wave_count[w];
            total += wave_count[w];
        }
        if (keep) list[before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = k;
        __syncthreads();

        // ---- the lane's voxels through the surviving views
        for (uint32_t e = 0; e < total; ++e) {
            const uint32_t view = __builtin_amdgcn_readfirstlane(list[e]);
            const float* P = s.poses + (size_t)view * 16;
            const float* D = s.depth + (size_t)view * hw;
            const double qx = px - (double)P[3], qy = py - (double)P[7], tz = (double)P[11];
            const double r20 = (double)P[8], r21 = (double)P[9], r22 = (double)P[10];
            const double pre0 = (double)P[0] * qx + (double)P[4] * qy;
            const double pre1 = (double)P[1] * qx + (double)P[5] * qy;
            const double pre2 = (double)P[2] * qx + (double)P[6] * qy;
#pragma unroll
            for (uint32_t r = 0; r < RUN; ++r) {
                const double qz = pz[r] - tz;
                const double cam0 = pre0 + r20 * qz, cam1 = pre1 + r21 * qz, cam2 = pre2 + r22 * qz;
                const double z = -cam2;
                const double u = s.cx + s.fx * (cam0 / z);
                const double vv = s.cy - s.fy * (cam1 / z);
                const double col = floor(u + 0.5), row = floor(vv + 0.5);
                if (!(ok[r] && z > 0.0 && col >= 0.0 && col < w_lim && row >= 0.0 && row < h_lim)) continue;
                const size_t pixel = (size_t)(uint32_t)row * s.W + (uint32_t)col;
                const double d = (double)D[pixel];
                const double sdf = d - z;
                if (!(d > 0.0 && d < INFINITY && d <= s.depth_max && sdf >= -s.trunc)) continue;
                double val = sdf / s.trunc;
                if (val > 1.0) val = 1.0;
                const double w0 = (double)weight[r], w1 = w0 + 1.0;
                tsdf[r] = (float)((((double)tsdf[r]) * w0 + val) / w1);
                if (COLOR) {
                    const float* C = s.rgb + ((size_t)view * hw + pixel) * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) color[r * 3 + ch] = (float)((((double)color[r * 3 + ch]) * w0 + (double)C[ch]) / w1);
                }
                weight[r] = (float)(w1 < s.max_weight ? w1 : s.max_weight);
                ++updates;
            }
        }
    }

    uint64_t observed = 0;
#pragma unroll
    for (uint32_t r = 0; r < RUN; ++r)
        if (ok[r]) {
            vol.tsdf[base + r] = tsdf[r];
            vol.weight[base + r] = weight[r];
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vol.color[(base + r) * 3 + ch] = color[r * 3 + ch];
            }
            observed += weight[r] > 0.0f ? 1u : 0u;
        }
    updates = block_reduce<WAVES>(updates, sm, Add());
    observed = block_reduce<WAVES>(observed, sm, Add());
    if (tid == 0) {
        if (updates) atomicAdd((unsigned long long*)&record->updates, (unsigned long long)updates);
        if (observed) atomicAdd((unsigned long long*)&record->observed, (unsigned long long)observed);
    }
}

// ------------------------------------------------------------------------------------------------ a window as dense arrays
struct Window {
    uint32_t lo[3], n[3];
    float* tsdf;
    float* weight;
    float* color;
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_gather_kernel(Pool v, Window w) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= (uint64_t)w.n[0] * w.n[1] * w.n[2]) return;
    const uint32_t k = (uint32_t)(e % w.n[2]), j = (uint32_t)((e / w.n[2]) % w.n[1]), i = (uint32_t)(e / ((uint64_t)w.n[2] * w.n[1]));
    const int32_t at = word_of(v, w.lo[0] + i, w.lo[1] + j, w.lo[2] + k);
    w.tsdf[e] = at < 0 ? 0.0f : v.tsdf[at];
    w.weight[e] = at < 0 ? 0.0f : v.weight[at];
    if (w.color) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) w.color[e * 3 + ch] = at < 0 ? 0.0f : v.color[(size_t)at * 3 + ch];
    }
}

// ------------------------------------------------------------------------------------------------ ray cast: the field
struct Base {
    uint32_t i0[3];
    double fr[3];
    bool valid;                         // 0 <= i0[a] <= D_a - 2 on every axis
};

__device__ __forceinline__ Base base_of(const Pool& v, double px, double py, double pz) {
    Base b;
    const double p[3] = {px, py, pz};
    const double top[3] = {(double)v.X - 2.0, (double)v.Y - 2.0, (double)v.Z - 2.0};
    b.valid = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double g = (p[a] - v.origin[a]) / v.voxel;
        const double f = floor(g);
        const bool ok = f >= 0.0 && f <= top[a];         // a NaN fails
        b.valid = b.valid && ok;
        b.i0[a] = ok ? (uint32_t)f : 0u;
        b.fr[a] = g - f;
    }
    return b;
}

// the pool words of the eight corners i0 .. i0 + 1 (i0 + 1 <= D - 1), -1 where the brick has no slot; false: `skip` is on and the
// base voxel's brick has none
__device__ __forceinline__ bool corner_words(const Pool& v, const uint32_t i0[3], bool skip, int32_t at[8]) {
    const uint32_t lx = i0[0] % BX, ly = i0[1] % BY, lz = i0[2] % BZ;
    const int32_t first = word_of(v, i0[0], i0[1], i0[2]);
    if (skip && first < 0) return false;
    if (lx + 1 < BX && ly + 1 < BY && lz + 1 < BZ) {                            // the eight in one brick
#pragma unroll
        for (int c = 0; c < 8; ++c) at[c] = first < 0 ? -1 : first + (int32_t)((c & 4 ? BY * BZ : 0u) + (c & 2 ? BZ : 0u) + (c & 1 ? 1u : 0u));
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) at[c] = c == 0 ? first : word_of(v, i0[0] + (c & 4 ? 1u : 0u), i0[1] + (c & 2 ? 1u : 0u), i0[2] + (c & 1 ? 1u : 0u));
    }
    return true;
}

struct Cast {
    const float* poses;
    uint32_t H, W;
    bool skip;                          // a base voxel without a slot makes the sample unknown: min_weight > 0, no MIPSF_SPARSE_NO_SKIP
    double fx, fy, cx, cy, near, far, step, min_weight;
};

// the trilinear field at a valid base; false: unknown
__device__ __forceinline__ bool field_at(const Pool& v, const Cast& s, const Base& b, double& f) {
    int32_t at[8];
    if (!corner_words(v, b.i0, s.skip, at)) return false;
    bool known = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) known = known && (double)(at[c] < 0 ? 0.0f : v.weight[at[c]]) >= s.min_weight;
    if (!known) return false;
    double w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = (double)(at[c] < 0 ? 0.0f : v.tsdf[at[c]]);
    const double fz = b.fr[2], fy = b.fr[1], fx = b.fr[0];
    const double c00 = w[0] * (1.0 - fz) + w[1] * fz, c01 = w[2] * (1.0 - fz) + w[3] * fz;
    const double c10 = w[4] * (1.0 - fz) + w[5] * fz, c11 = w[6] * (1.0 - fz) + w[7] * fz;
    const double c0 = c00 * (1.0 - fy) + c01 * fy, c1 = c10 * (1.0 - fy) + c11 * fy;
    f = c0 * (1.0 - fx) + c1 * fx;
    return true;
}

__device__ __forceinline__ bool field_of(const Pool& v, const Cast& s, double px, double py, double pz, double& f) {
    const Base b = base_of(v, px, py, pz);
    return b.valid && field_at(v, s, b, f);
}

// grid: (tiles of a view, n)
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_raycast_kernel(Pool v, Cast s, float* __restrict__ depth, float* __restrict__ normals,
                                                                               float* __restrict__ color_out, mipsf_track_record* __restrict__ record) {
    __shared__ uint64_t sm[WAVES];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tiles_x = (s.W + TILE - 1) / TILE;
    const uint32_t row = (blockIdx.x / tiles_x) * TILE + (wave >> 1) * 8u + (lane >> 3);
    const uint32_t col = (blockIdx.x % tiles_x) * TILE + (wave & 1u) * 8u + (lane & 7u);
    const bool in_image = row < s.H && col < s.W;
    const float* P = s.poses + (size_t)blockIdx.y * 16;
    uint64_t hits = 0;
    if (in_image) {
        const double t[3] = {(double)P[3], (double)P[7], (double)P[11]};
        const double dcx = ((double)col - s.cx) / s.fx, dcy = -(((double)row - s.cy) / s.fy), dcz = -1.0;
        double d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = ((double)P[4 * r] * dcx + (double)P[4 * r + 1] * dcy) + (double)P[4 * r + 2] * dcz;
        const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        bool miss = !(len > 0.0 && len < INFINITY);
        const double dt = s.step / len;
        const double dims[3] = {(double)v.X - 1.0, (double)v.Y - 1.0, (double)v.Z - 1.0};
        double t_in = s.near, t_out = s.far;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = v.origin[a], hi = v.origin[a] + v.voxel * dims[a];
            if (d[a] != 0.0) {
                const double ta = (lo - t[a]) / d[a], tb = (hi - t[a]) / d[a];
                const double mn = tb < ta ? tb : ta, mx = tb > ta ? tb : ta;
                t_in = mn > t_in ? mn : t_in;
                t_out = mx < t_out ? mx : t_out;
            } else if (t[a] < lo || t[a] > hi) {
                miss = true;
            }
        }
        miss = miss || !(t_out >= t_in);

        float out_d = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f}, out_c[3] = {0.0f, 0.0f, 0.0f};
        if (!miss) {
            bool prev_known = false, hit = false;
            double prev = 0.0, tstar = 0.0;
            for (uint32_t i = 0; i < MIPSF_TRACK_MAX_SAMPLES; ++i) {
                const double ti = t_in + (double)i * dt;
                if (!(ti <= t_out)) break;
                double f = 0.0;
                const bool known = field_of(v, s, t[0] + d[0] * ti, t[1] + d[1] * ti, t[2] + d[2] * ti, f);
                if (prev_known && known) {
                    if (prev > 0.0 && f <= 0.0) {
                        tstar = (t_in + (double)(i - 1u) * dt) + dt * (prev / (prev - f));      // t_{i-1}, not a running sum
                        hit = true;
                        break;
                    }
                    if (prev < 0.0 && f > 0.0) break;
                }
                prev_known = known, prev = f;
            }
            const float d32 = (float)tstar;
            if (hit && d32 > 0.0f && d32 < INFINITY) {
                out_d = d32;
                hits = 1;
                const double ps[3] = {t[0] + d[0] * tstar, t[1] + d[1] * tstar, t[2] + d[2] * tstar};
                if (normals) {
                    double grad[3];
                    bool all = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        double fp = 0.0, fm = 0.0;
                        const bool kp = field_of(v, s, a == 0 ? ps[0] + v.voxel : ps[0], a == 1 ? ps[1] + v.voxel : ps[1], a == 2 ? ps[2] + v.voxel : ps[2], fp);
                        const bool km = field_of(v, s, a == 0 ? ps[0] - v.voxel : ps[0], a == 1 ? ps[1] - v.voxel : ps[1], a == 2 ? ps[2] - v.voxel : ps[2], fm);
                        all = all && kp && km;
                        grad[a] = fp - fm;
                    }
                    const double L = sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
                    if (all && L > 0.0 && L < INFINITY) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) out_n[a] = (float)(grad[a] / L);
                    }
                }
                if (color_out) sample_color(v, (ps[0] - v.origin[0]) / v.voxel, (ps[1] - v.origin[1]) / v.voxel, (ps[2] - v.origin[2]) / v.voxel, out_c);
            }
        }
        const size_t pixel = ((size_t)blockIdx.y * s.H + row) * s.W + col;
        depth[pixel] = out_d;
        if (normals) {
#pragma unroll
            for (int a = 0; a < 3; ++a) normals[pixel * 3 + a] = out_n[a];
        }
        if (color_out) {
#pragma unroll
            for (int a = 0; a < 3; ++a) color_out[pixel * 3 + a] = out_c[a];
        }
    }
    hits = block_reduce<WAVES>(hits, sm, Add());
    if (tid == 0 && hits) atomicAdd((unsigned long long*)&record->hits, (unsigned long long)hits);
}

}  // namespace
}  // namespace mipsf

// ------------------------------------------------------------------------------------------------ host
using namespace mipsf;

// the allocation around its marks (sparse_dev.h): what mipsf_sparse_allocate launches before and after its mark kernel, for
// sparse_release.hip, whose restore makes the marks from an archive's bricks
void mipsf::sparse_fill(void* p, uint64_t words, uint32_t value, hipStream_t st) { fill(p, words, value, st); }

void mipsf::sparse_marks_clear(const Pool& v, uint32_t* mark, mipsf_sparse_alloc_record* record, hipStream_t st) {
    fill(record, sizeof(mipsf_sparse_alloc_record) / sizeof(uint32_t), 0u, st);
    fill(mark, v.bricks, UNMARKED, st);
    fill(v.birth, v.capacity, 0u, st);
}

void mipsf::sparse_marks_assign(const Pool& v, const uint32_t* mark, uint32_t* scan, mipsf_sparse_alloc_record* record, hipStream_t st) {
    const uint32_t nb = blocks_for(v.bricks, MIPSF_SPARSE_SCAN_TILE);
    hipLaunchKernelGGL(sparse_tile_kernel, dim3(nb), dim3(TPB), 0, st, v, mark, scan, record);
    hipLaunchKernelGGL(sparse_top_kernel, dim3(1), dim3(TPB), 0, st, v, scan, nb, record);
    hipLaunchKernelGGL(sparse_assign_kernel, dim3(nb), dim3(TPB), 0, st, v, mark, (const uint32_t*)scan, nb);
}

extern "C" uint64_t mipsf_sparse_scan_words(uint32_t X, uint32_t Y, uint32_t Z) {
    if (X == 0 || Y == 0 || Z == 0) return 0;
    const uint64_t xy = (uint64_t)blocks_for(X, BX) * blocks_for(Y, BY);
    if (xy > MIPSF_SPARSE_MAX_BRICKS || xy * blocks_for(Z, BZ) > MIPSF_SPARSE_MAX_BRICKS) return 0;
    return (uint64_t)blocks_for(brick_count(X, Y, Z), MIPSF_SPARSE_SCAN_TILE) + 1u;
}

extern "C" int mipsf_sparse_allocate(const mipsf_sparse_allocate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_allocate_args, "mipsf_sparse_allocate");
    if (volume_ok(a->vol, "mipsf_sparse_allocate") || images_ok(a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, "mipsf_sparse_allocate")) return 1;
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_sparse_allocate: depth_max is not a number");
    MIPSF_REQUIRE(a->band >= 0.0 && a->band < INFINITY, "mipsf_sparse_allocate: band %g is negative, infinite or not a number", a->band);
    MIPSF_REQUIRE(a->steps <= MIPSF_SPARSE_MAX_STEPS, "mipsf_sparse_allocate: %u steps, at most %u", a->steps, MIPSF_SPARSE_MAX_STEPS);
    MIPSF_REQUIRE(a->mark && a->scan && a->record && (a->n == 0 || (a->depth && a->poses)), "mipsf_sparse_allocate: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Pool v = pool_of(a->vol);
    sparse_marks_clear(v, a->mark, a->record, st);
    if (a->n > 0) {
        const Views s = {a->depth, a->poses, a->n, a->H, a->W, a->steps, a->fx, a->fy, a->cx, a->cy, a->depth_max};
        hipLaunchKernelGGL(sparse_mark_kernel, dim3(blocks_for((uint64_t)a->H * a->W, TPB), a->n), dim3(TPB), 0, st, v, s, a->mark);
    }
    sparse_marks_assign(v, a->mark, a->scan, a->record, st);
    return check_launch("sparse_allocate");
}

extern "C" int mipsf_sparse_integrate(const mipsf_sparse_integrate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_integrate_args, "mipsf_sparse_integrate");
    if (volume_ok(a->vol, "mipsf_sparse_integrate") || images_ok(a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, "mipsf_sparse_integrate")) return 1;
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_sparse_integrate: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_sparse_integrate: depth_max is not a number");
    MIPSF_REQUIRE(a->max_weight >= 1.0, "mipsf_sparse_integrate: max_weight %g, at least 1", a->max_weight);
    MIPSF_REQUIRE((a->flags & ~MIPSF_TSDF_NO_CULL) == 0, "mipsf_sparse_integrate: flags %u", a->flags);
    MIPSF_REQUIRE(a->n == 0 || (a->rgb != nullptr) == (a->vol.color != nullptr), "mipsf_sparse_integrate: rgb and color go together (rgb %s, color %s)",
                  a->rgb ? "given" : "null", a->vol.color ? "given" : "null");
    MIPSF_REQUIRE(a->record && (a->n == 0 || (a->depth && a->poses)), "mipsf_sparse_integrate: null pointer");
    hipStream_t st = (hipStream_t)stream;
    fill(a->record, sizeof(mipsf_tsdf_record) / sizeof(uint32_t), 0u, st);
    if (a->n == 0) return check_launch("sparse_integrate");
    const Pool v = pool_of(a->vol);
    const Frames s = {a->depth, a->rgb, a->poses, a->n, a->H, a->W, a->flags, a->fx, a->fy, a->cx, a->cy, a->trunc, a->depth_max, a->max_weight};
    if (v.color)
        hipLaunchKernelGGL(sparse_integrate_kernel<true>, dim3(v.capacity), dim3(TPB), 0, st, v, s, a->record);
    else
        hipLaunchKernelGGL(sparse_integrate_kernel<false>, dim3(v.capacity), dim3(TPB), 0, st, v, s, a->record);
    return check_launch("sparse_integrate");
}

extern "C" int mipsf_sparse_gather(const mipsf_sparse_gather_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_gather_args, "mipsf_sparse_gather");
    if (volume_ok(a->vol, "mipsf_sparse_gather")) return 1;
    const uint32_t D[3] = {a->vol.X, a->vol.Y, a->vol.Z};
    for (int d = 0; d < 3; ++d)
        MIPSF_REQUIRE(a->lo[d] < a->hi[d] && a->hi[d] <= D[d], "mipsf_sparse_gather: window %u .. %u on axis %d of %u voxels", a->lo[d], a->hi[d], d, D[d]);
    const uint64_t n01 = (uint64_t)(a->hi[0] - a->lo[0]) * (a->hi[1] - a->lo[1]), n2 = a->hi[2] - a->lo[2];
    MIPSF_REQUIRE(n01 <= MIPSF_TSDF_MAX_VOXELS && n01 * n2 <= MIPSF_TSDF_MAX_VOXELS, "mipsf_sparse_gather: a window of %u x %u x %u voxels, at most 2^31 - 1",
                  a->hi[0] - a->lo[0], a->hi[1] - a->lo[1], a->hi[2] - a->lo[2]);
    MIPSF_REQUIRE(!(a->color && !a->vol.color), "mipsf_sparse_gather: color needs a volume with color");
    MIPSF_REQUIRE(a->tsdf && a->weight, "mipsf_sparse_gather: null pointer");
    Window w;
    for (int d = 0; d < 3; ++d) w.lo[d] = a->lo[d], w.n[d] = a->hi[d] - a->lo[d];
    w.tsdf = a->tsdf, w.weight = a->weight, w.color = a->color;
    hipLaunchKernelGGL(sparse_gather_kernel, dim3(blocks_for(n01 * n2, TPB)), dim3(TPB), 0, (hipStream_t)stream, pool_of(a->vol), w);
    return check_launch("sparse_gather");
}

extern "C" int mipsf_sparse_raycast(const mipsf_sparse_raycast_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_raycast_args, "mipsf_sparse_raycast");
    if (volume_ok(a->vol, "mipsf_sparse_raycast") || images_ok(a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, "mipsf_sparse_raycast")) return 1;
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_sparse_raycast: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(pos_finite(a->step), "mipsf_sparse_raycast: step %g is not positive and finite", a->step);
    MIPSF_REQUIRE(a->near == a->near && a->far == a->far, "mipsf_sparse_raycast: near or far is not a number");
    MIPSF_REQUIRE(a->min_weight == a->min_weight, "mipsf_sparse_raycast: min_weight is not a number");
    const double ex = (double)a->vol.X - 1.0, ey = (double)a->vol.Y - 1.0, ez = (double)a->vol.Z - 1.0;
    const double most = a->vol.voxel * sqrt(ex * ex + ey * ey + ez * ez) / a->step + 2.0;
    MIPSF_REQUIRE(most <= (double)MIPSF_TRACK_MAX_SAMPLES, "mipsf_sparse_raycast: step %g gives up to %g samples a ray, at most %u", a->step, most,
                  MIPSF_TRACK_MAX_SAMPLES);
    MIPSF_REQUIRE((a->flags & ~MIPSF_SPARSE_NO_SKIP) == 0, "mipsf_sparse_raycast: flags %u", a->flags);
    MIPSF_REQUIRE(!(a->color_out && !a->vol.color), "mipsf_sparse_raycast: color_out needs a volume with color");
    MIPSF_REQUIRE(a->record && (a->n == 0 || (a->poses && a->depth)), "mipsf_sparse_raycast: null pointer");
    hipStream_t st = (hipStream_t)stream;
    fill(a->record, sizeof(mipsf_track_record) / sizeof(uint32_t), 0u, st);
    if (a->n == 0) return check_launch("sparse_raycast");
    const Cast s = {a->poses, a->H, a->W, !(a->flags & MIPSF_SPARSE_NO_SKIP) && a->min_weight > 0.0, a->fx, a->fy, a->cx, a->cy, a->near, a->far, a->step,
                    a->min_weight};
    hipLaunchKernelGGL(sparse_raycast_kernel, dim3(blocks_for(a->W, TILE) * blocks_for(a->H, TILE), a->n), dim3(TPB), 0, st, pool_of(a->vol), s, a->depth,
                       a->normals, a->color_out, a->record);
    return check_launch("sparse_raycast");
}
