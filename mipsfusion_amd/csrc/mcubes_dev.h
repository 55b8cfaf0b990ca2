// The marching rule and the weld (include/mipsf_mesh.h), stated once for mcubes.hip, which marches a dense volume, and
// sparse_mesh.hip, which marches the bricks of a sparse one: the tables, a dual value, the rejections on `thresh`, a vertex on an
// edge, the scan over block sums, and the weld over integer cells.  What a soup vertex's cell is, and what is written for a surviving
// vertex, is the caller's (`Cells`): the dense weld quantises the soup's floats, the sparse one adds the brick's base.  Everything
// sits in an unnamed namespace: each unit gets its own kernels.  Device code and the host's launch sequence of the weld.
#pragma once
#include "block_dev.h"
#include "../../include/mipsf_mesh.h"
#include "mcubes_tables.h"

#include <math.h>

namespace mipsf {

namespace {

__device__ const int8_t k_edge_ends[12][2] = MCUBES_EDGE_ENDS_INIT;
__device__ const uint8_t k_ntri[256] = MCUBES_NTRI_INIT;
__device__ const int8_t k_tri[256][3 * MCUBES_MAX_TRIS] = MCUBES_TRI_INIT;

constexpr uint32_t ITEMS = 16;                  // consecutive elements per thread of the scan family
constexpr uint32_t CHUNK = MIPSF_MCUBES_BLOCK_CELLS;
constexpr int WAVES = 256 / MIPSF_WAVE;         // of a workgroup of the scan family
static_assert(CHUNK == 256 * ITEMS, "a block of the offset table is one workgroup of the scan family");

// the eight voxels of a dual value in the order they are summed
__device__ __forceinline__ float dual_sum(float v000, float v100, float v010, float v001, float v110, float v011, float v101,
                                          float v111) {
    float d = 0.0f;
    d += 0.125f * v000;
    d += 0.125f * v100;
    d += 0.125f * v010;
    d += 0.125f * v001;
    d += 0.125f * v110;
    d += 0.125f * v011;
    d += 0.125f * v101;
    d += 0.125f * v111;
    return d;
}

// the per-cell rejections on `thresh`.  With every |d| <= thresh / 2 none of them can fire (|a| + |b| <= thresh and
// |a - b| <= |a| + |b|, also after rounding), so the 64 pairs are only visited beyond that.
__device__ __forceinline__ bool thresh_rejects(const float d[8], float thresh) {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) m = fmaxf(m, fabsf(d[c]));
    if (!(m > 0.5f * thresh)) return false;
    for (int k = 0; k < 8; ++k)
        for (int l = 0; l < 8; ++l) {
            if (d[k] * d[l] < 0.0f) {
                if (fabsf(d[k]) + fabsf(d[l]) > thresh) return true;
            } else if (fabsf(d[k] - d[l]) > thresh) {
                return true;
            }
        }
    for (int c = 0; c < 8; ++c)
        if (fabsf(d[c]) > thresh) return true;
    return false;
}

// in place: sums[0..n) -> exclusive prefix, sums[n] = total.  One workgroup of 1024 threads walks the array.
__global__ __launch_bounds__(1024) void scan_blocks_kernel(uint32_t* __restrict__ sums, uint32_t n) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t mine = i < n ? sums[i] : 0u;
        const uint32_t incl = wave_incl_scan(mine);
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t pre = carry_s;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        if (i < n) sums[i] = pre + incl - mine;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = pre + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[n] = carry_s;
}

struct Vec3 {
    float x, y, z;
};

// vertex on the edge between corner positions p1, p2 with values d1, d2 (snap rules first, in this order)
__device__ __forceinline__ Vec3 edge_vertex(float iso, Vec3 p1, Vec3 p2, float d1, float d2) {
    if (fabsf(iso - d1) < 0.00001f) return p1;
    if (fabsf(iso - d2) < 0.00001f) return p2;
    if (fabsf(d1 - d2) < 0.00001f) return p1;
    const float mu = (iso - d1) / (d2 - d1);
    Vec3 r;
    r.x = p1.x + mu * (p2.x - p1.x);
    r.y = p1.y + mu * (p2.y - p1.y);
    r.z = p1.z + mu * (p2.z - p1.z);
    return r;
}

// ------------------------------------------------------------------------------------------------------- weld
// Hash table of quantised cells: key = (x, y | z), value = the smallest soup index seen in the cell, later the smallest of its
// connected component.  A slot is claimed with two compare-and-swaps (xy word, then z word); a thread that loses either moves
// on, so no thread ever waits for another.  0 in a key word = empty (coordinates are >= 0 and stored + 1).
//
// Cells: `void cell(uint32_t v, int& x, int& y, int& z) const`, the integer cell of soup vertex v (a negative coordinate: the
// vertex cannot be placed), and `void keep(uint32_t v, uint32_t id) const`, which writes surviving vertex v as vertex id.
struct WeldTable {
    unsigned long long* xy;
    uint32_t* z;
    uint32_t* val;
    uint32_t mask;
};

__device__ __forceinline__ int weld_quantise(float v) {
    const int s = (0.0f < v) - (v < 0.0f);
    return (int)(v / MIPSF_MCUBES_WELD_GRID + 0.5f * (float)s);
}

__device__ __forceinline__ uint32_t weld_hash(int x, int y, int z) {
    uint32_t h = (uint32_t)x * 0x9E3779B1u ^ (uint32_t)y * 0x85EBCA77u ^ (uint32_t)z * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 13;
    return h;
}

constexpr uint32_t WELD_NONE = 0xFFFFFFFFu;
constexpr uint32_t WELD_OWNER = 0x80000000u;

__device__ __forceinline__ uint32_t weld_find(const WeldTable& tb, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0) return WELD_NONE;
    const unsigned long long kxy = (((unsigned long long)(uint32_t)x << 32) | (uint32_t)y) + 1ull;
    const uint32_t kz = (uint32_t)z + 1u;
    uint32_t s = weld_hash(x, y, z) & tb.mask;
    for (uint32_t probe = 0; probe <= tb.mask; ++probe, s = (s + 1) & tb.mask) {
        const unsigned long long cur = tb.xy[s];
        if (cur == 0ull) return WELD_NONE;
        if (cur == kxy && tb.z[s] == kz) return s;
    }
    return WELD_NONE;
}

__global__ __launch_bounds__(256) void weld_clear_kernel(WeldTable tb, uint32_t* __restrict__ counts) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s <= tb.mask) tb.xy[s] = 0ull, tb.z[s] = 0u, tb.val[s] = WELD_NONE;
    if (s < 4) counts[s] = 0;
}

template <class Cells>
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void weld_insert_kernel(Cells cells, uint32_t n, WeldTable tb, uint32_t* __restrict__ slot_of,
                                                                           uint32_t* __restrict__ counts) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    int x, y, z;
    cells.cell(v, x, y, z);
    uint32_t found = WELD_NONE;
    if (x >= 0 && y >= 0 && z >= 0 && z != 0x7FFFFFFF) {
        const unsigned long long kxy = (((unsigned long long)(uint32_t)x << 32) | (uint32_t)y) + 1ull;
        const uint32_t kz = (uint32_t)z + 1u;
        uint32_t s = weld_hash(x, y, z) & tb.mask;
        for (uint32_t probe = 0; probe <= tb.mask; ++probe, s = (s + 1) & tb.mask) {
            const unsigned long long was = atomicCAS(&tb.xy[s], 0ull, kxy);
            if (was != 0ull && was != kxy) continue;
            const uint32_t wz = atomicCAS(&tb.z[s], 0u, kz);
            if (wz != 0u && wz != kz) continue;
            found = s;
            break;
        }
    }
    if (found == WELD_NONE) {
        atomicAdd(&counts[2], 1u);
        slot_of[v] = WELD_NONE;
        return;
    }
    atomicMin(&tb.val[found], v);
    slot_of[v] = found;
}

// the first vertex of every cell does the cell's neighbour look-ups in the rounds that follow
__global__ __launch_bounds__(256) void weld_owner_kernel(uint32_t n, WeldTable tb, uint32_t* __restrict__ slot_of) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = slot_of[v];
    if (s != WELD_NONE && tb.val[s] == v) slot_of[v] = s | WELD_OWNER;
}

// one round of label propagation: a cell takes the smallest label among the 27 cells around it.  Labels only decrease and
// the fixed point (the smallest soup index of the connected component) does not depend on the order of the updates.
template <class Cells>
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void weld_round_kernel(Cells cells, uint32_t n, WeldTable tb, const uint32_t* __restrict__ slot_of,
                                                                          uint32_t* __restrict__ counts, uint32_t round) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t so = slot_of[v];
    if (so == WELD_NONE || !(so & WELD_OWNER)) return;
    const uint32_t s = so & ~WELD_OWNER;
    int x, y, z;
    cells.cell(v, x, y, z);
    const uint32_t mine = tb.val[s];
    uint32_t best = mine;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int c = -1; c <= 1; ++c) {
                if (a == 0 && b == 0 && c == 0) continue;
                const uint32_t t = weld_find(tb, x + a, y + b, z + c);
                if (t != WELD_NONE) best = min(best, tb.val[t]);
            }
    if (best < mine) {
        atomicMin(&tb.val[s], best);
        atomicMax(&counts[1], round + 1);
    }
}

__global__ __launch_bounds__(256) void weld_root_kernel(uint32_t n, WeldTable tb, const uint32_t* __restrict__ slot_of,
                                                        uint32_t* __restrict__ root) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t so = slot_of[v];
    root[v] = so == WELD_NONE ? v : tb.val[so & ~WELD_OWNER];
}

__global__ __launch_bounds__(256) void weld_reduce_kernel(const uint32_t* __restrict__ root, uint32_t n,
                                                          uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t wsum[WAVES];
    const uint32_t first = blockIdx.x * CHUNK + threadIdx.x * ITEMS;
    uint32_t mine = 0;
    for (uint32_t q = 0; q < ITEMS; ++q)
        if (first + q < n && root[first + q] == first + q) ++mine;
    const uint32_t total = block_reduce<WAVES>(mine, wsum, Add());
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// survivors (root == self) are numbered in soup order and kept
template <class Cells>
__global__ __launch_bounds__(256) void weld_compact_kernel(Cells cells, const uint32_t* __restrict__ root, uint32_t n,
                                                           const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ new_id,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[WAVES];
    const uint32_t first = blockIdx.x * CHUNK + threadIdx.x * ITEMS;
    uint32_t mine = 0;
    for (uint32_t q = 0; q < ITEMS; ++q)
        if (first + q < n && root[first + q] == first + q) ++mine;
    uint32_t off = block_offsets[blockIdx.x] + block_excl_scan<WAVES>(mine, wsum);
    for (uint32_t q = 0; q < ITEMS; ++q) {
        const uint32_t v = first + q;
        if (v < n && root[v] == v) {
            new_id[v] = off;
            cells.keep(v, off);
            ++off;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) counts[0] = block_offsets[gridDim.x];
}

__global__ __launch_bounds__(256) void weld_faces_kernel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ new_id,
                                                         uint32_t n, int32_t* __restrict__ faces) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = root[v];
    faces[v] = r < n ? (int32_t)new_id[r] : -1;
}

inline uint32_t n_blocks(uint64_t n) { return (uint32_t)((n + CHUNK - 1) / CHUNK); }

// the launches of a weld of T triangles over `scratch` (mcubes_weld_words(T) words, 8-byte aligned; slots = mcubes_weld_slots(T))
template <class Cells>
void weld_enqueue(const Cells& cells, uint32_t T, uint64_t slots, uint32_t* scratch, int32_t* faces, uint32_t* counts, uint32_t max_rounds,
                  hipStream_t s) {
    const uint32_t n = 3 * T, nb = n_blocks(n), g = (n + 255) / 256;
    WeldTable tb;
    tb.xy = reinterpret_cast<unsigned long long*>(scratch);
    tb.z = scratch + 2 * slots;
    tb.val = scratch + 3 * slots;
    tb.mask = (uint32_t)slots - 1;
    uint32_t* slot_of = scratch + 4 * slots;
    uint32_t* root = slot_of + n;
    uint32_t* new_id = root + n;
    uint32_t* offsets = new_id + n;
    hipLaunchKernelGGL(weld_clear_kernel, dim3((uint32_t)(slots / 256)), dim3(256), 0, s, tb, counts);
    if (n == 0) return;
    hipLaunchKernelGGL(weld_insert_kernel<Cells>, dim3(g), dim3(256), 0, s, cells, n, tb, slot_of, counts);
    hipLaunchKernelGGL(weld_owner_kernel, dim3(g), dim3(256), 0, s, n, tb, slot_of);
    for (uint32_t r = 0; r < max_rounds; ++r)
        hipLaunchKernelGGL(weld_round_kernel<Cells>, dim3(g), dim3(256), 0, s, cells, n, tb, (const uint32_t*)slot_of, counts, r);
    hipLaunchKernelGGL(weld_root_kernel, dim3(g), dim3(256), 0, s, n, tb, (const uint32_t*)slot_of, root);
    hipLaunchKernelGGL(weld_reduce_kernel, dim3(nb), dim3(256), 0, s, (const uint32_t*)root, n, offsets);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, s, offsets, nb);
    hipLaunchKernelGGL(weld_compact_kernel<Cells>, dim3(nb), dim3(256), 0, s, cells, (const uint32_t*)root, n, (const uint32_t*)offsets, new_id, counts);
    hipLaunchKernelGGL(weld_faces_kernel, dim3(g), dim3(256), 0, s, (const uint32_t*)root, (const uint32_t*)new_id, n, faces);
}

}  // namespace

}  // namespace mipsf
