// Mesh extraction on the device: marching cubes over the dual grid of an SDF volume with the upstream extractor's semantics
// (include/mipsf_mesh.h).  count = classify + reduce + scan, emit, weld.  The order of the soup is defined by
// scans only (no atomics); the weld uses atomicMin / atomicCAS on a hash table, whose fixed point does not depend on scheduling.
#include "block_dev.h"
#include "../../include/mipsf_mesh.h"
#include "mcubes_tables.h"

#include <math.h>

namespace mipsf {

namespace {

__device__ const int8_t k_edge_ends[12][2] = MCUBES_EDGE_ENDS_INIT;
__device__ const uint8_t k_ntri[256] = MCUBES_NTRI_INIT;
__device__ const int8_t k_tri[256][3 * MCUBES_MAX_TRIS] = MCUBES_TRI_INIT;

constexpr int BX = 8, BY = 8, BZ = 32;          // cells of a classify workgroup
constexpr int VX = BX + 2, VY = BY + 2, VZ = BZ + 2;
constexpr int DX = BX + 1, DY = BY + 1, DZ = BZ + 1;
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

// One workgroup classifies BX x BY x BZ cells.  The voxel brick (one halo voxel on every side) is staged in LDS with invalid
// voxels replaced by NaN, so that a dual value is NaN exactly when one of its voxels is invalid (valid voxels are finite and
// below the truncation, their sums stay finite); then the dual values, then one case byte per cell.
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void mcubes_classify_kernel(const float* __restrict__ vol, int X, int Y, int Z,
                                                                               float iso, float trunc,
                                                                               uint8_t* __restrict__ cases) {
    __shared__ float vox[VX * VY * VZ];
    __shared__ float du[DX * DY * DZ];
    const int i0 = blockIdx.z * BX, j0 = blockIdx.y * BY, k0 = blockIdx.x * BZ;
    const int tid = threadIdx.x;
    for (int t = tid; t < VX * VY * VZ; t += 256) {
        const int c = t % VZ, b = (t / VZ) % VY, a = t / (VZ * VY);
        const int gi = i0 - 1 + a, gj = j0 - 1 + b, gk = k0 - 1 + c;
        float v = __builtin_nanf("");
        if (gi >= 0 && gi < X && gj >= 0 && gj < Y && gk >= 0 && gk < Z) {
            const float d = vol[((size_t)gi * Y + gj) * Z + gk];
            if (d != -INFINITY && fabsf(d) < trunc) v = d;
        }
        vox[t] = v;
    }
    __syncthreads();
    for (int t = tid; t < DX * DY * DZ; t += 256) {
        const int c = t % DZ, b = (t / DZ) % DY, a = t / (DZ * DY);
        const float* p = vox + (a * VY + b) * VZ + c;
        du[t] = dual_sum(p[0], p[VY * VZ], p[VZ], p[1], p[VY * VZ + VZ], p[VZ + 1], p[VY * VZ + 1], p[VY * VZ + VZ + 1]);
    }
    __syncthreads();
    for (int t = tid; t < BX * BY * BZ; t += 256) {
        const int c = t % BZ, b = (t / BZ) % BY, a = t / (BZ * BY);
        const int gi = i0 + a, gj = j0 + b, gk = k0 + c;
        if (gi >= X || gj >= Y || gk >= Z) continue;
        float d[8];
        bool valid = true;
        uint32_t code = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            d[q] = du[((a + (q >> 2)) * DY + b + ((q >> 1) & 1)) * DZ + c + (q & 1)];
            valid = valid && (d[q] == d[q]);
            code |= (d[q] < iso ? 1u : 0u) << q;
        }
        if (!valid || k_ntri[code] == 0) code = 0;      // no crossing, or one of the patterns that emit nothing
        if (code != 0 && thresh_rejects(d, MIPSF_MCUBES_THRESH)) code = 0;
        cases[((size_t)gi * Y + gj) * Z + gk] = (uint8_t)code;
    }
}

// ---- the scan family: a workgroup owns CHUNK consecutive elements, a thread ITEMS consecutive ones; the scans are block_dev.h's
// the case bytes of a thread's ITEMS cells (0 beyond the end)
__device__ __forceinline__ void load_cases(const uint8_t* __restrict__ cases, uint32_t n, uint32_t first, uint8_t out[ITEMS]) {
    if (first + ITEMS <= n && (first & 15u) == 0) {
        const uint4 w = *reinterpret_cast<const uint4*>(cases + first);     // the buffer is 16-byte aligned (checked by the caller)
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t q = 0; q < ITEMS; ++q) out[q] = (uint8_t)(ws[q >> 2] >> (8 * (q & 3)));
    } else {
#pragma unroll
        for (uint32_t q = 0; q < ITEMS; ++q) out[q] = first + q < n ? cases[first + q] : (uint8_t)0;
    }
}

__global__ __launch_bounds__(256) void mcubes_reduce_kernel(const uint8_t* __restrict__ cases, uint32_t n,
                                                            uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t wsum[WAVES];
    uint8_t cs[ITEMS];
    load_cases(cases, n, blockIdx.x * CHUNK + threadIdx.x * ITEMS, cs);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < ITEMS; ++q) mine += k_ntri[cs[q]];
    const uint32_t total = block_reduce<WAVES>(mine, wsum, Add());
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
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

MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void mcubes_emit_kernel(const float* __restrict__ vol, int X, int Y, int Z, float iso,
                                                                           const uint8_t* __restrict__ cases,
                                                                           const uint32_t* __restrict__ block_offsets,
                                                                           float* __restrict__ soup, int32_t* __restrict__ cell_ids,
                                                                           uint32_t capacity) {
    __shared__ uint32_t wsum[WAVES];
    const uint32_t n = (uint32_t)X * Y * Z;
    const uint32_t first = blockIdx.x * CHUNK + threadIdx.x * ITEMS;
    uint8_t cs[ITEMS];
    load_cases(cases, n, first, cs);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < ITEMS; ++q) mine += k_ntri[cs[q]];
    uint32_t off = block_offsets[blockIdx.x] + block_excl_scan<WAVES>(mine, wsum);
    if (mine == 0) return;
    for (uint32_t q = 0; q < ITEMS; ++q) {
        const uint32_t code = cs[q];
        const uint32_t nt = k_ntri[code];
        if (nt == 0) continue;
        const uint32_t cell = first + q;
        const int k = cell % Z, j = (cell / Z) % Y, i = cell / ((uint32_t)Z * Y);
        // a non-zero case means every corner is valid, i.e. 1 <= i <= X-2 etc.: the 27 voxels exist (checked all the same)
        if (i < 1 || j < 1 || k < 1 || i > X - 2 || j > Y - 2 || k > Z - 2) continue;
        float v[3][3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                for (int c = 0; c < 3; ++c) v[a][b][c] = vol[((size_t)(i - 1 + a) * Y + (j - 1 + b)) * Z + (k - 1 + c)];
        float d[8];
        for (int c8 = 0; c8 < 8; ++c8) {
            const int a = c8 >> 2, b = (c8 >> 1) & 1, c = c8 & 1;
            d[c8] = dual_sum(v[a][b][c], v[a + 1][b][c], v[a][b + 1][c], v[a][b][c + 1], v[a + 1][b + 1][c], v[a][b + 1][c + 1],
                             v[a + 1][b][c + 1], v[a + 1][b + 1][c + 1]);
        }
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t o = off + t;
            if (o >= capacity) break;
            for (int w = 0; w < 3; ++w) {
                const int e = k_tri[code][3 * t + w];
                const int c1 = k_edge_ends[e][0], c2 = k_edge_ends[e][1];
                Vec3 p1, p2;
                p1.x = (float)i + ((c1 >> 2) & 1 ? 0.5f : -0.5f);
                p1.y = (float)j + ((c1 >> 1) & 1 ? 0.5f : -0.5f);
                p1.z = (float)k + (c1 & 1 ? 0.5f : -0.5f);
                p2.x = (float)i + ((c2 >> 2) & 1 ? 0.5f : -0.5f);
                p2.y = (float)j + ((c2 >> 1) & 1 ? 0.5f : -0.5f);
                p2.z = (float)k + (c2 & 1 ? 0.5f : -0.5f);
                const Vec3 r = edge_vertex(iso, p1, p2, d[c1], d[c2]);
                float* dst = soup + (size_t)o * 9 + 3 * w;
                dst[0] = r.x, dst[1] = r.y, dst[2] = r.z;
            }
            if (cell_ids) cell_ids[o] = (int32_t)cell;
        }
        off += nt;
    }
}

// ------------------------------------------------------------------------------------------------------- weld
// Hash table of quantised cells: key = (x, y | z), value = the smallest soup index seen in the cell, later the smallest of its
// connected component.  A slot is claimed with two compare-and-swaps (xy word, then z word); a thread that loses either moves
// on, so no thread ever waits for another.  0 in a key word = empty (coordinates are >= 0 and stored + 1).
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

MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void weld_insert_kernel(const float* __restrict__ soup, uint32_t n, WeldTable tb,
                                                                           uint32_t* __restrict__ slot_of,
                                                                           uint32_t* __restrict__ counts) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int x = weld_quantise(soup[3 * (size_t)v]), y = weld_quantise(soup[3 * (size_t)v + 1]),
              z = weld_quantise(soup[3 * (size_t)v + 2]);
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
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(256) void weld_round_kernel(const float* __restrict__ soup, uint32_t n, WeldTable tb,
                                                                          const uint32_t* __restrict__ slot_of,
                                                                          uint32_t* __restrict__ counts, uint32_t round) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t so = slot_of[v];
    if (so == WELD_NONE || !(so & WELD_OWNER)) return;
    const uint32_t s = so & ~WELD_OWNER;
    const int x = weld_quantise(soup[3 * (size_t)v]), y = weld_quantise(soup[3 * (size_t)v + 1]),
              z = weld_quantise(soup[3 * (size_t)v + 2]);
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

// survivors (root == self) are numbered in soup order and their coordinates copied
__global__ __launch_bounds__(256) void weld_compact_kernel(const float* __restrict__ soup, const uint32_t* __restrict__ root, uint32_t n,
                                                           const uint32_t* __restrict__ block_offsets,
                                                           uint32_t* __restrict__ new_id, float* __restrict__ vertices,
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
            vertices[3 * (size_t)off] = soup[3 * (size_t)v];
            vertices[3 * (size_t)off + 1] = soup[3 * (size_t)v + 1];
            vertices[3 * (size_t)off + 2] = soup[3 * (size_t)v + 2];
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

uint32_t n_blocks(uint64_t n) { return (uint32_t)((n + CHUNK - 1) / CHUNK); }

}  // namespace

uint64_t mcubes_offset_words(uint32_t X, uint32_t Y, uint32_t Z) {
    const uint64_t n = (uint64_t)X * Y * Z;
    if (n >= (1ull << 31)) return 0;
    return (uint64_t)n_blocks(n) + 1;
}

uint64_t mcubes_weld_slots(uint32_t T) {
    if (T > 0x0FFFFFFFu) return 0;
    uint64_t s = 1024;
    while (s < 6ull * T) s <<= 1;
    return s;
}

uint64_t mcubes_weld_words(uint32_t T) {
    const uint64_t slots = mcubes_weld_slots(T);
    if (slots == 0) return 0;
    const uint64_t n = 3ull * T;
    return 4 * slots + 3 * n + n_blocks(n) + 1;
}

}  // namespace mipsf

using namespace mipsf;

static int mcubes_check(const mipsf_mcubes_args* a, const char* who) {
    MIPSF_ARGS(a, mipsf_mcubes_args, who);
    MIPSF_REQUIRE(a->X >= 1 && a->Y >= 1 && a->Z >= 1 && mcubes_offset_words(a->X, a->Y, a->Z) != 0,
                  "%s: volume %u x %u x %u is empty or has 2^31 cells or more", who, a->X, a->Y, a->Z);
    MIPSF_REQUIRE(a->volume && a->cases && a->block_offsets, "%s: null pointer", who);
    MIPSF_REQUIRE(((uintptr_t)a->cases & 15u) == 0 && ((uintptr_t)a->volume & 3u) == 0, "%s: cases must be 16-byte aligned", who);
    MIPSF_REQUIRE(a->truncation == a->truncation && a->isovalue == a->isovalue, "%s: NaN parameter", who);
    return 0;
}

extern "C" int mipsf_mcubes_count(const mipsf_mcubes_args* a, void* stream) {
    if (int rc = mcubes_check(a, "mipsf_mcubes_count")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = a->X * a->Y * a->Z, nb = n_blocks(n);
    const dim3 grid((a->Z + BZ - 1) / BZ, (a->Y + BY - 1) / BY, (a->X + BX - 1) / BX);
    MIPSF_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "mipsf_mcubes_count: volume too large for one launch");
    hipLaunchKernelGGL(mcubes_classify_kernel, grid, dim3(256), 0, s, a->volume, (int)a->X, (int)a->Y, (int)a->Z, a->isovalue,
                       a->truncation, a->cases);
    hipLaunchKernelGGL(mcubes_reduce_kernel, dim3(nb), dim3(256), 0, s, a->cases, n, a->block_offsets);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, s, a->block_offsets, nb);
    return check_launch("mcubes_count");
}

extern "C" int mipsf_mcubes_emit(const mipsf_mcubes_args* a, void* stream) {
    if (int rc = mcubes_check(a, "mipsf_mcubes_emit")) return rc;
    if (a->capacity_tris == 0) return 0;
    MIPSF_REQUIRE(a->soup != nullptr, "mipsf_mcubes_emit: null soup");
    const uint32_t n = a->X * a->Y * a->Z;
    hipLaunchKernelGGL(mcubes_emit_kernel, dim3(n_blocks(n)), dim3(256), 0, (hipStream_t)stream, a->volume, (int)a->X, (int)a->Y,
                       (int)a->Z, a->isovalue, a->cases, a->block_offsets, a->soup, a->cell_ids, a->capacity_tris);
    return check_launch("mcubes_emit");
}

extern "C" int mipsf_mcubes_weld(const mipsf_mcubes_weld_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_mcubes_weld_args, "mipsf_mcubes_weld");
    MIPSF_REQUIRE(a->counts != nullptr && a->scratch != nullptr, "mipsf_mcubes_weld: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->scratch & 7u) == 0, "mipsf_mcubes_weld: scratch must be 8-byte aligned");
    const uint64_t slots = mcubes_weld_slots(a->T);
    MIPSF_REQUIRE(slots != 0, "mipsf_mcubes_weld: %u triangles are too many", a->T);
    MIPSF_REQUIRE(a->T == 0 || (a->soup && a->vertices && a->faces), "mipsf_mcubes_weld: null pointer");
    MIPSF_REQUIRE(a->max_rounds >= 1 && a->max_rounds <= 64, "mipsf_mcubes_weld: max_rounds %u outside 1..64", a->max_rounds);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = 3 * a->T, nb = n_blocks(n), g = (n + 255) / 256;
    WeldTable tb;
    tb.xy = reinterpret_cast<unsigned long long*>(a->scratch);
    tb.z = a->scratch + 2 * slots;
    tb.val = a->scratch + 3 * slots;
    tb.mask = (uint32_t)slots - 1;
    uint32_t* slot_of = a->scratch + 4 * slots;
    uint32_t* root = slot_of + n;
    uint32_t* new_id = root + n;
    uint32_t* offsets = new_id + n;
    hipLaunchKernelGGL(weld_clear_kernel, dim3((uint32_t)(slots / 256)), dim3(256), 0, s, tb, a->counts);
    if (n == 0) return check_launch("mcubes_weld");
    hipLaunchKernelGGL(weld_insert_kernel, dim3(g), dim3(256), 0, s, a->soup, n, tb, slot_of, a->counts);
    hipLaunchKernelGGL(weld_owner_kernel, dim3(g), dim3(256), 0, s, n, tb, slot_of);
    for (uint32_t r = 0; r < a->max_rounds; ++r)
        hipLaunchKernelGGL(weld_round_kernel, dim3(g), dim3(256), 0, s, a->soup, n, tb, slot_of, a->counts, r);
    hipLaunchKernelGGL(weld_root_kernel, dim3(g), dim3(256), 0, s, n, tb, slot_of, root);
    hipLaunchKernelGGL(weld_reduce_kernel, dim3(nb), dim3(256), 0, s, root, n, offsets);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, s, offsets, nb);
    hipLaunchKernelGGL(weld_compact_kernel, dim3(nb), dim3(256), 0, s, a->soup, root, n, offsets, new_id, a->vertices, a->counts);
    hipLaunchKernelGGL(weld_faces_kernel, dim3(g), dim3(256), 0, s, root, new_id, n, a->faces);
    return check_launch("mcubes_weld");
}
