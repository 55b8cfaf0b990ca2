// Mesh extraction on the device: marching cubes over the dual grid of an SDF volume with the upstream extractor's semantics
// (include/mipsf_mesh.h).  count = classify + reduce + scan, emit, weld.  The order of the soup is defined by
// scans only (no atomics); the weld uses atomicMin / atomicCAS on a hash table, whose fixed point does not depend on scheduling.
#include "mcubes_dev.h"

namespace mipsf {

namespace {

constexpr int BX = 8, BY = 8, BZ = 32;          // cells of a classify workgroup
constexpr int VX = BX + 2, VY = BY + 2, VZ = BZ + 2;
constexpr int DX = BX + 1, DY = BY + 1, DZ = BZ + 1;

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

// the dense weld's cells: the soup's own floats on the weld grid; a surviving vertex keeps its floats
struct SoupCells {
    const float* soup;
    float* vertices;
    __device__ __forceinline__ void cell(uint32_t v, int& x, int& y, int& z) const {
        x = weld_quantise(soup[3 * (size_t)v]), y = weld_quantise(soup[3 * (size_t)v + 1]), z = weld_quantise(soup[3 * (size_t)v + 2]);
    }
    __device__ __forceinline__ void keep(uint32_t v, uint32_t id) const {
        vertices[3 * (size_t)id] = soup[3 * (size_t)v];
        vertices[3 * (size_t)id + 1] = soup[3 * (size_t)v + 1];
        vertices[3 * (size_t)id + 2] = soup[3 * (size_t)v + 2];
    }
};

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
    weld_enqueue(SoupCells{a->soup, a->vertices}, a->T, slots, a->scratch, a->faces, a->counts, a->max_rounds, (hipStream_t)stream);
    return check_launch("mcubes_weld");
}
