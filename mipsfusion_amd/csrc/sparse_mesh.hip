// The mesh of a brick-sparse volume, marched brick by brick (include/mipsf_sparse_mesh.h): no dense window, and a
// virtual grid of 2^31 voxels and more in one call.  The rule is the dense marcher's (mcubes_dev.h) on the block of a brick: the brick
// plus one voxel on every side, read through the table.
//
// Shape of the kernels.  Count and emit: a workgroup per slot, as the fusion; the 27 table words of the neighbourhood go to LDS once,
// then the 10 x 10 x 18 block with invalid voxels as NaN (3.6 KB of halo per 4 KB of brick, each word read once), then the 9 x 9 x 17
// dual values: mcubes_classify_kernel's scheme with the brick as the tile.  A lane owns four consecutive cells along z, the words of
// its run in the slot.  The emit stages the block again and reads its dual values from LDS: the same function, so the same words.
// The slots' triangle counts are summed by block_dev.h's scans (tile sums, one block, the tiles again) under the mask of the count.
// The weld is mcubes_dev.h's with the brick's base added to a vertex's cell.
#include "mcubes_dev.h"
#include "sparse_dev.h"
#include "../../include/mipsf_sparse_mesh.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int VX = BRICK_X + 2, VY = BRICK_Y + 2, VZ = BRICK_Z + 2;          // voxels of a block
constexpr int DX = BRICK_X + 1, DY = BRICK_Y + 1, DZ = BRICK_Z + 1;          // its dual values
constexpr uint32_t RUN = 4;                                                  // cells of a lane, along z
constexpr float ISO = 0.0f, TRUNC = 1.0f;
static_assert(BRICK_X * BRICK_Y * (BRICK_Z / RUN) == TPB, "one lane per run of the brick");
static_assert(TPB * SCAN_ITEMS == MIPSF_SPARSE_MESH_SCAN_TILE, "a tile of the prefix sum");
static_assert(WAVES == TPB / MIPSF_WAVE, "the scans of a workgroup");

struct Block {
    float vox[VX * VY * VZ];
    float du[DX * DY * DZ];
    int32_t near[27];                   // the slots of the 27 bricks around, -1: none
};

// the slots in use
__device__ __forceinline__ uint32_t in_use(const Pool& v) { return min(*v.count, v.capacity); }

// the brick of a slot as coordinates; false: slot_brick does not hold a brick of the grid
__device__ __forceinline__ bool brick_at(const int32_t* slot_brick, uint32_t slot, uint32_t bricks, uint32_t bricks_y, uint32_t bricks_z, int b[3]) {
    const uint32_t brick = (uint32_t)slot_brick[slot];
    if (brick >= bricks) return false;
    b[2] = (int)(brick % bricks_z), b[1] = (int)((brick / bricks_z) % bricks_y), b[0] = (int)(brick / (bricks_z * bricks_y));
    return true;
}

// The block of the slot's brick in LDS: the marching volume with invalid voxels (no slot, low weight, -inf, at or beyond the
// truncation, outside the grid) as NaN, then the dual values, NaN exactly where one of the eight voxels is invalid.  Every thread of
// the workgroup makes the call; false (in every thread): the slot holds no brick of the grid.
__device__ __forceinline__ bool stage_block(const Pool& v, float min_weight, uint32_t slot, Block& s) {
    const int tid = threadIdx.x;
    int b[3];
    if (!brick_at(v.slot_brick, slot, v.bricks, v.bricks_y, v.bricks_z, b)) return false;
    const int bricks_x = (int)((v.X + BRICK_X - 1) / BRICK_X);
    if (tid < 27) {
        const int nx = b[0] + tid / 9 - 1, ny = b[1] + (tid / 3) % 3 - 1, nz = b[2] + tid % 3 - 1;
        int32_t at = -1;
        if (nx >= 0 && nx < bricks_x && ny >= 0 && ny < (int)v.bricks_y && nz >= 0 && nz < (int)v.bricks_z) {
            at = v.table[((size_t)nx * v.bricks_y + ny) * v.bricks_z + nz];
            if (at < 0 || (uint32_t)at >= v.capacity) at = -1;              // nothing is read beyond the pool
        }
        s.near[tid] = at;
    }
    __syncthreads();
    const int i0 = b[0] * (int)BRICK_X - 1, j0 = b[1] * (int)BRICK_Y - 1, k0 = b[2] * (int)BRICK_Z - 1;
    for (int t = tid; t < VX * VY * VZ; t += TPB) {
        const int c = t % VZ, bb = (t / VZ) % VY, a = t / (VZ * VY);
        const int gi = i0 + a, gj = j0 + bb, gk = k0 + c;
        float val = __builtin_nanf("");
        if (gi >= 0 && gi < (int)v.X && gj >= 0 && gj < (int)v.Y && gk >= 0 && gk < (int)v.Z) {
            const int32_t at = s.near[((a == 0 ? 0 : a == VX - 1 ? 2 : 1) * 3 + (bb == 0 ? 0 : bb == VY - 1 ? 2 : 1)) * 3 + (c == 0 ? 0 : c == VZ - 1 ? 2 : 1)];
            if (at >= 0) {
                const size_t word = (size_t)at * BRICK_VOXELS + ((gi % (int)BRICK_X) * BRICK_Y + gj % (int)BRICK_Y) * BRICK_Z + gk % (int)BRICK_Z;
                const float d = v.tsdf[word];
                if (v.weight[word] >= min_weight && d != -INFINITY && fabsf(d) < TRUNC) val = d;
            }
        }
        s.vox[t] = val;
    }
    __syncthreads();
    for (int t = tid; t < DX * DY * DZ; t += TPB) {
        const int c = t % DZ, bb = (t / DZ) % DY, a = t / (DZ * DY);
        const float* p = s.vox + (a * VY + bb) * VZ + c;
        s.du[t] = dual_sum(p[0], p[VY * VZ], p[VZ], p[1], p[VY * VZ + VZ], p[VZ + 1], p[VY * VZ + 1], p[VY * VZ + VZ + 1]);
    }
    __syncthreads();
    return true;
}

// the eight dual values of the brick's cell (a, b, c), 0-based within the brick; false: one of them is invalid
__device__ __forceinline__ bool cell_corners(const Block& s, int a, int b, int c, float d[8]) {
    bool valid = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        d[q] = s.du[((a + (q >> 2)) * DY + b + ((q >> 1) & 1)) * DZ + c + (q & 1)];
        valid = valid && (d[q] == d[q]);
    }
    return valid;
}

// grid: one workgroup per slot of the pool; those not in use return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_mesh_classify_kernel(Pool v, float min_weight, uint32_t* __restrict__ cases,
                                                                                    uint32_t* __restrict__ offsets) {
    __shared__ Block s;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    if (slot >= in_use(v)) return;                                              // the whole workgroup
    uint32_t word = 0, mine = 0;
    if (stage_block(v, min_weight, slot, s)) {
        const int a = tid >> 5, b = (tid >> 2) & 7, c0 = (tid & 3) * RUN;
#pragma unroll
        for (uint32_t r = 0; r < RUN; ++r) {
            float d[8];
            const bool valid = cell_corners(s, a, b, c0 + (int)r, d);
            uint32_t code = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) code |= (d[q] < ISO ? 1u : 0u) << q;
            if (!valid || k_ntri[code] == 0) code = 0;                          // no crossing, or one of the patterns that emit nothing
            if (code != 0 && thresh_rejects(d, MIPSF_MCUBES_THRESH)) code = 0;
            word |= code << (8 * r);
            mine += k_ntri[code];
        }
    }
    cases[(size_t)slot * TPB + tid] = word;                                     // the lane's four case bytes
    const uint32_t total = block_reduce<WAVES>(mine, wsum, Add());
    if (tid == 0) offsets[slot] = total;
}

// the triangles of slot s as mipsf_sparse_mesh_count left them before the scan; none beyond the count
__device__ __forceinline__ uint32_t slot_tris(const Pool& v, const uint32_t* offsets, uint64_t s, uint32_t used) { return s < used ? offsets[s] : 0u; }

// grid: tiles of 1024 slots
__global__ void __launch_bounds__(TPB) sparse_mesh_tile_kernel(Pool v, const uint32_t* __restrict__ offsets, uint64_t* __restrict__ sums) {
    __shared__ uint64_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    const uint32_t used = in_use(v);
    uint64_t mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) mine += slot_tris(v, offsets, base + e, used);
    mine = block_reduce<WAVES>(mine, sm, Add());
    if (threadIdx.x == 0) sums[blockIdx.x] = mine;
}

// ONE block: the tile sums become their exclusive scan; offsets[capacity] = T
__global__ void __launch_bounds__(TPB) sparse_mesh_top_kernel(Pool v, uint32_t* __restrict__ offsets, uint64_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint64_t sm[WAVES];
    const uint64_t total = scan_top<WAVES>(sums, nb, sm);
    if (threadIdx.x == 0) offsets[v.capacity] = total > 0xfffffffeull ? 0xffffffffu : (uint32_t)total;
}

// grid: the tiles again; in place
__global__ void __launch_bounds__(TPB) sparse_mesh_apply_kernel(Pool v, uint32_t* __restrict__ offsets, const uint64_t* __restrict__ sums) {
    __shared__ uint32_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    const uint32_t used = in_use(v);
    uint32_t val[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        val[e] = slot_tris(v, offsets, base + e, used);
        mine += val[e];
    }
    uint32_t run = block_excl_scan<WAVES>(mine, sm) + (uint32_t)sums[blockIdx.x];       // exact while T is below 2^32
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        if (base + e < v.capacity) offsets[base + e] = run;
        run += val[e];
    }
}

// grid: one workgroup per slot of the pool; those not in use, and those without a triangle, return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_mesh_emit_kernel(Pool v, float min_weight, const uint32_t* __restrict__ cases,
                                                                                const uint32_t* __restrict__ offsets, float* __restrict__ soup,
                                                                                int32_t* __restrict__ tri_slot, int32_t* __restrict__ cell_ids,
                                                                                uint32_t capacity_tris) {
    __shared__ Block s;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    if (slot >= in_use(v)) return;                                              // the whole workgroup
    const uint32_t first = offsets[slot];
    if (offsets[slot + 1] == first) return;
    if (!stage_block(v, min_weight, slot, s)) return;
    const uint32_t word = cases[(size_t)slot * TPB + tid];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < RUN; ++r) mine += k_ntri[(word >> (8 * r)) & 0xffu];
    uint32_t off = first + block_excl_scan<WAVES>(mine, wsum);
    if (mine == 0) return;
    const int a = tid >> 5, b = (tid >> 2) & 7, c0 = (tid & 3) * RUN;
    for (uint32_t r = 0; r < RUN; ++r) {
        const uint32_t code = (word >> (8 * r)) & 0xffu;
        const uint32_t nt = k_ntri[code];
        if (nt == 0) continue;
        const int c = c0 + (int)r;
        float d[8];
        cell_corners(s, a, b, c, d);
        const float ci = (float)(a + 1), cj = (float)(b + 1), ck = (float)(c + 1);       // the cell in the block's coordinates
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t o = off + t;
            if (o >= capacity_tris) break;
            for (int w = 0; w < 3; ++w) {
                const int e = k_tri[code][3 * t + w];
                const int c1 = k_edge_ends[e][0], c2 = k_edge_ends[e][1];
                Vec3 p1, p2;
                p1.x = ci + ((c1 >> 2) & 1 ? 0.5f : -0.5f);
                p1.y = cj + ((c1 >> 1) & 1 ? 0.5f : -0.5f);
                p1.z = ck + (c1 & 1 ? 0.5f : -0.5f);
                p2.x = ci + ((c2 >> 2) & 1 ? 0.5f : -0.5f);
                p2.y = cj + ((c2 >> 1) & 1 ? 0.5f : -0.5f);
                p2.z = ck + (c2 & 1 ? 0.5f : -0.5f);
                const Vec3 p = edge_vertex(ISO, p1, p2, d[c1], d[c2]);
                float* dst = soup + (size_t)o * 9 + 3 * w;
                dst[0] = p.x, dst[1] = p.y, dst[2] = p.z;
            }
            tri_slot[o] = (int32_t)slot;
            if (cell_ids) cell_ids[o] = (int32_t)((a * (int)BRICK_Y + b) * (int)BRICK_Z + c);
        }
        off += nt;
    }
}

// the sparse weld's cells: the brick's base on the global weld grid plus the local coordinate's cell; a surviving vertex is written
// in index units of the virtual grid, exactly
struct BrickCells {
    const float* soup;
    const int32_t* tri_slot;
    const int32_t* slot_brick;
    double* vertices;
    uint32_t capacity, bricks, bricks_y, bricks_z;

    __device__ __forceinline__ bool base_of(uint32_t v, int base[3]) const {
        const uint32_t slot = (uint32_t)tri_slot[v / 3];
        int b[3];
        if (slot >= capacity || !brick_at(slot_brick, slot, bricks, bricks_y, bricks_z, b)) return false;
        base[0] = b[0] * (int)BRICK_X - 1, base[1] = b[1] * (int)BRICK_Y - 1, base[2] = b[2] * (int)BRICK_Z - 1;
        return true;
    }
    __device__ __forceinline__ void cell(uint32_t v, int& x, int& y, int& z) const {
        int base[3], q[3] = {-1, -1, -1};
        if (base_of(v, base)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const long long at = (long long)base[a] * 100000ll + (long long)weld_quantise(soup[3 * (size_t)v + a]);
                q[a] = at < 0 || at > 0x7ffffffell ? -1 : (int)at;
            }
        }
        x = q[0], y = q[1], z = q[2];
    }
    __device__ __forceinline__ void keep(uint32_t v, uint32_t id) const {
        int base[3] = {0, 0, 0};
        base_of(v, base);
#pragma unroll
        for (int a = 0; a < 3; ++a) vertices[3 * (size_t)id + a] = (double)base[a] + (double)soup[3 * (size_t)v + a];
    }
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_sample_kernel(Pool v, const double* __restrict__ points, uint32_t m, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * TPB + threadIdx.x;
    if (p >= m) return;
    float res[3];
    sample_color(v, points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2], res);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[3 * (size_t)p + ch] = res[ch];
}

int mesh_ok(const mipsf_sparse_mesh_args* a, const char* who) {
    MIPSF_ARGS(a, mipsf_sparse_mesh_args, who);
    if (volume_ok(a->vol, who)) return 1;
    MIPSF_REQUIRE(a->min_weight == a->min_weight, "%s: min_weight is not a number", who);
    MIPSF_REQUIRE(a->cases && a->offsets, "%s: null pointer", who);
    MIPSF_REQUIRE(((uintptr_t)a->cases & 7u) == 0, "%s: cases must be 8-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_sparse_mesh_scan_words(uint32_t capacity) {
    if (capacity == 0 || capacity > MIPSF_SPARSE_MAX_CAPACITY) return 0;
    return 2ull * blocks_for(capacity, MIPSF_SPARSE_MESH_SCAN_TILE);
}

extern "C" int mipsf_sparse_mesh_count(const mipsf_sparse_mesh_args* a, void* stream) {
    if (int rc = mesh_ok(a, "mipsf_sparse_mesh_count")) return rc;
    MIPSF_REQUIRE(a->scan && ((uintptr_t)a->scan & 7u) == 0, "mipsf_sparse_mesh_count: scan is null or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Pool v = pool_of(a->vol);
    const uint32_t nb = blocks_for(v.capacity, MIPSF_SPARSE_MESH_SCAN_TILE);
    uint64_t* sums = reinterpret_cast<uint64_t*>(a->scan);
    hipLaunchKernelGGL(sparse_mesh_classify_kernel, dim3(v.capacity), dim3(TPB), 0, st, v, a->min_weight, reinterpret_cast<uint32_t*>(a->cases), a->offsets);
    hipLaunchKernelGGL(sparse_mesh_tile_kernel, dim3(nb), dim3(TPB), 0, st, v, (const uint32_t*)a->offsets, sums);
    hipLaunchKernelGGL(sparse_mesh_top_kernel, dim3(1), dim3(TPB), 0, st, v, a->offsets, sums, nb);
    hipLaunchKernelGGL(sparse_mesh_apply_kernel, dim3(nb), dim3(TPB), 0, st, v, a->offsets, (const uint64_t*)sums);
    return check_launch("sparse_mesh_count");
}

extern "C" int mipsf_sparse_mesh_emit(const mipsf_sparse_mesh_args* a, void* stream) {
    if (int rc = mesh_ok(a, "mipsf_sparse_mesh_emit")) return rc;
    if (a->capacity_tris == 0) return 0;
    MIPSF_REQUIRE(a->soup && a->tri_slot, "mipsf_sparse_mesh_emit: null pointer");
    const Pool v = pool_of(a->vol);
    hipLaunchKernelGGL(sparse_mesh_emit_kernel, dim3(v.capacity), dim3(TPB), 0, (hipStream_t)stream, v, a->min_weight,
                       reinterpret_cast<const uint32_t*>(a->cases), (const uint32_t*)a->offsets, a->soup, a->tri_slot, a->cell_ids, a->capacity_tris);
    return check_launch("sparse_mesh_emit");
}

extern "C" int mipsf_sparse_mesh_weld(const mipsf_sparse_mesh_weld_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_mesh_weld_args, "mipsf_sparse_mesh_weld");
    if (volume_ok(a->vol, "mipsf_sparse_mesh_weld")) return 1;
    const uint32_t side = a->vol.X > a->vol.Y ? (a->vol.X > a->vol.Z ? a->vol.X : a->vol.Z) : (a->vol.Y > a->vol.Z ? a->vol.Y : a->vol.Z);
    MIPSF_REQUIRE(side <= MIPSF_SPARSE_MESH_MAX_SIDE,
                  "mipsf_sparse_mesh_weld: a side of %u voxels (grid %u x %u x %u), at most %u: the weld keeps a vertex's cell on the 1e-5 grid in 32 bits", side,
                  a->vol.X, a->vol.Y, a->vol.Z, MIPSF_SPARSE_MESH_MAX_SIDE);
    MIPSF_REQUIRE(a->counts != nullptr && a->scratch != nullptr, "mipsf_sparse_mesh_weld: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->scratch & 7u) == 0, "mipsf_sparse_mesh_weld: scratch must be 8-byte aligned");
    const uint64_t slots = mcubes_weld_slots(a->T);
    MIPSF_REQUIRE(slots != 0, "mipsf_sparse_mesh_weld: %u triangles are too many for the weld table", a->T);
    MIPSF_REQUIRE(a->capacity_tris >= a->T, "mipsf_sparse_mesh_weld: capacity_tris %u is below the %u triangles of the soup", a->capacity_tris, a->T);
    MIPSF_REQUIRE(a->T == 0 || (a->soup && a->tri_slot && a->vertices && a->faces), "mipsf_sparse_mesh_weld: null pointer");
    MIPSF_REQUIRE(a->max_rounds >= 1 && a->max_rounds <= 64, "mipsf_sparse_mesh_weld: max_rounds %u outside 1..64", a->max_rounds);
    const Pool v = pool_of(a->vol);
    const BrickCells cells = {a->soup, a->tri_slot, v.slot_brick, a->vertices, v.capacity, v.bricks, v.bricks_y, v.bricks_z};
    weld_enqueue(cells, a->T, slots, a->scratch, a->faces, a->counts, a->max_rounds, (hipStream_t)stream);
    return check_launch("sparse_mesh_weld");
}

extern "C" int mipsf_sparse_sample(const mipsf_sparse_sample_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_sample_args, "mipsf_sparse_sample");
    if (volume_ok(a->vol, "mipsf_sparse_sample")) return 1;
    MIPSF_REQUIRE(a->vol.color != nullptr, "mipsf_sparse_sample: the volume has no colour");
    if (a->m == 0) return 0;
    MIPSF_REQUIRE(a->points && a->out, "mipsf_sparse_sample: null pointer");
    hipLaunchKernelGGL(sparse_sample_kernel, dim3(blocks_for(a->m, TPB)), dim3(TPB), 0, (hipStream_t)stream, pool_of(a->vol), a->points, a->m, a->out);
    return check_launch("sparse_sample");
}
