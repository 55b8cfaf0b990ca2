// Slots of the brick-sparse TSDF volume given back, archived and restored (include/mipsf_sparse_release.h).  Upstream has no TSDF
// code; the rules are this project's own.  DESIGN.md 4.28.
//
// Release.  A lane per slot reads six ticks and the box (OUTSIDE), a workgroup per slot reads the slot's 1024 weights (EMPTY, only
// when asked for); the candidate flags go through block_dev.h's device-wide prefix sum (tile sums, ONE block, the tiles again), which
// leaves per slot F = the released slots before it and the list of the released slots in ascending order.  F and the list are all
// the later launches need: entry k of the archive is slot list[k]; the j-th hole is list[j]; the rank of a tail survivor s among
// the tail survivors is (s - n') - (F[s] - F[n']).  A workgroup per slot of the tail n' .. n-1 moves a survivor into its hole and
// leaves the tail slot zero; it is also the one that clears table[] of the brick its hole held, before it overwrites slot_brick
// there (every hole receives exactly one survivor).  The old count stays in the volume until the last launch, one lane, which writes
// the record and the new count.
//
// Restore.  A lane per entry marks its brick with an integer atomic minimum of the entry's index; sparse.hip's own allocation
// launches (sparse_dev.h) number the marked bricks without a slot behind the slots in use and leave birth[slot] = the entry; a
// workgroup per new slot copies that entry's words.
//
// Words are moved as uint32: nothing is computed, and nothing can canonicalise a NaN's payload on the way.
#include "block_dev.h"
#include "sparse_dev.h"
#include "../../include/mipsf_sparse_release.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t SLOT = BRICK_VOXELS;
constexpr uint32_t UNBORN = MIPSF_SPARSE_UNBORN;
constexpr uint32_t NO_CAP = 0xffffffffu;
constexpr uint32_t PREDICATES = MIPSF_SPARSE_RELEASE_OUTSIDE | MIPSF_SPARSE_RELEASE_EMPTY;
static_assert(TPB * SCAN_ITEMS == MIPSF_SPARSE_SCAN_TILE, "a tile of the prefix sum");
static_assert(SLOT % TPB == 0, "a lane's words of a slot");
static_assert(sizeof(mipsf_sparse_release_record) == 56 && sizeof(mipsf_sparse_restore_record) == 56, "records");

// the scratch of a release, in uint32 words: the head, then three arrays of `capacity` words, then the tile sums
constexpr uint32_t HEAD = 16;                     // words 0..3 below, the two 64-bit counts at words 4 and 6
enum { H_BEFORE = 0, H_AFTER = 1, H_RELEASED = 2, H_CANDIDATES = 3, H_OUTSIDE = 4, H_EMPTY = 6 };
struct Work {
    uint32_t* head;                     // [HEAD]
    uint32_t* flags;                    // [capacity] the predicates that hold for a slot in use, 0 beyond
    uint32_t* before;                   // [capacity] F
    uint32_t* list;                     // [capacity] the released slots, ascending
    uint32_t* sums;                     // [tiles + 1]
    uint32_t cap;                       // the archive's entries, or NO_CAP
};

struct Archive {
    int32_t* brick;
    uint32_t* born;
    uint32_t* tsdf;
    uint32_t* weight;
    uint32_t* color;
};

inline uint32_t least(uint32_t a, uint32_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint32_t in_use(const Pool& v) { return min(*v.count, v.capacity); }

// the words of slot `from` of (tsdf, weight, color) to slot `to` of (tsdf_to, ..): a lane takes words tid, tid + 256, ..
__device__ __forceinline__ void copy_slot(const uint32_t* tsdf, const uint32_t* weight, const uint32_t* color, uint32_t from, uint32_t* tsdf_to,
                                          uint32_t* weight_to, uint32_t* color_to, uint32_t to) {
    const size_t a = (size_t)from * SLOT, b = (size_t)to * SLOT;
    for (uint32_t w = threadIdx.x; w < SLOT; w += TPB) {
        tsdf_to[b + w] = tsdf[a + w];
        weight_to[b + w] = weight[a + w];
    }
    if (color) {
        for (uint32_t w = threadIdx.x; w < SLOT * 3; w += TPB) color_to[b * 3 + w] = color[a * 3 + w];
    }
}

// ------------------------------------------------------------------------------------------------ release: the predicates
// grid: blocks of 256 slots; flags[s] for every slot of the pool
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_outside_kernel(Pool v, Work k, const double* __restrict__ box, uint32_t flags) {
    const uint32_t s = blockIdx.x * TPB + threadIdx.x;
    if (s >= v.capacity) return;
    uint32_t holds = 0;
    if (s < in_use(v) && (flags & MIPSF_SPARSE_RELEASE_OUTSIDE)) {
        const uint32_t brick = (uint32_t)v.slot_brick[s];
        const uint32_t b[3] = {brick / (v.bricks_z * v.bricks_y), (brick / v.bricks_z) % v.bricks_y, brick % v.bricks_z};
        const uint32_t B[3] = {BRICK_X, BRICK_Y, BRICK_Z}, D[3] = {v.X, v.Y, v.Z};
        bool outside = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double blo = v.ticks[a][B[a] * b[a]], bhi = v.ticks[a][min(B[a] * b[a] + B[a] - 1u, D[a] - 1u)];
            outside = outside || bhi < box[a] || blo > box[3 + a];              // a NaN fails
        }
        holds = outside ? MIPSF_SPARSE_RELEASE_OUTSIDE : 0u;
    }
    k.flags[s] = holds;
}

// grid: one block per slot of the pool; those not in use return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_empty_kernel(Pool v, Work k) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t s = blockIdx.x;
    if (s >= in_use(v)) return;                                                 // the whole block
    uint32_t seen = 0;
    for (uint32_t w = threadIdx.x; w < SLOT; w += TPB) seen += v.weight[(size_t)s * SLOT + w] > 0.0f ? 1u : 0u;
    seen = block_reduce<WAVES>(seen, sm, Add());
    if (threadIdx.x == 0 && seen == 0) k.flags[s] |= MIPSF_SPARSE_RELEASE_EMPTY;
}

// ------------------------------------------------------------------------------------------------ release: the prefix sum
// grid: tiles of 1024 slots; sums[tile] = candidates of the tile
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_tile_kernel(Pool v, Work k) {
    __shared__ uint32_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) mine += base + e < v.capacity && k.flags[base + e] ? 1u : 0u;
    mine = block_reduce<WAVES>(mine, sm, Add());
    if (threadIdx.x == 0) k.sums[blockIdx.x] = mine;
}

// ONE block: the tile sums become their exclusive scan; the head takes the counts.  The volume's count is left as it is.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_top_kernel(Pool v, Work k, uint32_t nb) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t total = scan_top<WAVES>(k.sums, nb, sm);
    if (threadIdx.x == 0) {
        const uint32_t n = in_use(v), released = min(total, k.cap);
        k.head[H_BEFORE] = n;
        k.head[H_AFTER] = n - released;
        k.head[H_RELEASED] = released;
        k.head[H_CANDIDATES] = total;
        k.head[H_OUTSIDE] = k.head[H_OUTSIDE + 1] = k.head[H_EMPTY] = k.head[H_EMPTY + 1] = 0u;
    }
}

// grid: the tiles again; F and the list of the released slots
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_apply_kernel(Pool v, Work k) {
    __shared__ uint32_t sm[WAVES];
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * SCAN_ITEMS;
    uint32_t f[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        f[e] = base + e < v.capacity ? k.flags[base + e] : 0u;
        mine += f[e] ? 1u : 0u;
    }
    uint32_t run = block_excl_scan<WAVES>(mine, sm) + k.sums[blockIdx.x];       // R of the lane's first slot
    uint32_t outside = 0, empty = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        if (base + e < v.capacity) k.before[base + e] = min(run, k.cap);
        if (f[e]) {
            if (run < k.cap) {
                k.list[run] = (uint32_t)(base + e);                             // run < candidates <= capacity
                outside += f[e] & MIPSF_SPARSE_RELEASE_OUTSIDE ? 1u : 0u;
                empty += f[e] & MIPSF_SPARSE_RELEASE_EMPTY ? 1u : 0u;
            }
            ++run;
        }
    }
    outside = block_reduce<WAVES>(outside, sm, Add());
    empty = block_reduce<WAVES>(empty, sm, Add());
    if (threadIdx.x == 0) {
        if (outside) atomicAdd((unsigned long long*)(k.head + H_OUTSIDE), (unsigned long long)outside);
        if (empty) atomicAdd((unsigned long long*)(k.head + H_EMPTY), (unsigned long long)empty);
    }
}

// ------------------------------------------------------------------------------------------------ release: archive, move, count
// grid: one block per entry of the archive (at most `capacity`); entries at or beyond `released` return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_archive_kernel(Pool v, Work k, const uint32_t* born, Archive to) {
    const uint32_t e = blockIdx.x;
    if (e >= k.head[H_RELEASED]) return;                                        // the whole block
    const uint32_t s = k.list[e];
    copy_slot((const uint32_t*)v.tsdf, (const uint32_t*)v.weight, (const uint32_t*)v.color, s, to.tsdf, to.weight, to.color, e);
    if (threadIdx.x == 0) {
        to.brick[e] = v.slot_brick[s];
        if (born) to.born[e] = born[s];
    }
}

// grid: one block per slot of the tail (at most `capacity`): slot n' + blockIdx.x; those at or beyond n return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_release_move_kernel(Pool v, Work k, uint32_t* born) {
    const uint32_t after = k.head[H_AFTER];
    const uint32_t s = after + blockIdx.x;
    if (blockIdx.x >= k.head[H_RELEASED]) return;                               // the whole block: the tail has `released` slots
    const bool released = k.flags[s] && k.before[s] < k.cap;
    const int32_t brick = v.slot_brick[s];
    uint32_t* const tsdf = (uint32_t*)v.tsdf;
    uint32_t* const weight = (uint32_t*)v.weight;
    uint32_t* const color = (uint32_t*)v.color;
    if (!released) {
        // the rank among the tail survivors: the tail slots before s, less the released ones among them
        const uint32_t hole = k.list[blockIdx.x - (k.before[s] - k.before[after])];
        copy_slot(tsdf, weight, color, s, tsdf, weight, color, hole);
        if (threadIdx.x == 0) {
            v.table[v.slot_brick[hole]] = -1;                                   // the brick the hole held, before its word goes
            v.slot_brick[hole] = brick;
            v.table[brick] = (int32_t)hole;
            if (born) born[hole] = born[s];
        }
    } else if (threadIdx.x == 0) {
        v.table[brick] = -1;
    }
    // the tail slot is left as an unused slot is: the lane zeroes the words it read above
    const size_t a = (size_t)s * SLOT;
    for (uint32_t w = threadIdx.x; w < SLOT; w += TPB) tsdf[a + w] = 0u, weight[a + w] = 0u;
    if (color) {
        for (uint32_t w = threadIdx.x; w < SLOT * 3; w += TPB) color[a * 3 + w] = 0u;
    }
    if (threadIdx.x == 0 && born) born[s] = UNBORN;
}

// ONE lane, the last launch: the record, and the count moves
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) sparse_release_count_kernel(Pool v, Work k, mipsf_sparse_release_record* __restrict__ record) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t after = k.head[H_AFTER], released = k.head[H_RELEASED], candidates = k.head[H_CANDIDATES];
    record->candidates = candidates;
    record->released = released;
    record->released_outside = *(const uint64_t*)(k.head + H_OUTSIDE);
    record->released_empty = *(const uint64_t*)(k.head + H_EMPTY);
    record->deferred = candidates - released;
    record->moved = released ? k.before[after] : 0u;                            // the holes: the released slots below n'
    record->in_use = after;
    *v.count = after;
}

// ------------------------------------------------------------------------------------------------ restore
enum { R_ALLOC = 0, R_INVALID = 8 };              // words of the scratch: the allocation's record (4 x uint64), the invalid count

// grid: blocks of 256 entries
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_restore_mark_kernel(Pool v, const int32_t* __restrict__ brick, uint32_t m, uint32_t* __restrict__ mark,
                                                                                    uint32_t* __restrict__ scratch) {
    __shared__ uint32_t sm[WAVES];
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    uint32_t invalid = 0;
    if (e < m) {
        const int32_t b = brick[e];
        if (b >= 0 && (uint32_t)b < v.bricks)
            atomicMin(&mark[b], e);
        else
            invalid = 1;
    }
    invalid = block_reduce<WAVES>(invalid, sm, Add());
    if (threadIdx.x == 0 && invalid) atomicAdd(scratch + R_INVALID, invalid);
}

// grid: one block per entry (at most `capacity`): slot (count before) + blockIdx.x; those at or beyond the count return
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_restore_copy_kernel(Pool v, const uint32_t* __restrict__ scan, uint32_t nb, uint32_t* born, Archive from) {
    const uint32_t s = scan[nb] + blockIdx.x;
    if (s >= in_use(v)) return;                                                 // the whole block
    const uint32_t e = v.birth[s];
    copy_slot(from.tsdf, from.weight, from.color, e, (uint32_t*)v.tsdf, (uint32_t*)v.weight, (uint32_t*)v.color, s);
    if (threadIdx.x == 0 && born) born[s] = from.born[e];
}

// ONE lane
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) sparse_restore_record_kernel(const uint32_t* __restrict__ scratch, uint32_t m,
                                                                                             mipsf_sparse_restore_record* __restrict__ record) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const mipsf_sparse_alloc_record* got = (const mipsf_sparse_alloc_record*)(scratch + R_ALLOC);
    const uint64_t invalid = scratch[R_INVALID];
    record->listed = m;
    record->invalid = invalid;
    record->duplicates = ((uint64_t)m - invalid) - got->marked;
    record->occupied = (got->marked - got->created) - got->dropped;
    record->restored = got->created;
    record->dropped = got->dropped;
    record->in_use = got->in_use;
}

}  // namespace
}  // namespace mipsf

// ------------------------------------------------------------------------------------------------ host
using namespace mipsf;

extern "C" uint64_t mipsf_sparse_release_scratch_words(uint32_t capacity) {
    if (capacity == 0 || capacity > MIPSF_SPARSE_MAX_CAPACITY) return 0;
    return (uint64_t)HEAD + 3ull * capacity + blocks_for(capacity, MIPSF_SPARSE_SCAN_TILE) + 1u;
}

extern "C" int mipsf_sparse_release(const mipsf_sparse_release_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_release_args, "mipsf_sparse_release");
    if (volume_ok(a->vol, "mipsf_sparse_release")) return 1;
    MIPSF_REQUIRE((a->flags & ~(PREDICATES | MIPSF_SPARSE_RELEASE_ARCHIVE)) == 0, "mipsf_sparse_release: flags %u", a->flags);
    MIPSF_REQUIRE((a->flags & PREDICATES) != 0, "mipsf_sparse_release: flags %u name no predicate (OUTSIDE, EMPTY)", a->flags);
    MIPSF_REQUIRE(!(a->flags & MIPSF_SPARSE_RELEASE_OUTSIDE) || a->box, "mipsf_sparse_release: OUTSIDE needs a box");
    const bool archive = (a->flags & MIPSF_SPARSE_RELEASE_ARCHIVE) != 0;
    if (archive && a->archive_capacity > 0) {
        MIPSF_REQUIRE(a->arch_brick && a->arch_tsdf && a->arch_weight, "mipsf_sparse_release: null pointer in the archive");
        MIPSF_REQUIRE(a->arch_color || !a->vol.color, "mipsf_sparse_release: the volume has colour, the archive has no arch_color");
        MIPSF_REQUIRE(a->arch_born || !a->born, "mipsf_sparse_release: the volume has a history, the archive has no arch_born");
    }
    MIPSF_REQUIRE(a->scratch && ((uintptr_t)a->scratch & 7u) == 0, "mipsf_sparse_release: scratch is null or not aligned to 8 bytes");
    MIPSF_REQUIRE(a->record, "mipsf_sparse_release: null record");
    hipStream_t st = (hipStream_t)stream;
    const Pool v = pool_of(a->vol);
    const uint32_t C = v.capacity, nb = blocks_for(C, MIPSF_SPARSE_SCAN_TILE);
    Work k;
    k.head = a->scratch, k.flags = k.head + HEAD, k.before = k.flags + C, k.list = k.before + C, k.sums = k.list + C;
    k.cap = archive ? a->archive_capacity : NO_CAP;
    hipLaunchKernelGGL(sparse_release_outside_kernel, dim3(blocks_for(C, TPB)), dim3(TPB), 0, st, v, k, a->box, a->flags);
    if (a->flags & MIPSF_SPARSE_RELEASE_EMPTY) hipLaunchKernelGGL(sparse_release_empty_kernel, dim3(C), dim3(TPB), 0, st, v, k);
    hipLaunchKernelGGL(sparse_release_tile_kernel, dim3(nb), dim3(TPB), 0, st, v, k);
    hipLaunchKernelGGL(sparse_release_top_kernel, dim3(1), dim3(TPB), 0, st, v, k, nb);
    hipLaunchKernelGGL(sparse_release_apply_kernel, dim3(nb), dim3(TPB), 0, st, v, k);
    if (archive && a->archive_capacity > 0) {
        const Archive to = {a->arch_brick, a->born ? a->arch_born : nullptr, (uint32_t*)a->arch_tsdf, (uint32_t*)a->arch_weight,
                            v.color ? (uint32_t*)a->arch_color : nullptr};
        hipLaunchKernelGGL(sparse_release_archive_kernel, dim3(least(a->archive_capacity, C)), dim3(TPB), 0, st, v, k, (const uint32_t*)a->born, to);
    }
    if (k.cap > 0) hipLaunchKernelGGL(sparse_release_move_kernel, dim3(least(k.cap, C)), dim3(TPB), 0, st, v, k, a->born);
    hipLaunchKernelGGL(sparse_release_count_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, v, k, a->record);
    return check_launch("sparse_release");
}

extern "C" int mipsf_sparse_restore(const mipsf_sparse_restore_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_restore_args, "mipsf_sparse_restore");
    if (volume_ok(a->vol, "mipsf_sparse_restore")) return 1;
    MIPSF_REQUIRE(a->m <= MIPSF_SPARSE_MAX_CAPACITY, "mipsf_sparse_restore: %u entries, at most %u a call", a->m, MIPSF_SPARSE_MAX_CAPACITY);
    if (a->m > 0) {
        MIPSF_REQUIRE(a->arch_brick && a->arch_tsdf && a->arch_weight, "mipsf_sparse_restore: null pointer in the archive");
        MIPSF_REQUIRE((a->arch_color != nullptr) == (a->vol.color != nullptr), "mipsf_sparse_restore: arch_color and color go together (arch_color %s, color %s)",
                      a->arch_color ? "given" : "null", a->vol.color ? "given" : "null");
        MIPSF_REQUIRE((a->arch_born != nullptr) == (a->born != nullptr), "mipsf_sparse_restore: arch_born and born go together (arch_born %s, born %s)",
                      a->arch_born ? "given" : "null", a->born ? "given" : "null");
    }
    MIPSF_REQUIRE(a->mark && a->scan && a->record, "mipsf_sparse_restore: null pointer");
    MIPSF_REQUIRE(a->scratch && ((uintptr_t)a->scratch & 7u) == 0, "mipsf_sparse_restore: scratch is null or not aligned to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    sparse_fill(a->record, sizeof(mipsf_sparse_restore_record) / sizeof(uint32_t), 0u, st);
    if (a->m == 0) return check_launch("sparse_restore");
    const Pool v = pool_of(a->vol);
    const uint32_t nb = blocks_for(v.bricks, MIPSF_SPARSE_SCAN_TILE);
    mipsf_sparse_alloc_record* got = (mipsf_sparse_alloc_record*)(a->scratch + R_ALLOC);
    sparse_fill(a->scratch + R_INVALID, 1, 0u, st);
    sparse_marks_clear(v, a->mark, got, st);
    hipLaunchKernelGGL(sparse_restore_mark_kernel, dim3(blocks_for(a->m, TPB)), dim3(TPB), 0, st, v, a->arch_brick, a->m, a->mark, a->scratch);
    sparse_marks_assign(v, a->mark, a->scan, got, st);
    const Archive from = {nullptr, (uint32_t*)a->arch_born, (uint32_t*)a->arch_tsdf, (uint32_t*)a->arch_weight, (uint32_t*)a->arch_color};
    hipLaunchKernelGGL(sparse_restore_copy_kernel, dim3(least(a->m, v.capacity)), dim3(TPB), 0, st, v, (const uint32_t*)a->scan, nb, a->born, from);
    hipLaunchKernelGGL(sparse_restore_record_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, (const uint32_t*)a->scratch, a->m, a->record);
    return check_launch("sparse_restore");
}
