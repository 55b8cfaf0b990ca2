// Views taken out of the brick-sparse TSDF volume again, and the per-brick history that makes it possible
// (include/mipsf_sparse_remove.h).  Upstream has no TSDF code; the rules are this project's own.  DESIGN.md 4.27.
//
// The stamp: a lane per slot writes the id of the first view the slot takes where none is written yet, and a launch of one lane
// moves the serial on afterwards; the order of the two on the stream is what keeps the read of the serial from its update.
//
// The removal has the shape of sparse_integrate_kernel (sparse.hip, tsdf.hip where the shape is argued): a workgroup of 256 lanes
// owns a slot, a lane a run of 4 voxels along z, contiguous in the slot, whose words live in registers across all views; per chunk
// of 256 views one lane per view tests the brick's ball and the history, the survivors go to LDS in ascending order and every lane
// walks that list.  What a view does to a voxel -- the ball test, the projection, `updated` -- and the step on the running words
// are tsdf_dev.h's, the code the dense removal runs.
#include "block_dev.h"
#include "sparse_dev.h"
#include "../../include/mipsf_sparse_remove.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t BX = BRICK_X, BY = BRICK_Y, BZ = BRICK_Z;
constexpr uint32_t SLOT = BRICK_VOXELS;
constexpr uint32_t RUN = 4;                       // voxels of a lane, along z
constexpr uint32_t CHUNK = MIPSF_TSDF_VIEW_CHUNK;
constexpr uint32_t UNBORN = MIPSF_SPARSE_UNBORN;
static_assert(BX * BY * (BZ / RUN) == TPB, "one lane per run of the brick");
static_assert(CHUNK == TPB, "one lane per view of a chunk");
static_assert(sizeof(mipsf_sparse_remove_record) == 40, "remove record");

// p[0..n) = 0: the clear of the record is a launch, not a memset node, so that a captured graph replays it as it replays the kernels
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) sparse_remove_clear_kernel(uint32_t* __restrict__ p, uint32_t n) {
    if (threadIdx.x < n) p[threadIdx.x] = 0u;
}

// ------------------------------------------------------------------------------------------------ the history
// grid: blocks of 256 slots
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_stamp_kernel(Pool v, uint32_t* __restrict__ born, const uint32_t* __restrict__ serial) {
    const uint32_t slot = blockIdx.x * TPB + threadIdx.x;
    if (slot >= min(*v.count, v.capacity)) return;
    if (born[slot] == UNBORN) born[slot] = *serial + v.birth[slot];
}

// ONE lane, after the stamp on the stream
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) sparse_serial_kernel(uint32_t* __restrict__ serial, uint32_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *serial = *serial + n;
}

// ------------------------------------------------------------------------------------------------ the removal
// grid: one block per slot of the pool; those not in use return
template <bool COLOR>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) sparse_remove_kernel(Pool vol, TsdfFrames s, const uint32_t* __restrict__ view_ids,
                                                                             const uint32_t* __restrict__ born_of,
                                                                             mipsf_sparse_remove_record* __restrict__ record) {
    __shared__ uint32_t list[CHUNK];
    __shared__ uint32_t wave_count[WAVES];
    __shared__ uint64_t sm[WAVES];
    const uint32_t slot = blockIdx.x;
    if (slot >= min(*vol.count, vol.capacity)) return;                          // the whole block
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t brick = (uint32_t)vol.slot_brick[slot], born = born_of[slot];
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

    // the ball that holds the brick's voxels (every lane the same); a brick without one takes every view of its history
    TsdfGrid grid = {};
    for (int d = 0; d < 3; ++d) grid.ticks[d] = vol.ticks[d];
    double c[3], radius;
    const bool ball = tsdf_brick_ball(grid, x0, x1, y0, y1, z0, z1, c, radius);
    const bool cull = !(s.flags & MIPSF_TSDF_NO_CULL) && ball;

    const size_t hw = (size_t)s.H * s.W;
    uint64_t removed = 0, missing = 0, emptied = 0;
    for (uint32_t first = 0; first < s.n; first += CHUNK) {
        // ---- which views of the chunk the brick holds and can have taken, in ascending order
        const uint32_t k = first + tid;
        const bool keep = k < s.n && born != UNBORN && view_ids[k] >= born && (!cull || tsdf_view_can_update(s, k, c, radius));
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
            const TsdfViewRow row = tsdf_view_row(P, px, py);
#pragma unroll
            for (uint32_t r = 0; r < RUN; ++r) {
                size_t pixel;
                double val;
                if (!(ok[r] && tsdf_view_hits(s, row, D, pz[r], pixel, val))) continue;
                tsdf_remove_step<COLOR>(tsdf[r], weight[r], color + (COLOR ? r * 3 : 0), val, COLOR ? s.rgb + ((size_t)view * hw + pixel) * 3 : nullptr,
                                        removed, missing, emptied);
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
    removed = block_reduce<WAVES>(removed, sm, Add());
    missing = block_reduce<WAVES>(missing, sm, Add());
    emptied = block_reduce<WAVES>(emptied, sm, Add());
    observed = block_reduce<WAVES>(observed, sm, Add());
    if (tid == 0) {
        if (removed) atomicAdd((unsigned long long*)&record->removed, (unsigned long long)removed);
        if (missing) atomicAdd((unsigned long long*)&record->missing, (unsigned long long)missing);
        if (emptied) atomicAdd((unsigned long long*)&record->emptied, (unsigned long long)emptied);
        if (observed)
            atomicAdd((unsigned long long*)&record->observed, (unsigned long long)observed);
        else
            atomicAdd((unsigned long long*)&record->bricks_emptied, 1ull);      // the workgroup owns the slot: no voxel of it is left
    }
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" int mipsf_sparse_stamp(const mipsf_sparse_stamp_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_stamp_args, "mipsf_sparse_stamp");
    if (volume_ok(a->vol, "mipsf_sparse_stamp")) return 1;
    MIPSF_REQUIRE(a->n <= MIPSF_SPARSE_MAX_VIEWS, "mipsf_sparse_stamp: %u views, at most %u a call", a->n, MIPSF_SPARSE_MAX_VIEWS);
    MIPSF_REQUIRE(a->born && a->serial, "mipsf_sparse_stamp: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Pool v = pool_of(a->vol);
    hipLaunchKernelGGL(sparse_stamp_kernel, dim3(blocks_for(v.capacity, TPB)), dim3(TPB), 0, st, v, a->born, (const uint32_t*)a->serial);
    hipLaunchKernelGGL(sparse_serial_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, a->serial, a->n);
    return check_launch("sparse_stamp");
}

extern "C" int mipsf_sparse_deintegrate(const mipsf_sparse_deintegrate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_sparse_deintegrate_args, "mipsf_sparse_deintegrate");
    if (volume_ok(a->vol, "mipsf_sparse_deintegrate") || images_ok(a->n, a->H, a->W, a->fx, a->fy, a->cx, a->cy, "mipsf_sparse_deintegrate")) return 1;
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_sparse_deintegrate: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_sparse_deintegrate: depth_max is not a number");
    MIPSF_REQUIRE((a->flags & ~MIPSF_TSDF_NO_CULL) == 0, "mipsf_sparse_deintegrate: flags %u", a->flags);
    MIPSF_REQUIRE(a->n == 0 || (a->rgb != nullptr) == (a->vol.color != nullptr), "mipsf_sparse_deintegrate: rgb and color go together (rgb %s, color %s)",
                  a->rgb ? "given" : "null", a->vol.color ? "given" : "null");
    MIPSF_REQUIRE(a->record && a->born && (a->n == 0 || (a->depth && a->poses && a->view_ids)), "mipsf_sparse_deintegrate: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sparse_remove_clear_kernel, dim3(1), dim3(MIPSF_WAVE), 0, st, (uint32_t*)a->record,
                       (uint32_t)(sizeof(mipsf_sparse_remove_record) / sizeof(uint32_t)));
    const Pool v = pool_of(a->vol);
    const TsdfFrames s = {a->depth, a->rgb, a->poses, a->n, a->H, a->W, a->flags, a->fx, a->fy, a->cx, a->cy, a->trunc, a->depth_max, INFINITY};
    if (v.color)
        hipLaunchKernelGGL(sparse_remove_kernel<true>, dim3(v.capacity), dim3(TPB), 0, st, v, s, a->view_ids, a->born, a->record);
    else
        hipLaunchKernelGGL(sparse_remove_kernel<false>, dim3(v.capacity), dim3(TPB), 0, st, v, s, a->view_ids, a->born, a->record);
    return check_launch("sparse_remove");
}
