// Views taken out of the dense TSDF volume again (include/mipsf_deintegrate.h): the inverse of tsdf.hip's running mean, for the
// views a loop closure moved and for a frame that turned out to be bad.  Upstream has no TSDF code; the rule is this project's
// own.  DESIGN.md 4.26.
//
// The kernel has the shape of tsdf_integrate_kernel (tsdf.hip, where the shape is argued): a workgroup of 256 lanes owns a brick
// of 8 x 8 x 16 voxels, a lane a run of 4 voxels along z whose words live in registers across all views; per chunk of 256 views
// one lane per view tests the brick's ball, the survivors go to LDS in ascending order and every lane walks that list.  What a
// view does to a voxel -- the ball test, the projection, `updated` -- is tsdf_dev.h's, the same code the fusion runs, so a view
// is taken out of exactly the voxels it went into; only the step on the running words differs: a subtraction for the addition,
// w0 - 1 for w0 + 1, and the never-observed state, without a division, when the last view leaves (tsdf_remove_step, tsdf_dev.h: the
// sparse volume's removal, sparse_remove.hip, runs the same).
#include "block_dev.h"
#include "tsdf_dev.h"
#include "../../include/mipsf_deintegrate.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t BX = MIPSF_TSDF_BRICK_X, BY = MIPSF_TSDF_BRICK_Y, BZ = MIPSF_TSDF_BRICK_Z;
constexpr uint32_t RUN = 4;                       // voxels of a lane, along z
constexpr uint32_t CHUNK = MIPSF_TSDF_VIEW_CHUNK;
static_assert(BX * BY * (BZ / RUN) == TPB, "one lane per run of the brick");
static_assert(CHUNK == TPB, "one lane per view of a chunk");
static_assert(sizeof(mipsf_deintegrate_record) == 32, "deintegrate record");

// grid: one block per brick, bricks in (x, y, z) order with z fastest
template <bool COLOR>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) tsdf_remove_kernel(TsdfGrid vol, TsdfFrames s, mipsf_deintegrate_record* __restrict__ record) {
    __shared__ uint32_t list[CHUNK];
    __shared__ uint32_t wave_count[WAVES];
    __shared__ uint64_t sm[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t bz = blockIdx.x % vol.bricks_z, by = (blockIdx.x / vol.bricks_z) % vol.bricks_y, bx = blockIdx.x / (vol.bricks_z * vol.bricks_y);
    const uint32_t x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;                    // the brick; it holds at least one voxel
    const uint32_t x1 = min(x0 + BX, vol.X), y1 = min(y0 + BY, vol.Y), z1 = min(z0 + BZ, vol.Z);

    // the lane's run: voxels (i, j, k0 .. k0 + 3); a lane outside the volume reads the brick's first voxel and writes nothing
    const uint32_t i = x0 + (tid >> 5), j = y0 + ((tid >> 2) & 7u), k0 = z0 + (tid & 3u) * RUN;
    const bool row_ok = i < vol.X && j < vol.Y;
    const size_t base = ((size_t)(row_ok ? i : x0) * vol.Y + (row_ok ? j : y0)) * vol.Z;
    const double px = (double)(float)vol.ticks[0][row_ok ? i : x0], py = (double)(float)vol.ticks[1][row_ok ? j : y0];
    bool ok[RUN];
    double pz[RUN];
    float tsdf[RUN], weight[RUN], color[COLOR ? RUN * 3 : 1];
#pragma unroll
    for (uint32_t r = 0; r < RUN; ++r) {
        ok[r] = row_ok && k0 + r < vol.Z;
        const uint32_t k = ok[r] ? k0 + r : z0;
        pz[r] = (double)(float)vol.ticks[2][k];
        tsdf[r] = ok[r] ? vol.tsdf[base + k] : 0.0f;
        weight[r] = ok[r] ? vol.weight[base + k] : 0.0f;
        if (COLOR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) color[r * 3 + c] = ok[r] ? vol.color[(base + k) * 3 + c] : 0.0f;
        }
    }

    // the ball that holds the brick's voxels (every lane the same); a brick without one takes every view
    double c[3], radius;
    const bool ball = tsdf_brick_ball(vol, x0, x1, y0, y1, z0, z1, c, radius);
    const bool cull = !(s.flags & MIPSF_TSDF_NO_CULL) && ball;

    const size_t hw = (size_t)s.H * s.W;
    uint64_t removed = 0, missing = 0, emptied = 0;
    for (uint32_t first = 0; first < s.n; first += CHUNK) {
        // ---- which views of the chunk can reach the brick, in ascending order
        const uint32_t k = first + tid;
        const bool keep = k < s.n && (!cull || tsdf_view_can_update(s, k, c, radius));
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
            vol.tsdf[base + k0 + r] = tsdf[r];
            vol.weight[base + k0 + r] = weight[r];
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vol.color[(base + k0 + r) * 3 + ch] = color[r * 3 + ch];
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
        if (observed) atomicAdd((unsigned long long*)&record->observed, (unsigned long long)observed);
    }
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

static bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }

extern "C" int mipsf_deintegrate_views(const mipsf_deintegrate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_deintegrate_args, "mipsf_deintegrate_views");
    MIPSF_REQUIRE(a->X > 0 && a->Y > 0 && a->Z > 0, "mipsf_deintegrate_views: a volume of %u x %u x %u has no voxels", a->X, a->Y, a->Z);
    MIPSF_REQUIRE((uint64_t)a->X * a->Y * a->Z <= MIPSF_TSDF_MAX_VOXELS, "mipsf_deintegrate_views: %u x %u x %u voxels, at most 2^31 - 1", a->X, a->Y,
                  a->Z);
    const uint64_t bricks = (uint64_t)blocks_for(a->X, BX) * blocks_for(a->Y, BY) * blocks_for(a->Z, BZ);
    MIPSF_REQUIRE(bricks <= MIPSF_TSDF_MAX_BRICKS, "mipsf_deintegrate_views: %u x %u x %u voxels make %llu bricks, at most %u (a launch holds 2^32 lanes)",
                  a->X, a->Y, a->Z, (unsigned long long)bricks, MIPSF_TSDF_MAX_BRICKS);
    MIPSF_REQUIRE(a->n == 0 || (a->H > 0 && a->W > 0), "mipsf_deintegrate_views: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_TSDF_MAX_SIDE && a->W <= MIPSF_TSDF_MAX_SIDE, "mipsf_deintegrate_views: image %u x %u, at most %u a side", a->H, a->W,
                  MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_deintegrate_views: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(pos_finite(a->fx) && pos_finite(a->fy) && fabs(a->cx) < INFINITY && fabs(a->cy) < INFINITY,
                  "mipsf_deintegrate_views: intrinsics %g %g %g %g", a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_deintegrate_views: depth_max is not a number");
    MIPSF_REQUIRE((a->flags & ~MIPSF_TSDF_NO_CULL) == 0, "mipsf_deintegrate_views: flags %u", a->flags);
    MIPSF_REQUIRE(a->n == 0 || (a->rgb != nullptr) == (a->color != nullptr), "mipsf_deintegrate_views: rgb and color go together (rgb %s, color %s)",
                  a->rgb ? "given" : "null", a->color ? "given" : "null");
    MIPSF_REQUIRE(a->ticks[0] && a->ticks[1] && a->ticks[2] && a->tsdf && a->weight && a->record && (a->n == 0 || (a->depth && a->poses)),
                  "mipsf_deintegrate_views: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(a->record, 0, sizeof(mipsf_deintegrate_record), st) != hipSuccess) return check_launch("tsdf_remove (record)");
    if (a->n == 0) return check_launch("tsdf_remove");
    TsdfGrid vol;
    for (int d = 0; d < 3; ++d) vol.ticks[d] = a->ticks[d];
    vol.tsdf = a->tsdf, vol.weight = a->weight, vol.color = a->color;
    vol.X = a->X, vol.Y = a->Y, vol.Z = a->Z;
    vol.bricks_y = blocks_for(a->Y, BY), vol.bricks_z = blocks_for(a->Z, BZ);
    const TsdfFrames s = {a->depth, a->rgb, a->poses, a->n, a->H, a->W, a->flags, a->fx, a->fy, a->cx, a->cy, a->trunc, a->depth_max, INFINITY};
    if (a->color)
        hipLaunchKernelGGL(tsdf_remove_kernel<true>, dim3((uint32_t)bricks), dim3(TPB), 0, st, vol, s, a->record);
    else
        hipLaunchKernelGGL(tsdf_remove_kernel<false>, dim3((uint32_t)bricks), dim3(TPB), 0, st, vol, s, a->record);
    return check_launch("tsdf_remove");
}
