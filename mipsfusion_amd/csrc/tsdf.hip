// Depth frames fused into a dense TSDF volume, and the colour of marched vertices (include/mipsf_tsdf.h).  Upstream has no TSDF
// code (the papers that followed it fuse rendered depth with a host library); the rule is this project's own.  DESIGN.md 4.19.
//
// Shape of the kernel: a workgroup of 256 lanes owns a brick of 8 x 8 x 16 voxels, a lane a run of 4 voxels along z (the fastest
// axis: 16 contiguous bytes of tsdf and of weight per lane, 64 per row of the brick).  The lane's tsdf, weight and colour words
// are loaded once, live in registers across all views and are stored once: no atomics on the state.  The views come in chunks of
// 256: one lane per view tests the brick's bounding sphere against the view, the survivors' indices go to LDS in ascending order
// (the update is order-dependent by definition), and every lane walks that list; the pose of a view is read through a
// wave-uniform index.  The sphere test is the only arithmetic here that the header does not fix: it may be generous, it must
// never leave out a pair the rule updates.  The projection is stated a second time, next to raster.hip's: in tsdf_dev.h, with the
// sphere test, where tsdf_remove.hip takes the same views out of the same voxels again.
#include "block_dev.h"
#include "tsdf_dev.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t BX = MIPSF_TSDF_BRICK_X, BY = MIPSF_TSDF_BRICK_Y, BZ = MIPSF_TSDF_BRICK_Z;
constexpr uint32_t RUN = 4;                       // voxels of a lane, along z
constexpr uint32_t CHUNK = MIPSF_TSDF_VIEW_CHUNK;
static_assert(BX * BY * (BZ / RUN) == TPB, "one lane per run of the brick");
static_assert(CHUNK == TPB, "one lane per view of a chunk");
static_assert(sizeof(mipsf_tsdf_record) == 16, "tsdf record");

using Frames = TsdfFrames;                        // tsdf_dev.h: the views, the volume, the ball test and the projection, shared with
using Volume = TsdfGrid;                          // tsdf_remove.hip

// grid: one block per brick, bricks in (x, y, z) order with z fastest
template <bool COLOR>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) tsdf_integrate_kernel(Volume vol, Frames s, mipsf_tsdf_record* __restrict__ record) {
    __shared__ uint32_t list[CHUNK];
    __shared__ uint32_t wave_count[WAVES];
    __shared__ uint64_t sm[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t bz = blockIdx.x % vol.bricks_z, by = (blockIdx.x / vol.bricks_z) % vol.bricks_y, bx = blockIdx.x / (vol.bricks_z * vol.bricks_y);
    const uint32_t x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;                    // the brick; it holds at least one voxel
    const uint32_t x1 = min(x0 + BX, vol.X), y1 = min(y0 + BY, vol.Y), z1 = min(z0 + BZ, vol.Z);

    // the lane's run: voxels (i, j, k0 .. k0 + 3)
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
    uint64_t updates = 0;
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
            vol.tsdf[base + k0 + r] = tsdf[r];
            vol.weight[base + k0 + r] = weight[r];
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) vol.color[(base + k0 + r) * 3 + ch] = color[r * 3 + ch];
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

// ------------------------------------------------------------------------------------------------ colour of marched vertices
// the rule itself: tsdf_dev.h (tsdf_track.hip colours its hits with it)
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) tsdf_sample_kernel(const double* __restrict__ points, uint32_t m, uint32_t X, uint32_t Y,
                                                                            uint32_t Z, const float* __restrict__ weight,
                                                                            const float* __restrict__ color, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * TPB + threadIdx.x;
    if (p >= m) return;
    const double x = points[(size_t)p * 3], y = points[(size_t)p * 3 + 1], z = points[(size_t)p * 3 + 2];
    float res[3];
    tsdf_sample_color(x, y, z, X, Y, Z, weight, color, res);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[(size_t)p * 3 + ch] = res[ch];
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

static bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }

extern "C" int mipsf_tsdf_integrate(const mipsf_tsdf_integrate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_tsdf_integrate_args, "mipsf_tsdf_integrate");
    MIPSF_REQUIRE(a->X > 0 && a->Y > 0 && a->Z > 0, "mipsf_tsdf_integrate: a volume of %u x %u x %u has no voxels", a->X, a->Y, a->Z);
    MIPSF_REQUIRE((uint64_t)a->X * a->Y * a->Z <= MIPSF_TSDF_MAX_VOXELS, "mipsf_tsdf_integrate: %u x %u x %u voxels, at most 2^31 - 1", a->X, a->Y,
                  a->Z);
    const uint64_t bricks = (uint64_t)blocks_for(a->X, BX) * blocks_for(a->Y, BY) * blocks_for(a->Z, BZ);
    MIPSF_REQUIRE(bricks <= MIPSF_TSDF_MAX_BRICKS, "mipsf_tsdf_integrate: %u x %u x %u voxels make %llu bricks, at most %u (a launch holds 2^32 lanes)",
                  a->X, a->Y, a->Z, (unsigned long long)bricks, MIPSF_TSDF_MAX_BRICKS);
    MIPSF_REQUIRE(a->n == 0 || (a->H > 0 && a->W > 0), "mipsf_tsdf_integrate: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_TSDF_MAX_SIDE && a->W <= MIPSF_TSDF_MAX_SIDE, "mipsf_tsdf_integrate: image %u x %u, at most %u a side", a->H, a->W,
                  MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_tsdf_integrate: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(pos_finite(a->fx) && pos_finite(a->fy) && fabs(a->cx) < INFINITY && fabs(a->cy) < INFINITY,
                  "mipsf_tsdf_integrate: intrinsics %g %g %g %g", a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_tsdf_integrate: depth_max is not a number");
    MIPSF_REQUIRE(a->max_weight >= 1.0, "mipsf_tsdf_integrate: max_weight %g, at least 1", a->max_weight);
    MIPSF_REQUIRE((a->flags & ~MIPSF_TSDF_NO_CULL) == 0, "mipsf_tsdf_integrate: flags %u", a->flags);
    MIPSF_REQUIRE(a->n == 0 || (a->rgb != nullptr) == (a->color != nullptr), "mipsf_tsdf_integrate: rgb and color go together (rgb %s, color %s)",
                  a->rgb ? "given" : "null", a->color ? "given" : "null");
    MIPSF_REQUIRE(a->ticks[0] && a->ticks[1] && a->ticks[2] && a->tsdf && a->weight && a->record && (a->n == 0 || (a->depth && a->poses)),
                  "mipsf_tsdf_integrate: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(a->record, 0, sizeof(mipsf_tsdf_record), st) != hipSuccess) return check_launch("tsdf_integrate (record)");
    if (a->n == 0) return check_launch("tsdf_integrate");
    Volume vol;
    for (int d = 0; d < 3; ++d) vol.ticks[d] = a->ticks[d];
    vol.tsdf = a->tsdf, vol.weight = a->weight, vol.color = a->color;
    vol.X = a->X, vol.Y = a->Y, vol.Z = a->Z;
    vol.bricks_y = blocks_for(a->Y, BY), vol.bricks_z = blocks_for(a->Z, BZ);
    const Frames s = {a->depth, a->rgb, a->poses, a->n, a->H, a->W, a->flags, a->fx, a->fy, a->cx, a->cy, a->trunc, a->depth_max, a->max_weight};
    if (a->color)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3((uint32_t)bricks), dim3(TPB), 0, st, vol, s, a->record);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3((uint32_t)bricks), dim3(TPB), 0, st, vol, s, a->record);
    return check_launch("tsdf_integrate");
}

extern "C" int mipsf_tsdf_sample(const mipsf_tsdf_sample_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_tsdf_sample_args, "mipsf_tsdf_sample");
    MIPSF_REQUIRE(a->X > 0 && a->Y > 0 && a->Z > 0, "mipsf_tsdf_sample: a volume of %u x %u x %u has no voxels", a->X, a->Y, a->Z);
    MIPSF_REQUIRE((uint64_t)a->X * a->Y * a->Z <= MIPSF_TSDF_MAX_VOXELS, "mipsf_tsdf_sample: %u x %u x %u voxels, at most 2^31 - 1", a->X, a->Y, a->Z);
    if (a->m == 0) return 0;
    MIPSF_REQUIRE(a->points && a->weight && a->color && a->out, "mipsf_tsdf_sample: null pointer");
    hipLaunchKernelGGL(tsdf_sample_kernel, dim3(blocks_for(a->m, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->points, a->m, a->X, a->Y, a->Z, a->weight,
                       a->color, a->out);
    return check_launch("tsdf_sample");
}
