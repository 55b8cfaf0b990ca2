// mipsf_track_register with a photometric term (include/mipsf_track_color.h): the geometric pair of tsdf_track.hip,
// word for word, and for a pair whose projection falls into a 2 x 2 patch of model pixels with a depth, a second row -- the
// bilinear intensity of the model's colour image against the live pixel's, with the patch's own derivatives for a gradient.  A
// lane per live pixel carries both Jacobians and all 32 columns of the sums in float64 registers; the sums, the finish step and
// the `done` word are icp_dev.h's.  Upstream has no TSDF code; the rule is this project's own.
#include "icp_dev.h"
#include "../../include/mipsf_track_color.h"

namespace mipsf {
namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint64_t REG_STATE_BYTES = 256;
static_assert(MIPSF_TRACK_COLOR_RESULT_DOUBLES == MIPSF_TRACK_RESULT_DOUBLES + 2, "the result of mipsf_track_register, rows, colour rmse");
static_assert(NSUM_PAD == 32 && NSUM == 29, "columns 30 and 31 are the photometric ones");
static_assert(sizeof(IcpState) <= REG_STATE_BYTES, "IcpState");

struct RegColor {
    const float* model_depth;
    const float* model_normals;
    const float* model_color;
    const float* pose_ref;
    const float* live;
    const float* live_color;
    uint32_t H, W;
    double fx, fy, cx, cy, depth_max, maxd2, color_weight, max_color_diff;
};

__device__ __forceinline__ double intensity(const float* __restrict__ image, size_t pixel) {
    return (((double)image[pixel * 3] + (double)image[pixel * 3 + 1]) + (double)image[pixel * 3 + 2]) / 3.0;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) track_color_init_kernel(const float* __restrict__ pose_init, IcpState* st,
                                                                                        double* __restrict__ result) {
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 16; ++j) st->T[j] = (double)pose_init[j];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) st->U[4 * r + c] = r == c ? 1.0 : 0.0;
    st->prev_fitness = st->prev_rmse = st->prev_color_rmse = 0.0;
    st->done = 0u, st->iter = 0u;
    for (int j = 0; j < (int)MIPSF_TRACK_COLOR_RESULT_DOUBLES; ++j) result[j] = 0.0;
}

// One evaluation: a lane per live pixel, the block's sums in partial[block][NSUM_PAD].  Up to `mate` this is track_pair_kernel.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) track_color_pair_kernel(RegColor g, const IcpState* st, double* __restrict__ partial,
                                                                                 int32_t* __restrict__ partner, int32_t* __restrict__ color_partner) {
    if (st->done) return;
    __shared__ double sm[WAVES][NSUM_PAD];
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    double c[NSUM_PAD];
#pragma unroll
    for (int k = 0; k < NSUM_PAD; ++k) c[k] = 0.0;
    if (i < g.H * g.W) {
        const uint32_t row = i / g.W, col = i % g.W;
        const double d = (double)g.live[i];
        int32_t mate = -1, row_given = 0;
        if (d > 0.0 && d < INFINITY && d <= g.depth_max) {
            c[NSUM] = 1.0;
            const double* T = st->T;
            const float* Q = g.pose_ref;
            const double cx_ = d * (((double)col - g.cx) / g.fx), cy_ = -(d * (((double)row - g.cy) / g.fy)), cz_ = -d;
            double p[3], q[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                p[r] = ((T[4 * r] * cx_ + T[4 * r + 1] * cy_) + T[4 * r + 2] * cz_) + T[4 * r + 3];
                q[r] = p[r] - (double)Q[4 * r + 3];
            }
            double cam[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) cam[a] = ((double)Q[a] * q[0] + (double)Q[4 + a] * q[1]) + (double)Q[8 + a] * q[2];
            const double z = -cam[2];
            const double u = g.cx + g.fx * (cam[0] / z), vv = g.cy - g.fy * (cam[1] / z);
            const double col2 = floor(u + 0.5), row2 = floor(vv + 0.5);
            if (z > 0.0 && col2 >= 0.0 && col2 < (double)g.W && row2 >= 0.0 && row2 < (double)g.H) {
                const uint32_t pixel = (uint32_t)row2 * g.W + (uint32_t)col2;
                const double dm = (double)g.model_depth[pixel];
                const double nx = (double)g.model_normals[(size_t)pixel * 3], ny = (double)g.model_normals[(size_t)pixel * 3 + 1],
                             nz = (double)g.model_normals[(size_t)pixel * 3 + 2];
                if (dm > 0.0 && dm < INFINITY && (nx * nx + ny * ny) + nz * nz > 0.0) {
                    const double mx = dm * ((col2 - g.cx) / g.fx), my = -(dm * ((row2 - g.cy) / g.fy)), mz = -dm;
                    double e[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        e[r] = p[r] - ((((double)Q[4 * r] * mx + (double)Q[4 * r + 1] * my) + (double)Q[4 * r + 2] * mz) + (double)Q[4 * r + 3]);
                    const double d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                    if (d2 <= g.maxd2) {
                        mate = (int32_t)pixel;
                        const double r = (e[0] * nx + e[1] * ny) + e[2] * nz;
                        icp_pair_sums(c, p[0], p[1], p[2], nx, ny, nz, r, d2);
                        // the photometric row: the patch (r0, c0) .. (r0 + 1, c0 + 1) lies in the image and has a depth everywhere
                        const double c0 = floor(u), r0 = floor(vv);
                        if (c0 >= 0.0 && c0 + 1.0 < (double)g.W && r0 >= 0.0 && r0 + 1.0 < (double)g.H) {
                            const size_t p00 = (size_t)(uint32_t)r0 * g.W + (uint32_t)c0, p10 = p00 + g.W;
                            const double d00 = (double)g.model_depth[p00], d01 = (double)g.model_depth[p00 + 1], d10 = (double)g.model_depth[p10],
                                         d11 = (double)g.model_depth[p10 + 1];
                            if (d00 > 0.0 && d00 < INFINITY && d01 > 0.0 && d01 < INFINITY && d10 > 0.0 && d10 < INFINITY && d11 > 0.0 && d11 < INFINITY) {
                                const double I00 = intensity(g.model_color, p00), I01 = intensity(g.model_color, p00 + 1),
                                             I10 = intensity(g.model_color, p10), I11 = intensity(g.model_color, p10 + 1);
                                const double Il = intensity(g.live_color, i);
                                const double fu = u - c0, fv = vv - r0;
                                const double Im = (I00 * (1.0 - fu) + I01 * fu) * (1.0 - fv) + (I10 * (1.0 - fu) + I11 * fu) * fv;
                                const double Iu = (I01 - I00) * (1.0 - fv) + (I11 - I10) * fv;
                                const double Iv = (I10 - I00) * (1.0 - fu) + (I11 - I01) * fu;
                                const double rI = Im - Il;
                                if (fabs(rI) <= g.max_color_diff && fabs(rI) < INFINITY) {
                                    row_given = 1;
                                    const double zz = z * z;
                                    const double gx = Iu * (g.fx / z), gy = -(Iv * (g.fy / z));
                                    const double gz = Iu * (g.fx * (cam[0] / zz)) - Iv * (g.fy * (cam[1] / zz));
                                    double w[3];
#pragma unroll
                                    for (int a = 0; a < 3; ++a) w[a] = ((double)Q[4 * a] * gx + (double)Q[4 * a + 1] * gy) + (double)Q[4 * a + 2] * gz;
                                    const double Jc[6] = {p[1] * w[2] - p[2] * w[1], p[2] * w[0] - p[0] * w[2], p[0] * w[1] - p[1] * w[0], w[0], w[1], w[2]};
                                    int k = 0;
#pragma unroll
                                    for (int a = 0; a < 6; ++a)
#pragma unroll
                                        for (int bb = a; bb < 6; ++bb, ++k) c[k] = c[k] + g.color_weight * (Jc[a] * Jc[bb]);
#pragma unroll
                                    for (int a = 0; a < 6; ++a) c[21 + a] = c[21 + a] + g.color_weight * (Jc[a] * rI);
                                    c[30] = 1.0;
                                    c[31] = rI * rI;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (partner) partner[i] = mate;
        if (color_partner) color_partner[i] = row_given;
    }
    icp_block_sums<WAVES, NSUM_PAD>(c, sm, partial);
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) track_color_finish_kernel(const double* __restrict__ partial, uint32_t nb, IcpState* st,
                                                                                          uint32_t max_iteration, double rel_fitness, double rel_rmse,
                                                                                          double rel_color, double* __restrict__ result,
                                                                                          float* __restrict__ pose_out) {
    if (st->done) return;
    icp_finish<NSUM_PAD>(partial, nb, 0u, st, max_iteration, rel_fitness, rel_rmse, result, rel_color);
    if (threadIdx.x == 0)
        for (int j = 0; j < 16; ++j) pose_out[j] = (float)result[j];
}

bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }
bool is_finite(double v) { return fabs(v) < INFINITY; }

}  // namespace

// mipsf_track_workspace_bytes(MIPSF_TRACK_WS_REGISTER_COLOR, H, W, 0) (tsdf_track.hip holds the switch)
uint64_t track_color_workspace_bytes(uint32_t H, uint32_t W) {
    if (H == 0 || W == 0 || H > MIPSF_TSDF_MAX_SIDE || W > MIPSF_TSDF_MAX_SIDE) return 0;
    return REG_STATE_BYTES + (uint64_t)blocks_for((uint64_t)H * W, TPB) * NSUM_PAD * sizeof(double);
}

}  // namespace mipsf

using namespace mipsf;

extern "C" int mipsf_track_register_color(const mipsf_track_register_color_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_track_register_color_args, "mipsf_track_register_color");
    MIPSF_REQUIRE(a->H > 0 && a->W > 0, "mipsf_track_register_color: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_TSDF_MAX_SIDE && a->W <= MIPSF_TSDF_MAX_SIDE, "mipsf_track_register_color: image %u x %u, at most %u a side", a->H,
                  a->W, MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(pos_finite(a->fx) && pos_finite(a->fy) && is_finite(a->cx) && is_finite(a->cy), "mipsf_track_register_color: intrinsics %g %g %g %g",
                  a->fx, a->fy, a->cx, a->cy);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_track_register_color: depth_max is not a number");
    MIPSF_REQUIRE(a->max_dist >= 0.0 && a->max_dist < INFINITY, "mipsf_track_register_color: max_dist %g", a->max_dist);
    MIPSF_REQUIRE(a->max_iteration <= MIPSF_TRACK_MAX_ITERATION, "mipsf_track_register_color: max_iteration %u above %u", a->max_iteration,
                  MIPSF_TRACK_MAX_ITERATION);
    MIPSF_REQUIRE(a->color_weight >= 0.0 && a->color_weight < INFINITY, "mipsf_track_register_color: color_weight %g", a->color_weight);
    MIPSF_REQUIRE(a->max_color_diff >= 0.0, "mipsf_track_register_color: max_color_diff %g", a->max_color_diff);
    MIPSF_REQUIRE(a->relative_color_rmse == a->relative_color_rmse, "mipsf_track_register_color: relative_color_rmse is not a number");
    MIPSF_REQUIRE(a->model_color && a->live_color, "mipsf_track_register_color: null colour pointer (model_color, live_color)");
    MIPSF_REQUIRE(a->model_depth && a->model_normals && a->pose_ref && a->live && a->pose_init && a->result && a->pose_out && a->workspace,
                  "mipsf_track_register_color: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_track_register_color: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    IcpState* st = (IcpState*)a->workspace;
    double* partial = (double*)((char*)a->workspace + REG_STATE_BYTES);
    const uint32_t nb = blocks_for((uint64_t)a->H * a->W, TPB);
    const RegColor g = {a->model_depth, a->model_normals, a->model_color, a->pose_ref, a->live, a->live_color, a->H, a->W, a->fx, a->fy, a->cx, a->cy,
                        a->depth_max, a->max_dist * a->max_dist, a->color_weight, a->max_color_diff};
    hipLaunchKernelGGL(track_color_init_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, a->pose_init, st, a->result);
    for (uint32_t k = 0; k <= a->max_iteration; ++k) {
        hipLaunchKernelGGL(track_color_pair_kernel, dim3(nb), dim3(TPB), 0, s, g, (const IcpState*)st, partial, a->partner, a->color_partner);
        hipLaunchKernelGGL(track_color_finish_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, (const double*)partial, nb, st, a->max_iteration,
                           a->relative_fitness, a->relative_rmse, a->relative_color_rmse, a->result, a->pose_out);
    }
    return check_launch("track_register_color");
}
