// The model side of a frame-to-model depth tracker over the TSDF volume (include/mipsf_track.h): depth, normal and colour images of
// the volume by ray casting, and a point-to-plane registration of a live depth frame against them by projective association.
// Upstream has no TSDF code; the rules are this project's own (KinectFusion's model side).  DESIGN.md 4.21.
//
// Shape of the kernels.  Ray cast: a workgroup of 256 lanes takes 16 x 16 pixels of one view, a wave 8 x 8 of them, a lane one ray,
// so the eight corner reads of neighbouring rays fall into the same cache lines and the brick marks are shared; a lane that has hit
// or left the box idles (its exec bit is off) until the longest ray of its wave is through.  The marks (one byte per brick of
// tsdf.hip's 8 x 8 x 16 voxels) come from one launch over the volume before it; a sample whose base voxel lies in an unmarked brick
// costs one byte read instead of sixteen words and a trilinear blend.  Registration: a lane per live pixel, the sums of icp.hip
// (icp_dev.h) per block and then by one wave, max_iteration + 1 evaluations behind a `done` word.  Only the arithmetic is float64;
// the words of the volume and the images are read as fp32.
#include "block_dev.h"
#include "icp_dev.h"
#include "tsdf_dev.h"
#include "../../include/mipsf_track_color.h"

namespace mipsf {
uint64_t track_color_workspace_bytes(uint32_t H, uint32_t W);         // track_color.hip

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / MIPSF_WAVE;
constexpr uint32_t BX = MIPSF_TSDF_BRICK_X, BY = MIPSF_TSDF_BRICK_Y, BZ = MIPSF_TSDF_BRICK_Z;
constexpr uint32_t TILE = MIPSF_TRACK_TILE;
static_assert(TILE * TILE == TPB && TILE == 16, "a lane per pixel of the tile, a wave per 8 x 8 quarter");
static_assert(sizeof(mipsf_track_record) == 16, "track record");
static_assert(MIPSF_TRACK_RESULT_DOUBLES == 20, "the result layout of mipsf_icp_register");

struct Field {
    const float* tsdf;
    const float* weight;
    const float* color;
    const uint8_t* marks;               // [bricks_x, bricks_y, bricks_z], null: no skipping
    uint32_t X, Y, Z;
    uint32_t bricks_y, bricks_z;
    double origin[3], voxel, min_weight;
};

// ------------------------------------------------------------------------------------------------ brick marks
// grid: one block per brick, bricks in (x, y, z) order with z fastest; the brick with an apron of one voxel, clipped
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) track_mark_kernel(Field v, uint8_t* __restrict__ marks, mipsf_track_record* __restrict__ record) {
    const uint32_t bz = blockIdx.x % v.bricks_z, by = (blockIdx.x / v.bricks_z) % v.bricks_y, bx = blockIdx.x / (v.bricks_z * v.bricks_y);
    const uint32_t x0 = bx * BX > 0 ? bx * BX - 1 : 0, y0 = by * BY > 0 ? by * BY - 1 : 0, z0 = bz * BZ > 0 ? bz * BZ - 1 : 0;
    const uint32_t x1 = min(bx * BX + BX + 1, v.X), y1 = min(by * BY + BY + 1, v.Y), z1 = min(bz * BZ + BZ + 1, v.Z);      // exclusive
    const uint32_t nx = x1 - x0, ny = y1 - y0, nz = z1 - z0;
    int any = 0;
    for (uint32_t e = threadIdx.x; e < nx * ny * nz; e += TPB) {
        const uint32_t k = z0 + e % nz, j = y0 + (e / nz) % ny, i = x0 + e / (nz * ny);
        const size_t idx = ((size_t)i * v.Y + j) * v.Z + k;
        any |= ((double)v.weight[idx] >= v.min_weight && v.tsdf[idx] <= 0.0f) ? 1 : 0;
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        marks[blockIdx.x] = any ? 1 : 0;
        if (any) atomicAdd((unsigned long long*)&record->marked, 1ull);
    }
}

// ------------------------------------------------------------------------------------------------ the field
struct Base {
    uint32_t i0[3];
    double fr[3];
    bool valid;                         // 0 <= i0[a] <= D_a - 2 on every axis
};

__device__ __forceinline__ Base base_of(const Field& v, double px, double py, double pz) {
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

// whether the sample can be left to `unknown or positive` without a look at the volume
__device__ __forceinline__ bool is_free(const Field& v, const Base& b) {
    if (!b.valid) return true;
    return v.marks[((size_t)(b.i0[0] / BX) * v.bricks_y + b.i0[1] / BY) * v.bricks_z + b.i0[2] / BZ] == 0;
}

// the trilinear field at a valid base; false: unknown
__device__ __forceinline__ bool field_at(const Field& v, const Base& b, double& f) {
    const size_t sx = (size_t)v.Y * v.Z, sy = v.Z;
    const size_t at = (size_t)b.i0[0] * sx + (size_t)b.i0[1] * sy + b.i0[2];         // corners at + {0, sx} + {0, sy} + {0, 1}: i0 + 1 <= D - 1
    bool known = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) known = known && (double)v.weight[at + (c & 4 ? sx : 0) + (c & 2 ? sy : 0) + (c & 1)] >= v.min_weight;
    if (!known) return false;
    double w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = (double)v.tsdf[at + (c & 4 ? sx : 0) + (c & 2 ? sy : 0) + (c & 1)];
    const double fz = b.fr[2], fy = b.fr[1], fx = b.fr[0];
    const double c00 = w[0] * (1.0 - fz) + w[1] * fz, c01 = w[2] * (1.0 - fz) + w[3] * fz;
    const double c10 = w[4] * (1.0 - fz) + w[5] * fz, c11 = w[6] * (1.0 - fz) + w[7] * fz;
    const double c0 = c00 * (1.0 - fy) + c01 * fy, c1 = c10 * (1.0 - fy) + c11 * fy;
    f = c0 * (1.0 - fx) + c1 * fx;
    return true;
}

__device__ __forceinline__ bool field_of(const Field& v, double px, double py, double pz, double& f) {
    const Base b = base_of(v, px, py, pz);
    return b.valid && field_at(v, b, f);
}

// whether sample i of the ray exists and is not free; only the skipping asks
__device__ __forceinline__ bool busy(const Field& v, double tx, double ty, double tz, double dx, double dy, double dz, double t_in, double dt, double t_out,
                                     uint32_t i) {
    const double ti = t_in + (double)i * dt;
    if (!(i < MIPSF_TRACK_MAX_SAMPLES && ti <= t_out)) return false;
    return !is_free(v, base_of(v, tx + dx * ti, ty + dy * ti, tz + dz * ti));
}

struct Camera {
    const float* poses;
    uint32_t H, W;
    double fx, fy, cx, cy, near, far, step;
};

// grid: (tiles of a view, n)
template <bool SKIP>
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) track_raycast_kernel(Field v, Camera s, float* __restrict__ depth, float* __restrict__ normals,
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
            bool cur_busy = SKIP ? busy(v, t[0], t[1], t[2], d[0], d[1], d[2], t_in, dt, t_out, 0u) : true;
            for (uint32_t i = 0; i < MIPSF_TRACK_MAX_SAMPLES; ++i) {
                const double ti = t_in + (double)i * dt;
                if (!(ti <= t_out)) break;
                const bool nxt_busy = SKIP ? busy(v, t[0], t[1], t[2], d[0], d[1], d[2], t_in, dt, t_out, i + 1u) : true;
                double f = 0.0;
                bool known = false;
                if (cur_busy || nxt_busy) {
                    const Base b = base_of(v, t[0] + d[0] * ti, t[1] + d[1] * ti, t[2] + d[2] * ti);
                    known = b.valid && field_at(v, b, f);
                }
                if (prev_known && known) {
                    if (prev > 0.0 && f <= 0.0) {
                        tstar = (t_in + (double)(i - 1u) * dt) + dt * (prev / (prev - f));      // t_{i-1}, not a running sum
                        hit = true;
                        break;
                    }
                    if (prev < 0.0 && f > 0.0) break;
                }
                prev_known = known, prev = f;
                cur_busy = nxt_busy;
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
                        const bool kp = field_of(v, a == 0 ? ps[0] + v.voxel : ps[0], a == 1 ? ps[1] + v.voxel : ps[1], a == 2 ? ps[2] + v.voxel : ps[2], fp);
                        const bool km = field_of(v, a == 0 ? ps[0] - v.voxel : ps[0], a == 1 ? ps[1] - v.voxel : ps[1], a == 2 ? ps[2] - v.voxel : ps[2], fm);
                        all = all && kp && km;
                        grad[a] = fp - fm;
                    }
                    const double L = sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
                    if (all && L > 0.0 && L < INFINITY) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) out_n[a] = (float)(grad[a] / L);
                    }
                }
                if (color_out)
                    tsdf_sample_color((ps[0] - v.origin[0]) / v.voxel, (ps[1] - v.origin[1]) / v.voxel, (ps[2] - v.origin[2]) / v.voxel, v.X, v.Y, v.Z,
                                      v.weight, v.color, out_c);
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

// ------------------------------------------------------------------------------------------------ registration
struct Reg {
    const float* model_depth;
    const float* model_normals;
    const float* pose_ref;
    const float* live;
    uint32_t H, W;
    double fx, fy, cx, cy, depth_max, maxd2;
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) track_init_kernel(const float* __restrict__ pose_init, IcpState* st,
                                                                                  double* __restrict__ result) {
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 16; ++j) st->T[j] = (double)pose_init[j];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) st->U[4 * r + c] = r == c ? 1.0 : 0.0;
    st->prev_fitness = st->prev_rmse = 0.0;
    st->done = 0u, st->iter = 0u;
    for (int j = 0; j < (int)MIPSF_TRACK_RESULT_DOUBLES; ++j) result[j] = 0.0;
}

// One evaluation: a lane per live pixel, the block's sums in partial[block][NSUM_PAD]; column NSUM counts the usable pixels.
MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) track_pair_kernel(Reg g, const IcpState* st, double* __restrict__ partial,
                                                                           int32_t* __restrict__ partner) {
    if (st->done) return;
    __shared__ double sm[WAVES][NSUM_PAD];
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    double c[NSUM + 1];
#pragma unroll
    for (int k = 0; k < NSUM + 1; ++k) c[k] = 0.0;
    if (i < g.H * g.W) {
        const uint32_t row = i / g.W, col = i % g.W;
        const double d = (double)g.live[i];
        int32_t mate = -1;
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
                    }
                }
            }
        }
        if (partner) partner[i] = mate;
    }
    icp_block_sums<WAVES, NSUM + 1>(c, sm, partial);
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(MIPSF_WAVE) track_finish_kernel(const double* __restrict__ partial, uint32_t nb, IcpState* st,
                                                                                    uint32_t max_iteration, double rel_fitness, double rel_rmse,
                                                                                    double* __restrict__ result, float* __restrict__ pose_out) {
    if (st->done) return;
    icp_finish<NSUM + 1>(partial, nb, 0u, st, max_iteration, rel_fitness, rel_rmse, result);
    if (threadIdx.x == 0)
        for (int j = 0; j < 16; ++j) pose_out[j] = (float)result[j];
}

bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }
bool is_finite(double v) { return fabs(v) < INFINITY; }

uint64_t brick_count(uint32_t X, uint32_t Y, uint32_t Z) { return (uint64_t)blocks_for(X, BX) * blocks_for(Y, BY) * blocks_for(Z, BZ); }

constexpr uint64_t REG_STATE_BYTES = 256;

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_track_workspace_bytes(int which, uint32_t a, uint32_t b, uint32_t c) {
    switch (which) {
        case MIPSF_TRACK_WS_RAYCAST:
            if (a == 0 || b == 0 || c == 0 || (uint64_t)a * b * c > MIPSF_TSDF_MAX_VOXELS || brick_count(a, b, c) > MIPSF_TSDF_MAX_BRICKS) return 0;
            return align16(brick_count(a, b, c));
        case MIPSF_TRACK_WS_REGISTER:
            if (a == 0 || b == 0 || a > MIPSF_TSDF_MAX_SIDE || b > MIPSF_TSDF_MAX_SIDE) return 0;
            return REG_STATE_BYTES + (uint64_t)blocks_for((uint64_t)a * b, TPB) * NSUM_PAD * sizeof(double);
        case MIPSF_TRACK_WS_REGISTER_COLOR:
            return track_color_workspace_bytes(a, b);
        default:
            return 0;
    }
}

extern "C" int mipsf_track_raycast(const mipsf_track_raycast_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_track_raycast_args, "mipsf_track_raycast");
    MIPSF_REQUIRE(a->X > 0 && a->Y > 0 && a->Z > 0, "mipsf_track_raycast: a volume of %u x %u x %u has no voxels", a->X, a->Y, a->Z);
    MIPSF_REQUIRE((uint64_t)a->X * a->Y * a->Z <= MIPSF_TSDF_MAX_VOXELS, "mipsf_track_raycast: %u x %u x %u voxels, at most 2^31 - 1", a->X, a->Y, a->Z);
    const uint64_t bricks = brick_count(a->X, a->Y, a->Z);
    MIPSF_REQUIRE(bricks <= MIPSF_TSDF_MAX_BRICKS, "mipsf_track_raycast: %u x %u x %u voxels make %llu bricks, at most %u", a->X, a->Y, a->Z,
                  (unsigned long long)bricks, MIPSF_TSDF_MAX_BRICKS);
    MIPSF_REQUIRE(a->n == 0 || (a->H > 0 && a->W > 0), "mipsf_track_raycast: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_TSDF_MAX_SIDE && a->W <= MIPSF_TSDF_MAX_SIDE, "mipsf_track_raycast: image %u x %u, at most %u a side", a->H, a->W,
                  MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(a->n <= MIPSF_TRACK_MAX_VIEWS, "mipsf_track_raycast: %u views, at most %u a call", a->n, MIPSF_TRACK_MAX_VIEWS);
    MIPSF_REQUIRE(pos_finite(a->voxel), "mipsf_track_raycast: voxel %g is not positive and finite", a->voxel);
    MIPSF_REQUIRE(pos_finite(a->trunc), "mipsf_track_raycast: trunc %g is not positive and finite", a->trunc);
    MIPSF_REQUIRE(pos_finite(a->step), "mipsf_track_raycast: step %g is not positive and finite", a->step);
    MIPSF_REQUIRE(pos_finite(a->fx) && pos_finite(a->fy) && is_finite(a->cx) && is_finite(a->cy), "mipsf_track_raycast: intrinsics %g %g %g %g", a->fx, a->fy,
                  a->cx, a->cy);
    MIPSF_REQUIRE(is_finite(a->origin[0]) && is_finite(a->origin[1]) && is_finite(a->origin[2]), "mipsf_track_raycast: origin %g %g %g", a->origin[0],
                  a->origin[1], a->origin[2]);
    MIPSF_REQUIRE(a->near == a->near && a->far == a->far, "mipsf_track_raycast: near or far is not a number");
    MIPSF_REQUIRE(a->min_weight == a->min_weight, "mipsf_track_raycast: min_weight is not a number");
    const double ex = (double)a->X - 1.0, ey = (double)a->Y - 1.0, ez = (double)a->Z - 1.0;
    const double most = a->voxel * sqrt(ex * ex + ey * ey + ez * ez) / a->step + 2.0;
    MIPSF_REQUIRE(most <= (double)MIPSF_TRACK_MAX_SAMPLES, "mipsf_track_raycast: step %g gives up to %g samples a ray, at most %u", a->step, most,
                  MIPSF_TRACK_MAX_SAMPLES);
    MIPSF_REQUIRE((a->flags & ~MIPSF_TRACK_NO_SKIP) == 0, "mipsf_track_raycast: flags %u", a->flags);
    MIPSF_REQUIRE(!(a->color_out && !a->color), "mipsf_track_raycast: color_out needs a volume with color");
    MIPSF_REQUIRE(a->tsdf && a->weight && a->record && a->workspace && (a->n == 0 || (a->poses && a->depth)), "mipsf_track_raycast: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_track_raycast: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(a->record, 0, sizeof(mipsf_track_record), st) != hipSuccess) return check_launch("track_raycast (record)");
    if (a->n == 0) return check_launch("track_raycast");
    const bool skip = !(a->flags & MIPSF_TRACK_NO_SKIP);
    Field v;
    v.tsdf = a->tsdf, v.weight = a->weight, v.color = a->color, v.marks = skip ? (const uint8_t*)a->workspace : nullptr;
    v.X = a->X, v.Y = a->Y, v.Z = a->Z;
    v.bricks_y = blocks_for(a->Y, BY), v.bricks_z = blocks_for(a->Z, BZ);
    for (int d = 0; d < 3; ++d) v.origin[d] = a->origin[d];
    v.voxel = a->voxel, v.min_weight = a->min_weight;
    const Camera s = {a->poses, a->H, a->W, a->fx, a->fy, a->cx, a->cy, a->near, a->far, a->step};
    const dim3 grid(blocks_for(a->W, TILE) * blocks_for(a->H, TILE), a->n);
    if (skip) {
        hipLaunchKernelGGL(track_mark_kernel, dim3((uint32_t)bricks), dim3(TPB), 0, st, v, (uint8_t*)a->workspace, a->record);
        hipLaunchKernelGGL(track_raycast_kernel<true>, grid, dim3(TPB), 0, st, v, s, a->depth, a->normals, a->color_out, a->record);
    } else {
        hipLaunchKernelGGL(track_raycast_kernel<false>, grid, dim3(TPB), 0, st, v, s, a->depth, a->normals, a->color_out, a->record);
    }
    return check_launch("track_raycast");
}

extern "C" int mipsf_track_register(const mipsf_track_register_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_track_register_args, "mipsf_track_register");
    MIPSF_REQUIRE(a->H > 0 && a->W > 0, "mipsf_track_register: an image of %u x %u has no pixels", a->H, a->W);
    MIPSF_REQUIRE(a->H <= MIPSF_TSDF_MAX_SIDE && a->W <= MIPSF_TSDF_MAX_SIDE, "mipsf_track_register: image %u x %u, at most %u a side", a->H, a->W,
                  MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(pos_finite(a->fx) && pos_finite(a->fy) && is_finite(a->cx) && is_finite(a->cy), "mipsf_track_register: intrinsics %g %g %g %g", a->fx, a->fy,
                  a->cx, a->cy);
    MIPSF_REQUIRE(a->depth_max == a->depth_max, "mipsf_track_register: depth_max is not a number");
    MIPSF_REQUIRE(a->max_dist >= 0.0 && a->max_dist < INFINITY, "mipsf_track_register: max_dist %g", a->max_dist);
    MIPSF_REQUIRE(a->max_iteration <= MIPSF_TRACK_MAX_ITERATION, "mipsf_track_register: max_iteration %u above %u", a->max_iteration,
                  MIPSF_TRACK_MAX_ITERATION);
    MIPSF_REQUIRE(a->model_depth && a->model_normals && a->pose_ref && a->live && a->pose_init && a->result && a->pose_out && a->workspace,
                  "mipsf_track_register: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_track_register: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    IcpState* st = (IcpState*)a->workspace;
    double* partial = (double*)((char*)a->workspace + REG_STATE_BYTES);
    const uint32_t nb = blocks_for((uint64_t)a->H * a->W, TPB);
    const Reg g = {a->model_depth, a->model_normals, a->pose_ref, a->live, a->H, a->W, a->fx, a->fy, a->cx, a->cy, a->depth_max, a->max_dist * a->max_dist};
    hipLaunchKernelGGL(track_init_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, a->pose_init, st, a->result);
    for (uint32_t k = 0; k <= a->max_iteration; ++k) {
        hipLaunchKernelGGL(track_pair_kernel, dim3(nb), dim3(TPB), 0, s, g, (const IcpState*)st, partial, a->partner);
        hipLaunchKernelGGL(track_finish_kernel, dim3(1), dim3(MIPSF_WAVE), 0, s, (const double*)partial, nb, st, a->max_iteration,
                           a->relative_fitness, a->relative_rmse, a->result, a->pose_out);
    }
    return check_launch("track_register");
}
