// The colour of a point of the fused volume (the rule of mipsf_tsdf_sample, include/mipsf_tsdf.h), stated once for tsdf.hip, which
// colours marched vertices with it, and tsdf_track.hip, which colours the hits of a ray cast; and what a view does to a voxel of the
// dense volume -- the views and the volume by value, the brick's ball and its test against a view, the projection and `updated` of
// mipsf_tsdf_integrate -- stated once for tsdf.hip, which adds the view to the running mean, and tsdf_remove.hip, which takes it out
// again (include/mipsf_deintegrate.h); and the step that takes it out, stated once for tsdf_remove.hip and sparse_remove.hip, which
// takes views out of the brick-sparse volume (include/mipsf_sparse_remove.h).  Device code only.
#pragma once
#include "common.h"
#include "../../include/mipsf_tsdf.h"

namespace mipsf {

// ------------------------------------------------------------------------------------------------ a view against a voxel
struct TsdfFrames {
    const float* depth;
    const float* rgb;
    const float* poses;
    uint32_t n, H, W, flags;
    double fx, fy, cx, cy, trunc, depth_max, max_weight;
};

struct TsdfGrid {
    const double* ticks[3];
    float* tsdf;
    float* weight;
    float* color;
    uint32_t X, Y, Z;
    uint32_t bricks_y, bricks_z;
};

// Whether view k can update a voxel of the ball (centre c, radius r) that holds the brick.  With cc the centre in the camera frame
// and a point of the ball at most r_c = r * |column c of R| from it along camera axis c (Cauchy-Schwarz on the header's
// cam[c] = column c of R . q), a pair can update only when
//   z > 0                       ->  zc + r_z > 0
//   z <= d + trunc <= depth_max + trunc  ->  zc - r_z <= depth_max + trunc
//   -0.5 <= u < W - 0.5         ->  x - a0 z >= 0 and x - a1 z <= 0 with a0 = (-1.5 - cx)/fx, a1 = (W + 0.5 - cx)/fx, and the like for v
// The image is so taken a pixel wider on every side, and r a millionth larger plus 1e-9 of the scene's scale, which is many orders
// above the rounding of the rule's own u, v and z (relative 1e-15) wherever the rule's z is large enough to land in the image at
// all; where it is not, the voxel is within rounding of the camera centre, the ball holds the centre and every test passes.  A
// pose with an entry that is not finite updates nothing (cam, u or v is then infinite or NaN for every voxel, or z is and
// sdf = -inf) and is left out.  NaN ticks among finite ones are ignored by the box (fmin, fmax): their voxels
// project nowhere.
__device__ __forceinline__ bool tsdf_view_can_update(const TsdfFrames& s, uint32_t k, const double c[3], double r) {
    const float* P = s.poses + (size_t)k * 16;
    double R[9], t[3], scale = 1.0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        R[i * 3] = (double)P[i * 4], R[i * 3 + 1] = (double)P[i * 4 + 1], R[i * 3 + 2] = (double)P[i * 4 + 2];
        t[i] = (double)P[i * 4 + 3];
        finite = finite && fabs(R[i * 3]) < INFINITY && fabs(R[i * 3 + 1]) < INFINITY && fabs(R[i * 3 + 2]) < INFINITY && fabs(t[i]) < INFINITY;
        scale += fabs(t[i]) + fabs(c[i]);
    }
    if (!finite) return false;
    const double q[3] = {c[0] - t[0], c[1] - t[1], c[2] - t[2]};
    const double rr = r * 1.000001 + 1.0e-9 * scale;
    double cc[3], rc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cc[a] = (R[a] * q[0] + R[3 + a] * q[1]) + R[6 + a] * q[2];
        rc[a] = rr * sqrt((R[a] * R[a] + R[3 + a] * R[3 + a]) + R[6 + a] * R[6 + a]) * 1.000001;
    }
    const double zc = -cc[2];
    bool keep = zc + rc[2] > 0.0 && zc - rc[2] <= s.depth_max + s.trunc;
    const double a0 = (-1.5 - s.cx) / s.fx, a1 = ((double)s.W + 0.5 - s.cx) / s.fx;
    keep = keep && (cc[0] - a0 * zc) + (rc[0] + fabs(a0) * rc[2]) >= 0.0 && (cc[0] - a1 * zc) - (rc[0] + fabs(a1) * rc[2]) <= 0.0;
    // v = cy - fy*(y/z) in [-1.5, H + 0.5]  ->  y/z in [b0, b1] = [(cy - H - 0.5)/fy, (cy + 1.5)/fy]
    const double b0 = (s.cy - (double)s.H - 0.5) / s.fy, b1 = (s.cy + 1.5) / s.fy;
    keep = keep && (cc[1] - b0 * zc) + (rc[1] + fabs(b0) * rc[2]) >= 0.0 && (cc[1] - b1 * zc) - (rc[1] + fabs(b1) * rc[2]) <= 0.0;
    return keep;
}

// The ball that holds the voxels of the brick [x0,x1) x [y0,y1) x [z0,z1): the box of their positions, its centre and half its
// diagonal (every lane the same).  -> whether there is a ball to test: a tick that is infinite (or NaN on a whole axis) leaves
// none, and such a brick takes every view.
__device__ __forceinline__ bool tsdf_brick_ball(const TsdfGrid& vol, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1,
                                                double c[3], double& radius) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t a = x0; a < x1; ++a) lo[0] = fmin(lo[0], (double)(float)vol.ticks[0][a]), hi[0] = fmax(hi[0], (double)(float)vol.ticks[0][a]);
    for (uint32_t a = y0; a < y1; ++a) lo[1] = fmin(lo[1], (double)(float)vol.ticks[1][a]), hi[1] = fmax(hi[1], (double)(float)vol.ticks[1][a]);
    for (uint32_t a = z0; a < z1; ++a) lo[2] = fmin(lo[2], (double)(float)vol.ticks[2][a]), hi[2] = fmax(hi[2], (double)(float)vol.ticks[2][a]);
    double h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = 0.5 * lo[a] + 0.5 * hi[a], h[a] = fmax(hi[a] - c[a], c[a] - lo[a]);
    radius = sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
    return fabs(c[0]) < INFINITY && fabs(c[1]) < INFINITY && fabs(c[2]) < INFINITY && radius < INFINITY;
}

// The part of the header's projection that a row of voxels along z shares: q.x and q.y are those of the row, so the first two
// products of every cam[c] are formed once per view.
struct TsdfViewRow {
    double pre0, pre1, pre2, r20, r21, r22, tz;
};
__device__ __forceinline__ TsdfViewRow tsdf_view_row(const float* P, double px, double py) {
    const double qx = px - (double)P[3], qy = py - (double)P[7];
    TsdfViewRow v;
    v.tz = (double)P[11];
    v.r20 = (double)P[8], v.r21 = (double)P[9], v.r22 = (double)P[10];
    v.pre0 = (double)P[0] * qx + (double)P[4] * qy;
    v.pre1 = (double)P[1] * qx + (double)P[5] * qy;
    v.pre2 = (double)P[2] * qx + (double)P[6] * qy;
    return v;
}

// `updated` of mipsf_tsdf_integrate for the voxel of the row at pz and the view with depth image D; when it holds, the pixel and
// val = min(sdf/trunc, 1)
__device__ __forceinline__ bool tsdf_view_hits(const TsdfFrames& s, const TsdfViewRow& v, const float* __restrict__ D, double pz, size_t& pixel,
                                               double& val) {
    const double qz = pz - v.tz;
    const double cam0 = v.pre0 + v.r20 * qz, cam1 = v.pre1 + v.r21 * qz, cam2 = v.pre2 + v.r22 * qz;
    const double z = -cam2;
    const double u = s.cx + s.fx * (cam0 / z);
    const double w = s.cy - s.fy * (cam1 / z);
    const double col = floor(u + 0.5), row = floor(w + 0.5);
    if (!(z > 0.0 && col >= 0.0 && col < (double)s.W && row >= 0.0 && row < (double)s.H)) return false;
    pixel = (size_t)(uint32_t)row * s.W + (uint32_t)col;
    const double d = (double)D[pixel];
    const double sdf = d - z;
    if (!(d > 0.0 && d < INFINITY && d <= s.depth_max && sdf >= -s.trunc)) return false;
    val = sdf / s.trunc;
    if (val > 1.0) val = 1.0;
    return true;
}

// What a view that hits a voxel does to its running words when it is taken out again (the rule of include/mipsf_deintegrate.h):
// stated once for tsdf_remove.hip and sparse_remove.hip.  val is tsdf_view_hits's; C the view's colour at the pixel (COLOR only).
template <bool COLOR>
__device__ __forceinline__ void tsdf_remove_step(float& tsdf, float& weight, float* color, double val, const float* __restrict__ C, uint64_t& removed,
                                                 uint64_t& missing, uint64_t& emptied) {
    const double w0 = (double)weight;
    if (!(w0 > 0.0)) {                                                          // nothing of this view is in the voxel (a NaN weight too)
        ++missing;
        return;
    }
    ++removed;
    const double w1 = w0 - 1.0;
    if (!(w1 > 0.0)) {                                                          // the last view leaves: the never-observed state
        tsdf = 0.0f, weight = 0.0f;
        if (COLOR) color[0] = color[1] = color[2] = 0.0f;
        ++emptied;
        return;
    }
    tsdf = (float)((((double)tsdf) * w0 - val) / w1);
    if (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) color[ch] = (float)((((double)color[ch]) * w0 - (double)C[ch]) / w1);
    }
    weight = (float)w1;
}

// ------------------------------------------------------------------------------------------------ the colour of a point

struct TsdfAxis {
    uint32_t i0, i1;
    double f;
};
__device__ __forceinline__ TsdfAxis tsdf_axis_of(double x, uint32_t D) {
    if (D < 2) return TsdfAxis{0u, 0u, fmin(fmax(x, 0.0), 1.0)};
    const double i0 = fmin(fmax(floor(x), 0.0), (double)(D - 2));
    return TsdfAxis{(uint32_t)i0, (uint32_t)i0 + 1u, fmin(fmax(x - i0, 0.0), 1.0)};
}

// (x, y, z) in index units -> res[3]
__device__ __forceinline__ void tsdf_sample_color(double x, double y, double z, uint32_t X, uint32_t Y, uint32_t Z, const float* __restrict__ weight,
                                                  const float* __restrict__ color, float res[3]) {
    res[0] = res[1] = res[2] = 0.0f;
    if (fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY) {
        const TsdfAxis ax = tsdf_axis_of(x, X), ay = tsdf_axis_of(y, Y), az = tsdf_axis_of(z, Z);
        double den = 0.0, num[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const bool a = corner & 4, b = corner & 2, c = corner & 1;
            const double share = ((a ? ax.f : 1.0 - ax.f) * (b ? ay.f : 1.0 - ay.f)) * (c ? az.f : 1.0 - az.f);
            const size_t idx = ((size_t)(a ? ax.i1 : ax.i0) * Y + (b ? ay.i1 : ay.i0)) * Z + (c ? az.i1 : az.i0);
            const double mshare = weight[idx] > 0.0f ? share : 0.0;
            den = den + mshare;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) num[ch] = num[ch] + mshare * (double)color[idx * 3 + ch];
        }
        if (den > 0.0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) res[ch] = (float)(num[ch] / den);
        }
    }
}

}  // namespace mipsf
