// The colour of a point of the fused volume (the rule of mipsf_tsdf_sample, include/mipsf_tsdf.h), stated once for tsdf.hip, which
// colours marched vertices with it, and tsdf_track.hip, which colours the hits of a ray cast.  Device code only.
#pragma once
#include "common.h"
#include "../../include/mipsf_tsdf.h"

namespace mipsf {

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
