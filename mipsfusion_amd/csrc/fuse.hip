// The scene as one mesh (include/mipsf_fuse.h): visibility of points from keyframes, fusion of the sub-maps' SDFs on one grid,
// connected components of a mesh.  Upstream: model/Mesher.py extract_mesh_jointly, vis/math_helper.py.  DESIGN.md 4.13.
//
// Shape of the kernels: one point per lane.  A keyframe record is the same for every lane of a wave, so it is read through
// uniform (scalar, constant-cache) loads; a wave leaves the keyframe loop as soon as a 64-bit ballot shows no lane still
// waiting to be seen.  Nothing of size [keyframes, points] or [points, sub-maps] exists.  The library is built with
// -ffp-contract=off: the fp32 expressions below round where the upstream's torch expressions round.
#include "common.h"
#include "../../include/mipsf_fuse.h"

#include <math.h>

namespace mipsf {
namespace {

constexpr int TPB = 256;

struct Item {
    float x, y, z;
    uint32_t row;       // the item's row in a per-voxel / per-vertex state array
};

// item first + p of the description; the caller has checked p < n
__device__ __forceinline__ Item fetch(const mipsf_fuse_points& P, uint32_t p) {
    Item it;
    const uint32_t q = P.first + p;
    if (P.points) {
        const float* s = P.points + (size_t)q * 3;
        it.x = s[0], it.y = s[1], it.z = s[2];
        it.row = q;
    } else {
        const uint32_t iz = q % P.size[2], t = q / P.size[2];
        const uint32_t iy = t % P.size[1], ix = t / P.size[1];
        const uint32_t gx = P.lo[0] + ix, gy = P.lo[1] + iy, gz = P.lo[2] + iz;
        it.x = (float)P.ticks[0][gx], it.y = (float)P.ticks[1][gy], it.z = (float)P.ticks[2][gz];
        it.row = (gx * P.dims[1] + gy) * P.dims[2] + gz;
    }
    return it;
}

// Mesher.py:261-280 for one keyframe record r (MIPSF_FUSE_KF_FLOATS floats, wave-uniform address)
__device__ __forceinline__ bool seen_by(const float* __restrict__ r, const Item& it, const mipsf_fuse_camera& c) {
    const float px = ((it.x * r[0] + it.y * r[1]) + it.z * r[2]) + r[3];
    const float py = ((it.x * r[4] + it.y * r[5]) + it.z * r[6]) + r[7];
    const float pz = ((it.x * r[8] + it.y * r[9]) + it.z * r[10]) + r[11];
    const float den = pz + 1e-5f;
    const float u = (c.fx * (-px) + c.cx * pz) / den;
    const float v = (c.fy * py + c.cy * pz) / den;
    const float az = fabsf(pz);
    return (u < c.W - c.edge) && (u > c.edge) && (v < c.H - c.edge) && (v > c.edge) && (pz < 0.0f) && (az > 0.0f) && (az < r[12]);
}

// OR over the keyframes; `want` = this lane has a point that is still to be tested.  Wave-uniform trip count.
__device__ __forceinline__ bool seen_by_any(const mipsf_fuse_camera& c, const Item& it, bool want) {
    bool seen = false;
    for (uint32_t j = 0; j < c.k; ++j) {
        if (__ballot(want && !seen) == 0ull) break;
        seen = seen || seen_by(c.keyframes + (size_t)j * MIPSF_FUSE_KF_FLOATS, it, c);
    }
    return want && seen;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) fuse_visibility_kernel(mipsf_fuse_points P, mipsf_fuse_camera cam,
                                                                                uint8_t* __restrict__ seen) {
    const uint32_t p = blockIdx.x * TPB + threadIdx.x;
    const bool live = p < P.n;
    Item it = {0.f, 0.f, 0.f, 0u};
    if (live) it = fetch(P, p);
    const bool s = seen_by_any(cam, it, live);
    if (live) seen[p] = s ? 1 : 0;
}

struct LocalCfg {
    float w2l[12];
    double sub[3], div[3];
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) fuse_local_kernel(mipsf_fuse_points P, LocalCfg L, double* __restrict__ out) {
    const uint32_t p = blockIdx.x * TPB + threadIdx.x;
    if (p >= P.n) return;
    const Item it = fetch(P, p);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float l = ((it.x * L.w2l[4 * d] + it.y * L.w2l[4 * d + 1]) + it.z * L.w2l[4 * d + 2]) + L.w2l[4 * d + 3];
        out[(size_t)p * 3 + d] = ((double)l - L.sub[d]) / L.div[d];
    }
}

struct AccumCfg {
    const int32_t* rows;
    uint32_t n_rows, channels, sigmoid;
    const float* values;
    const float* entropy;
    uint32_t value_stride, entropy_stride, use_obb;
    double obb_centre[3], obb_axes[9], obb_half[3];
    float centroid[3], sigma, gauss_k;
    float* num;
    float* den;
    uint8_t* flags;
};

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) fuse_accumulate_kernel(mipsf_fuse_points P, mipsf_fuse_camera cam, AccumCfg A) {
    const uint32_t p = blockIdx.x * TPB + threadIdx.x;
    bool live = p < P.n;
    Item it = {0.f, 0.f, 0.f, 0u};
    if (live) {
        it = fetch(P, p);
        if (A.rows) it.row = (uint32_t)A.rows[p];
        live = it.row < A.n_rows;
    }
    bool inside = live;
    if (live && A.use_obb) {
        const double dx = (double)it.x - A.obb_centre[0], dy = (double)it.y - A.obb_centre[1], dz = (double)it.z - A.obb_centre[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double s = (dx * A.obb_axes[i] + dy * A.obb_axes[3 + i]) + dz * A.obb_axes[6 + i];
            inside = inside && (fabs(s) <= A.obb_half[i]);
        }
    }
    const bool on = seen_by_any(cam, it, inside);
    if (!live) return;
    uint8_t f = MIPSF_FUSE_IN_BOX;
    if (on) {
        f |= MIPSF_FUSE_SEEN;
        const float e = fminf(fmaxf(A.entropy[(size_t)p * A.entropy_stride], 0.0f), 10000.0f);
        const float dx = it.x - A.centroid[0], dy = it.y - A.centroid[1], dz = it.z - A.centroid[2];
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float m = dist / A.sigma;
        const float w = expf(-10.0f * e) * (A.gauss_k * expf(-0.5f * (m * m)));
        for (uint32_t c = 0; c < A.channels; ++c) {
            float v = A.values[(size_t)p * A.value_stride + c];
            if (A.sigmoid) v = 1.0f / (1.0f + expf(-v));
            A.num[(size_t)it.row * A.channels + c] += w * v;
        }
        A.den[it.row] += w;
    }
    if (A.flags) A.flags[it.row] |= f;
}

MIPSF_SINGLE_FP32 __global__ void __launch_bounds__(TPB) fuse_finalize_kernel(uint32_t n, uint32_t channels, const float* __restrict__ num,
                                                                              const float* __restrict__ den,
                                                                              const uint8_t* __restrict__ flags, float* __restrict__ out,
                                                                              float* __restrict__ volume) {
    const uint32_t r = blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    const float d = den[r];
    const uint32_t f = flags ? flags[r] : (MIPSF_FUSE_IN_BOX | MIPSF_FUSE_SEEN);
    const bool seen = (f & MIPSF_FUSE_SEEN) != 0;
    float first = 0.0f;
    for (uint32_t c = 0; c < channels; ++c) {
        const float v = seen ? (d > 0.0f ? num[(size_t)r * channels + c] / d : 0.0f) : -1.0f;
        if (c == 0) first = v;
        if (out) out[(size_t)r * channels + c] = v;
    }
    if (volume) volume[r] = (seen && (f & MIPSF_FUSE_IN_BOX)) ? first : -INFINITY;
}

// ---- connected components: labels only ever decrease and labels[i] <= i, so every chain ends at a root (labels[r] == r)
__device__ __forceinline__ int32_t root_of(const int32_t* labels, int32_t i) {
    int32_t t;
    while ((t = __atomic_load_n(labels + i, __ATOMIC_RELAXED)) != i) i = t;
    return i;
}

__global__ void __launch_bounds__(TPB) label_init_kernel(int32_t* labels, uint32_t F, uint32_t* counts) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < F) labels[i] = (int32_t)i;
    if (i < 4) counts[i] = 0;
}

__global__ void __launch_bounds__(TPB) label_hook_kernel(const int32_t* __restrict__ pairs, uint32_t E, uint32_t F, int32_t* labels,
                                                         uint32_t* counts) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const int32_t a = pairs[2 * (size_t)e], b = pairs[2 * (size_t)e + 1];
    if ((uint32_t)a >= F || (uint32_t)b >= F) return;
    const int32_t ra = root_of(labels, a), rb = root_of(labels, b);
    if (ra == rb) return;
    atomicMin(labels + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    counts[2] = 1;
}

__global__ void __launch_bounds__(TPB) label_jump_kernel(int32_t* labels, uint32_t F) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= F) return;
    const int32_t r = root_of(labels, (int32_t)i);
    __atomic_store_n(labels + i, r, __ATOMIC_RELAXED);
}

__global__ void label_round_end_kernel(uint32_t* counts) {
    if (threadIdx.x == 0 && counts[2]) {
        counts[1] += 1;
        counts[2] = 0;
    }
}

int points_check(const mipsf_fuse_points& P, const char* who) {
    if (P.points) return 0;
    MIPSF_REQUIRE(P.ticks[0] && P.ticks[1] && P.ticks[2], "%s: neither a point list nor tick arrays", who);
    MIPSF_REQUIRE((uint64_t)P.dims[0] * P.dims[1] * P.dims[2] < (1ull << 31), "%s: grid of 2^31 points or more", who);
    for (int d = 0; d < 3; ++d)
        MIPSF_REQUIRE(P.size[d] >= 1 && (uint64_t)P.lo[d] + P.size[d] <= P.dims[d], "%s: sub-box [%u, %u + %u) leaves axis %d of %u ticks",
                      who, P.lo[d], P.lo[d], P.size[d], d, P.dims[d]);
    MIPSF_REQUIRE((uint64_t)P.first + P.n <= (uint64_t)P.size[0] * P.size[1] * P.size[2], "%s: items %u + %u leave the sub-box", who,
                  P.first, P.n);
    return 0;
}

int camera_check(const mipsf_fuse_camera& c, const char* who) {
    MIPSF_REQUIRE(c.k == 0 || c.keyframes != nullptr, "%s: null keyframe table", who);
    MIPSF_REQUIRE(((uintptr_t)c.keyframes & 63u) == 0, "%s: the keyframe table must be 64-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" int mipsf_fuse_visibility(const mipsf_fuse_visibility_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_fuse_visibility_args, "mipsf_fuse_visibility");
    if (a->pts.n == 0) return 0;
    if (points_check(a->pts, "mipsf_fuse_visibility") || camera_check(a->cam, "mipsf_fuse_visibility")) return 1;
    MIPSF_REQUIRE(a->seen != nullptr, "mipsf_fuse_visibility: null output");
    hipLaunchKernelGGL(fuse_visibility_kernel, dim3(blocks_for(a->pts.n, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->pts, a->cam, a->seen);
    return check_launch("fuse_visibility");
}

extern "C" int mipsf_fuse_local_points(const mipsf_fuse_local_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_fuse_local_args, "mipsf_fuse_local_points");
    if (a->pts.n == 0) return 0;
    if (points_check(a->pts, "mipsf_fuse_local_points")) return 1;
    MIPSF_REQUIRE(a->out != nullptr, "mipsf_fuse_local_points: null output");
    LocalCfg L;
    for (int i = 0; i < 12; ++i) L.w2l[i] = a->w2l[i];
    for (int d = 0; d < 3; ++d) {
        MIPSF_REQUIRE(a->div[d] != 0.0, "mipsf_fuse_local_points: zero extent on axis %d", d);
        L.sub[d] = a->sub[d], L.div[d] = a->div[d];
    }
    hipLaunchKernelGGL(fuse_local_kernel, dim3(blocks_for(a->pts.n, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->pts, L, a->out);
    return check_launch("fuse_local_points");
}

extern "C" int mipsf_fuse_accumulate(const mipsf_fuse_accumulate_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_fuse_accumulate_args, "mipsf_fuse_accumulate");
    if (a->pts.n == 0) return 0;
    if (points_check(a->pts, "mipsf_fuse_accumulate") || camera_check(a->cam, "mipsf_fuse_accumulate")) return 1;
    MIPSF_REQUIRE(a->channels == 1 || a->channels == 3, "mipsf_fuse_accumulate: %u channels (1 or 3)", a->channels);
    MIPSF_REQUIRE(a->values && a->entropy && a->num && a->den, "mipsf_fuse_accumulate: null pointer");
    MIPSF_REQUIRE(a->value_stride >= a->channels && a->entropy_stride >= 1, "mipsf_fuse_accumulate: bad strides");
    MIPSF_REQUIRE(a->rows == nullptr || a->pts.points != nullptr, "mipsf_fuse_accumulate: `rows` goes with a point list");
    MIPSF_REQUIRE(a->sigma > 0.0f && a->n_rows > 0, "mipsf_fuse_accumulate: sigma must be positive and n_rows non-zero");
    if (!a->pts.points)
        MIPSF_REQUIRE((uint64_t)a->pts.dims[0] * a->pts.dims[1] * a->pts.dims[2] <= a->n_rows, "mipsf_fuse_accumulate: the state has %u rows, the grid more", a->n_rows);
    else if (!a->rows)
        MIPSF_REQUIRE((uint64_t)a->pts.first + a->pts.n <= a->n_rows, "mipsf_fuse_accumulate: the state has %u rows, the list more", a->n_rows);
    AccumCfg A;
    A.rows = a->rows, A.n_rows = a->n_rows, A.channels = a->channels, A.sigmoid = a->sigmoid;
    A.values = a->values, A.entropy = a->entropy, A.value_stride = a->value_stride, A.entropy_stride = a->entropy_stride;
    A.use_obb = a->use_obb;
    for (int i = 0; i < 3; ++i) A.obb_centre[i] = a->obb_centre[i], A.obb_half[i] = a->obb_half[i], A.centroid[i] = a->centroid[i];
    for (int i = 0; i < 9; ++i) A.obb_axes[i] = a->obb_axes[i];
    A.sigma = a->sigma, A.gauss_k = a->gauss_k;
    A.num = a->num, A.den = a->den, A.flags = a->flags;
    hipLaunchKernelGGL(fuse_accumulate_kernel, dim3(blocks_for(a->pts.n, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->pts, a->cam, A);
    return check_launch("fuse_accumulate");
}

extern "C" int mipsf_fuse_finalize(const mipsf_fuse_finalize_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_fuse_finalize_args, "mipsf_fuse_finalize");
    if (a->n == 0) return 0;
    MIPSF_REQUIRE(a->num && a->den && (a->out || a->volume), "mipsf_fuse_finalize: null pointer");
    MIPSF_REQUIRE(a->channels == 1 || (a->channels == 3 && !a->volume), "mipsf_fuse_finalize: %u channels (1, or 3 without a volume)",
                  a->channels);
    hipLaunchKernelGGL(fuse_finalize_kernel, dim3(blocks_for(a->n, TPB)), dim3(TPB), 0, (hipStream_t)stream, a->n, a->channels, a->num, a->den,
                       a->flags, a->out, a->volume);
    return check_launch("fuse_finalize");
}

extern "C" int mipsf_fuse_label_components(const mipsf_fuse_label_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_fuse_label_args, "mipsf_fuse_label_components");
    MIPSF_REQUIRE(a->counts != nullptr, "mipsf_fuse_label_components: null counts");
    MIPSF_REQUIRE(a->F < (1u << 31) && a->E < (1u << 31), "mipsf_fuse_label_components: 2^31 items or pairs, or more");
    MIPSF_REQUIRE(a->F == 0 || a->labels != nullptr, "mipsf_fuse_label_components: null labels");
    MIPSF_REQUIRE(a->E == 0 || a->pairs != nullptr, "mipsf_fuse_label_components: null pairs");
    const hipStream_t s = (hipStream_t)stream;
    if (!a->resume) hipLaunchKernelGGL(label_init_kernel, dim3(blocks_for(a->F > 4 ? a->F : 4, TPB)), dim3(TPB), 0, s, a->labels, a->F, a->counts);
    if (a->F && a->E)
        for (uint32_t r = 0; r < a->max_rounds; ++r) {
            hipLaunchKernelGGL(label_hook_kernel, dim3(blocks_for(a->E, TPB)), dim3(TPB), 0, s, a->pairs, a->E, a->F, a->labels, a->counts);
            hipLaunchKernelGGL(label_jump_kernel, dim3(blocks_for(a->F, TPB)), dim3(TPB), 0, s, a->labels, a->F);
            hipLaunchKernelGGL(label_round_end_kernel, dim3(1), dim3(64), 0, s, a->counts);
        }
    return check_launch("fuse_label_components");
}
