// The brick-sparse volume as the kernels read it (include/mipsf_sparse.h), stated once for sparse.hip, which fuses, gathers and ray
// casts it, sparse_mesh.hip, which marches it brick by brick, sparse_remove.hip, which takes views out of it again, and
// sparse_release.hip, which gives slots back: the volume by
// value, voxel -> word of the pool through the table, the colour of a point (the rule of mipsf_tsdf_sample with the corner reads
// through the table), and what every entry point refuses of a volume and of the views.
#pragma once
#include <math.h>

#include "tsdf_dev.h"
#include "../../include/mipsf_sparse.h"

namespace mipsf {

constexpr uint32_t BRICK_X = MIPSF_TSDF_BRICK_X, BRICK_Y = MIPSF_TSDF_BRICK_Y, BRICK_Z = MIPSF_TSDF_BRICK_Z;
constexpr uint32_t BRICK_VOXELS = MIPSF_SPARSE_BRICK_VOXELS;
static_assert(BRICK_X * BRICK_Y * BRICK_Z == BRICK_VOXELS, "the words of a slot");

struct Pool {
    const double* ticks[3];
    int32_t* table;
    int32_t* slot_brick;
    uint32_t* birth;
    uint32_t* count;
    float* tsdf;
    float* weight;
    float* color;
    uint32_t X, Y, Z, capacity;
    uint32_t bricks_y, bricks_z, bricks;
    double origin[3], voxel;
};

__device__ __forceinline__ uint32_t brick_of(const Pool& v, uint32_t i, uint32_t j, uint32_t k) {
    return ((i / BRICK_X) * v.bricks_y + j / BRICK_Y) * v.bricks_z + k / BRICK_Z;      // below 2^31: the host refuses more bricks
}

// the word of voxel (i, j, k) in the pool, or -1: its brick has no slot
__device__ __forceinline__ int32_t word_of(const Pool& v, uint32_t i, uint32_t j, uint32_t k) {
    const int32_t slot = v.table[brick_of(v, i, j, k)];
    return slot < 0 ? -1 : (int32_t)((uint32_t)slot * BRICK_VOXELS + ((i % BRICK_X) * BRICK_Y + j % BRICK_Y) * BRICK_Z + k % BRICK_Z);
}

// the rule of mipsf_tsdf_sample (tsdf_dev.h states it for dense arrays) with the corner reads through the table
__device__ __forceinline__ void sample_color(const Pool& v, double x, double y, double z, float res[3]) {
    res[0] = res[1] = res[2] = 0.0f;
    if (fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY) {
        const TsdfAxis ax = tsdf_axis_of(x, v.X), ay = tsdf_axis_of(y, v.Y), az = tsdf_axis_of(z, v.Z);
        double den = 0.0, num[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const bool a = corner & 4, b = corner & 2, c = corner & 1;
            const double share = ((a ? ax.f : 1.0 - ax.f) * (b ? ay.f : 1.0 - ay.f)) * (c ? az.f : 1.0 - az.f);
            const int32_t at = word_of(v, a ? ax.i1 : ax.i0, b ? ay.i1 : ay.i0, c ? az.i1 : az.i0);
            const double mshare = (at < 0 ? 0.0f : v.weight[at]) > 0.0f ? share : 0.0;
            den = den + mshare;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) num[ch] = num[ch] + mshare * (double)(at < 0 ? 0.0f : v.color[(size_t)at * 3 + ch]);
        }
        if (den > 0.0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) res[ch] = (float)(num[ch] / den);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
inline bool pos_finite(double x) { return x > 0.0 && x < INFINITY; }
inline bool is_finite(double x) { return fabs(x) < INFINITY; }

inline uint64_t brick_count(uint32_t X, uint32_t Y, uint32_t Z) {
    return (uint64_t)blocks_for(X, BRICK_X) * blocks_for(Y, BRICK_Y) * blocks_for(Z, BRICK_Z);
}

// what every entry point refuses of the volume; 0: fine
inline int volume_ok(const mipsf_sparse_volume& g, const char* who) {
    MIPSF_REQUIRE(g.X > 0 && g.Y > 0 && g.Z > 0, "%s: a grid of %u x %u x %u has no voxels", who, g.X, g.Y, g.Z);
    // three factors below 2^29 each: the product of the first two fits 64 bits, and is compared before the third comes in
    const uint64_t xy = (uint64_t)blocks_for(g.X, BRICK_X) * blocks_for(g.Y, BRICK_Y);
    MIPSF_REQUIRE(xy <= MIPSF_SPARSE_MAX_BRICKS && xy * blocks_for(g.Z, BRICK_Z) <= MIPSF_SPARSE_MAX_BRICKS,
                  "%s: a grid of %u x %u x %u voxels has 2^31 bricks or more", who, g.X, g.Y, g.Z);
    MIPSF_REQUIRE(g.capacity > 0 && g.capacity <= MIPSF_SPARSE_MAX_CAPACITY, "%s: capacity %u, from 1 to %u slots", who, g.capacity,
                  MIPSF_SPARSE_MAX_CAPACITY);
    MIPSF_REQUIRE(pos_finite(g.voxel), "%s: voxel %g is not positive and finite", who, g.voxel);
    MIPSF_REQUIRE(is_finite(g.origin[0]) && is_finite(g.origin[1]) && is_finite(g.origin[2]), "%s: origin %g %g %g", who, g.origin[0], g.origin[1],
                  g.origin[2]);
    MIPSF_REQUIRE(g.ticks[0] && g.ticks[1] && g.ticks[2] && g.table && g.slot_brick && g.birth && g.count && g.tsdf && g.weight,
                  "%s: null pointer in the volume", who);
    return 0;
}

// what the entry points that take views refuse of the images and the intrinsics; 0: fine
inline int images_ok(uint32_t n, uint32_t H, uint32_t W, double fx, double fy, double cx, double cy, const char* who) {
    MIPSF_REQUIRE(n == 0 || (H > 0 && W > 0), "%s: an image of %u x %u has no pixels", who, H, W);
    MIPSF_REQUIRE(H <= MIPSF_TSDF_MAX_SIDE && W <= MIPSF_TSDF_MAX_SIDE, "%s: image %u x %u, at most %u a side", who, H, W, MIPSF_TSDF_MAX_SIDE);
    MIPSF_REQUIRE(n <= MIPSF_SPARSE_MAX_VIEWS, "%s: %u views, at most %u a call", who, n, MIPSF_SPARSE_MAX_VIEWS);
    MIPSF_REQUIRE(pos_finite(fx) && pos_finite(fy) && is_finite(cx) && is_finite(cy), "%s: intrinsics %g %g %g %g", who, fx, fy, cx, cy);
    return 0;
}

inline Pool pool_of(const mipsf_sparse_volume& g) {
    Pool v;
    for (int d = 0; d < 3; ++d) v.ticks[d] = g.ticks[d], v.origin[d] = g.origin[d];
    v.table = g.table, v.slot_brick = g.slot_brick, v.birth = g.birth, v.count = g.count;
    v.tsdf = g.tsdf, v.weight = g.weight, v.color = g.color;
    v.X = g.X, v.Y = g.Y, v.Z = g.Z, v.capacity = g.capacity;
    v.bricks_y = blocks_for(g.Y, BRICK_Y), v.bricks_z = blocks_for(g.Z, BRICK_Z), v.bricks = (uint32_t)brick_count(g.X, g.Y, g.Z);
    v.voxel = g.voxel;
    return v;
}

// sparse.hip: the launches of mipsf_sparse_allocate around its mark kernel, with the kernels as they stand there.  sparse_fill:
// p[0..words) = value, by a kernel.  sparse_marks_clear: the record 0, every mark 0xffffffff, every birth 0.  sparse_marks_assign: the
// marked bricks without a slot get the slots count, count + 1, .. in ascending brick index (tile sums, the top block, the tiles
// again); scan[tiles] keeps the count before.
void sparse_fill(void* p, uint64_t words, uint32_t value, hipStream_t st);
void sparse_marks_clear(const Pool& v, uint32_t* mark, mipsf_sparse_alloc_record* record, hipStream_t st);
void sparse_marks_assign(const Pool& v, const uint32_t* mark, uint32_t* scan, mipsf_sparse_alloc_record* record, hipStream_t st);

}  // namespace mipsf
