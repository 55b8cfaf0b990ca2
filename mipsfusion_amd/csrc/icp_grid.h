// The uniform grid mipsf_icp_bin builds over a cloud (include/mipsf_icp.h), as its readers see it: the layout of the blob, the
// device view, the cell of a coordinate and the float64 squared distance every search orders by.  Stated once for icp.hip (which
// builds the grid and searches it within a radius) and eval.hip (which searches it without one).
#pragma once
#include "common.h"

#include <math.h>

namespace mipsf {

constexpr int GRID_TPB = 256;                 // threads of the grid's kernels; the box partials are per block of this size
constexpr int GRID_SCAN_TILE = GRID_TPB * 4;  // entries one block of the cell scan takes (block_dev.h: SCAN_ITEMS a thread)

struct GridHdr {
    double origin[3];
    double edge;
    uint32_t dims[3];
    uint32_t ncells;
    uint32_t pad[4];
};
static_assert(sizeof(GridHdr) == 64, "GridHdr");

struct GridLayout {
    uint64_t hdr, bbox, start, cnt, bsum, sorted, bytes;
};

inline GridLayout grid_layout(uint32_t n, uint32_t cells) {
    GridLayout L;
    L.hdr = 0;
    L.bbox = 128;
    L.start = align16(L.bbox + (uint64_t)blocks_for(n ? n : 1, GRID_TPB) * 6 * sizeof(float));
    L.cnt = align16(L.start + ((uint64_t)cells + 1) * 4);
    L.bsum = align16(L.cnt + ((uint64_t)cells + 1) * 4);
    L.sorted = align16(L.bsum + (uint64_t)blocks_for((uint64_t)cells + 1, GRID_SCAN_TILE) * 4);
    L.bytes = L.sorted + (uint64_t)(n ? n : 1) * 16;
    return L;
}

struct Grid {       // device view
    const GridHdr* hdr;
    const uint32_t* start;
    const float4* sorted;
};

inline Grid grid_view(const void* blob, uint32_t n, uint32_t cells) {
    const GridLayout L = grid_layout(n, cells);
    const char* b = (const char*)blob;
    return Grid{(const GridHdr*)(b + L.hdr), (const uint32_t*)(b + L.start), (const float4*)(b + L.sorted)};
}

// cell coordinate of x along an axis, clamped into the grid (NaN -> 0)
__device__ __forceinline__ uint32_t cell_of(double x, double origin, double edge, uint32_t dim) {
    const double f = floor((x - origin) / edge);
    return f >= (double)(dim - 1) ? dim - 1 : (f > 0.0 ? (uint32_t)f : 0u);
}

__device__ __forceinline__ double dist2(double qx, double qy, double qz, const float4& v) {
    const double dx = qx - (double)v.x, dy = qy - (double)v.y, dz = qz - (double)v.z;
    return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace mipsf
