// Workgroup reductions and scans, stated once for the geometry units (mcubes, icp, posegraph, submap, eval, raster; fuse has
// none): what a result of theirs is, bit for bit, is decided by the order written here, and tests/*_cpu.py restate that order
// word for word.
//
//   wave    butterfly over the 64 lanes with __shfl_xor 32, 16, .. 1, v = op(v, other lane's v); scans climb __shfl_up 1, 2, .. 32
//   block   one word per wave in sm[WAVES]; the waves are folded in ascending order starting from wave 0: op(op(op(w0, w1), w2), w3)
//   device  block partials (tile sums) in a buffer, then ONE block or ONE wave finishes them
//
// Barriers, the same in every block-level helper: one on entry, before sm is written, and one after the write.  So calls may
// follow each other on the same sm without a barrier between them; a caller that touches sm itself after a call puts a barrier
// before its own write.  Every thread of the block must make the call.
//
// The operators stay with the units: their minima and maxima treat NaN differently (b < a ? b : a, fminf, fmax) and results
// depend on which one a unit uses.  Device code only.
#pragma once
#include "common.h"

namespace mipsf {

struct Add {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// ------------------------------------------------------------------------------------------------ wave (64 lanes)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) { return wave_reduce(v, Add()); }

// uint32_t or uint64_t
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_excl_scan(T v) { return wave_incl_scan(v) - v; }

// ------------------------------------------------------------------------------------------------ block of WAVES waves
// op over the threads of the block, in every thread
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* sm, Op op) {
    v = wave_reduce(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sm[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = op(r, sm[w]);
    return r;
}

// exclusive prefix sum over the threads of the block; *total (optional): the block's sum, in every thread
template <int WAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* sm, T* total = nullptr) {
    const int w = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) sm[w] = inc;
    __syncthreads();
    T base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        if (i < w) base += sm[i];
        all += sm[i];
    }
    if (total) *total = all;
    return base + (inc - v);
}

// ------------------------------------------------------------------------------------------------ device-wide prefix sum
// Three launches of blocks of WAVES waves: the sum of every tile of WAVES * 64 * SCAN_ITEMS items (scan_tile_sum, or the kernel
// that makes the items), ONE block that scans the tile sums in place (scan_top), and the tiles again, each with its offset
// (scan_apply).  Thread t of a tile owns items 4t .. 4t + 3.
constexpr int SCAN_ITEMS = 4;

// the sum of this block's tile of in[0..n), in every thread
template <int WAVES, class T>
__device__ __forceinline__ T scan_tile_sum(const T* in, uint32_t n, T* sm) {
    const uint64_t base = ((uint64_t)blockIdx.x * (WAVES * 64) + threadIdx.x) * SCAN_ITEMS;
    T s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) s += in[base + k];
    return block_reduce<WAVES>(s, sm, Add());
}

// the tile sums thread t of the one top block owns: [lo, hi), chunk = ceil(nb / threads) consecutive ones
template <int WAVES>
__device__ __forceinline__ void scan_top_range(uint32_t nb, uint32_t& lo, uint32_t& hi) {
    const uint32_t chunk = (nb + WAVES * 64 - 1) / (WAVES * 64);
    lo = min(threadIdx.x * chunk, nb), hi = min(lo + chunk, nb);
}

// ONE block: sums[0..nb) becomes its exclusive scan; returns the total in every thread
template <int WAVES, class T>
__device__ __forceinline__ T scan_top(T* sums, uint32_t nb, T* sm) {
    uint32_t lo, hi;
    scan_top_range<WAVES>(nb, lo, hi);
    T s = 0, total;
    for (uint32_t i = lo; i < hi; ++i) s += sums[i];
    T run = block_excl_scan<WAVES>(s, sm, &total);
    for (uint32_t i = lo; i < hi; ++i) {
        const T t = sums[i];
        sums[i] = run;
        run += t;
    }
    return total;
}

// out[0..n) = the prefix sum of in[0..n), with item i itself (Inclusive) or without; sums: what scan_top left; out may be in
template <int WAVES, bool Inclusive, class T>
__device__ __forceinline__ void scan_apply(const T* in, uint32_t n, const T* sums, T* out, T* sm) {
    const uint64_t base = ((uint64_t)blockIdx.x * (WAVES * 64) + threadIdx.x) * SCAN_ITEMS;
    T v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? in[base + k] : (T)0;
        s += v[k];
    }
    T run = block_excl_scan<WAVES>(s, sm) + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (Inclusive) run += v[k];
        if (base + k < n) out[base + k] = run;
        if (!Inclusive) run += v[k];
    }
}

}  // namespace mipsf
