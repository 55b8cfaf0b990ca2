// The finish step of a point-to-plane registration, stated once for its users: icp.hip (nearest-neighbour pairs between two
// clouds, include/mipsf_icp.h), tsdf_track.hip (projective pairs between a depth frame and a ray-cast model,
// include/mipsf_track.h) and track_color.hip (the same pairs with photometric rows added to the same sums,
// include/mipsf_track_color.h).  All leave the sums of the normal equations per block in partial[block][NSUM_PAD] and enqueue
// max_iteration + 1 evaluations; the `done` word makes the later ones return at once.  Device code only.
#pragma once
#include "common.h"

namespace mipsf {

constexpr int NSUM = 29;                 // 21 (upper triangle of J^T J) + 6 (J^T r) + pairs + sum of squared distances
constexpr int NSUM_PAD = 32;             // column NSUM: the count of source points, where only the device knows it

struct IcpState {
    double T[16];
    double U[12];       // the update the next evaluation applies to its points, 3x4
    double prev_fitness, prev_rmse;
    uint32_t done, iter;
    double prev_color_rmse;   // track_color.hip alone: the photometric rmse of the evaluation before
};
static_assert(sizeof(IcpState) <= 256, "IcpState");

// a pair's share of the sums: J = (p x n, n), residual r, squared distance d2
__device__ __forceinline__ void icp_pair_sums(double c[NSUM], double px, double py, double pz, double nx, double ny, double nz, double r, double d2) {
    const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int bb = a; bb < 6; ++bb) c[k++] = J[a] * J[bb];
#pragma unroll
    for (int a = 0; a < 6; ++a) c[21 + a] = J[a] * r;
    c[27] = 1.0;
    c[28] = d2;
}

// One wave, st->done not set: add the partials in index order, judge the evaluation, and -- unless it was the last -- solve for
// the next update.  COLS = NSUM: the fitness is over n_source; COLS = NSUM + 1: over the sum of column NSUM.  COLS = NSUM_PAD
// (track_color.hip): as NSUM + 1, and column 30 counts photometric rows and column 31 sums their squared residuals; their rmse goes
// to result[20..21] and the relative stop also needs it to have moved by less than rel_color.  Every lane calls.
template <int COLS>
__device__ __forceinline__ void icp_finish(const double* __restrict__ partial, uint32_t nb, uint32_t n_source, IcpState* st, uint32_t max_iteration,
                                           double rel_fitness, double rel_rmse, double* __restrict__ result, double rel_color = 0.0) {
    static_assert(COLS == NSUM || COLS == NSUM + 1 || COLS == NSUM_PAD, "columns of the partials");
    constexpr bool COLOR = COLS == NSUM_PAD;
    __shared__ double S[NSUM_PAD];
    __shared__ double A[6][6];
    __shared__ double x[6];
    if (threadIdx.x < COLS) {
        double s = 0.0;
        for (uint32_t b = 0; b < nb; ++b) s += partial[(size_t)b * NSUM_PAD + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double pairs = S[27];
    const double sources = COLS > NSUM ? S[NSUM] : (double)n_source;
    const double fitness = sources > 0.0 ? pairs / sources : 0.0;
    const double rmse = pairs > 0.0 ? sqrt(S[28] / pairs) : 0.0;
    const uint32_t iter = st->iter;
    double color_rmse = 0.0;
    if constexpr (COLOR) color_rmse = S[30] > 0.0 ? sqrt(S[31] / S[30]) : 0.0;
    bool stop = iter >= max_iteration;
    bool still = iter > 0 && fabs(st->prev_fitness - fitness) < rel_fitness && fabs(st->prev_rmse - rmse) < rel_rmse;
    if constexpr (COLOR) still = still && fabs(st->prev_color_rmse - color_rmse) < rel_color;
    if (still) stop = true;
    for (int j = 0; j < 16; ++j) result[j] = st->T[j];
    result[16] = pairs, result[17] = fitness, result[18] = rmse, result[19] = (double)iter;
    if constexpr (COLOR) result[20] = S[30], result[21] = color_rmse;
    if (stop) {
        st->done = 1u;
        return;
    }
    // J^T J x = -J^T r by Cholesky; no pairs, a pivot that is not above 1e-12 of its diagonal entry (a system without full rank,
    // whatever the rounding made of it) or a solution that is not finite: no update
    bool ok = pairs > 0.0;
    if (ok) {
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = S[k++];
        for (int j = 0; j < 6 && ok; ++j) {
            const double diag = A[j][j];
            double d = diag;
            for (int m = 0; m < j; ++m) d -= A[j][m] * A[j][m];
            ok = d > 0.0 && d > 1.0e-12 * diag;
            if (!ok) break;
            d = sqrt(d);
            A[j][j] = d;
            for (int r = j + 1; r < 6; ++r) {
                double v = A[r][j];
                for (int m = 0; m < j; ++m) v -= A[r][m] * A[j][m];
                A[r][j] = v / d;
            }
        }
    }
    if (ok) {
        for (int r = 0; r < 6; ++r) {
            double v = -S[21 + r];
            for (int m = 0; m < r; ++m) v -= A[r][m] * x[m];
            x[r] = v / A[r][r];
        }
        for (int r = 5; r >= 0; --r) {
            double v = x[r];
            for (int m = r + 1; m < 6; ++m) v -= A[m][r] * x[m];
            x[r] = v / A[r][r];
        }
        for (int r = 0; r < 6; ++r) ok = ok && fabs(x[r]) < INFINITY;
    }
    double U[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (ok) {       // R = Rz(x2) Ry(x1) Rx(x0)
        const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sc = sin(x[2]), cc = cos(x[2]);
        U[0] = cc * cb, U[1] = cc * sb * sa - sc * ca, U[2] = cc * sb * ca + sc * sa, U[3] = x[3];
        U[4] = sc * cb, U[5] = sc * sb * sa + cc * ca, U[6] = sc * sb * ca - cc * sa, U[7] = x[4];
        U[8] = -sb, U[9] = cb * sa, U[10] = cb * ca, U[11] = x[5];
    }
    double Tn[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double v = (U[4 * r] * st->T[c] + U[4 * r + 1] * st->T[4 + c]) + U[4 * r + 2] * st->T[8 + c];
            if (c == 3) v += U[4 * r + 3];
            Tn[4 * r + c] = v;
        }
    for (int j = 0; j < 12; ++j) st->T[j] = Tn[j], st->U[j] = U[j];
    st->prev_fitness = fitness, st->prev_rmse = rmse;
    if constexpr (COLOR) st->prev_color_rmse = color_rmse;
    st->iter = iter + 1u;
}

// the block's sums of c[0..COLS) into partial[block][*]; sm: [WAVES][NSUM_PAD]
template <int WAVES, int COLS>
__device__ __forceinline__ void icp_block_sums(const double* c, double (*sm)[NSUM_PAD], double* __restrict__ partial) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
        const double v = wave_sum_d(c[k]);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < COLS) {
        double v = sm[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) v += sm[w][threadIdx.x];
        partial[(size_t)blockIdx.x * NSUM_PAD + threadIdx.x] = v;
    }
}

}  // namespace mipsf
