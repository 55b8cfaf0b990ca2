// Sub-map pose graph (include/mipsf_posegraph.h): Levenberg-Marquardt over the anchors of all sub-maps as ONE
// launch of ONE workgroup.  Residuals and Jacobian blocks one edge per lane, the normal equations one 6x6 block per lane with the
// edges of a block added in ascending index, a dense float64 Cholesky and two triangular solves by the workgroup (packed lower
// triangle, in LDS up to MIPSF_POSEGRAPH_LDS_NODES nodes, in the workspace above).  A latency kernel: the barriers between the
// factorisation's columns are its cost.  tests/posegraph_cpu.py is the restatement every formula here follows line by line.
#include "block_dev.h"

#include <math.h>

#include "../../include/mipsf_posegraph.h"

namespace mipsf {
namespace {

constexpr int PG_TPB = 256, PG_WAVES = PG_TPB / MIPSF_WAVE, PG_BATCH = 16;
constexpr int PG_MAX_NODES = MIPSF_POSEGRAPH_MAX_NODES;
constexpr int PG_MAX_EDGES = MIPSF_POSEGRAPH_MAX_EDGES;
constexpr int PG_MAX_N = 6 * (PG_MAX_NODES - 1);                         // unknowns: 378
constexpr int PG_LDS_N = 6 * ((int)MIPSF_POSEGRAPH_LDS_NODES - 1);      // 114
constexpr int PG_LDS_TRI = PG_LDS_N * (PG_LDS_N + 1) / 2;               // 6555 doubles = 52 440 bytes
constexpr int PG_EDGE_DOUBLES = 66;                                      // r 6 | g 6 | S 9 | U 9 | M 36
constexpr double PG_SMALL_ANGLE = 0.05, PG_SMALL_QUAT = 1e-3, PG_MAX_DIAG = 1e32;
static_assert(PG_LDS_TRI * 8 + 3 * PG_MAX_N * 8 + 2 * PG_MAX_EDGES + 128 <= 65536, "posegraph LDS");

// workspace, in doubles: anchors | saved anchors | observations | edge records | the triangle (above PG_LDS_N unknowns)
constexpr uint64_t WS_X = 0, WS_SAVE = WS_X + PG_MAX_NODES * 12, WS_P = WS_SAVE + PG_MAX_NODES * 12, WS_REC = WS_P + (uint64_t)PG_MAX_EDGES * 12;
__host__ __device__ inline uint64_t ws_tri(uint32_t n_edges) { return WS_REC + (uint64_t)n_edges * PG_EDGE_DOUBLES; }

struct PgCfg {
    const void* anchors;
    const int32_t* edges;
    const void* observations;
    const double* weights;
    int n_nodes, n_edges, input_f64, steps, patience, max_rejects;
    double decreasing, radius, min_diag;
    double* out64;
    float* out32;
    double* result;
    double* ws;
};

struct Coef {
    double a, b, c1, c2, c3, ci;
};

__device__ Coef coefficients(double theta) {
    Coef c;
    if (theta < PG_SMALL_ANGLE) {
        const double x = theta * theta;
        c.a = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040)));
        c.b = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320)));
        c.c1 = 1.0 / 6 + x * (-1.0 / 120 + x * (1.0 / 5040 + x * (-1.0 / 362880)));
        c.c2 = 1.0 / 24 + x * (-1.0 / 720 + x * (1.0 / 40320 + x * (-1.0 / 3628800)));
        c.c3 = 1.0 / 120 + x * (-1.0 / 2520 + x * (1.0 / 120960 + x * (-1.0 / 9979200)));
        c.ci = 1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x * (1.0 / 1209600)));
    } else {
        const double t = theta, t2 = t * t, s = sin(t), co = cos(t), h = 0.5 * t;
        c.a = s / t;
        c.b = (1.0 - co) / t2;
        c.c1 = (t - s) / (t2 * t);
        c.c2 = (t2 + 2.0 * co - 2.0) / (2.0 * t2 * t2);
        c.c3 = (2.0 * t - 3.0 * s + t * co) / (2.0 * t2 * t2 * t);
        c.ci = (1.0 - h * cos(h) / sin(h)) / t2;
    }
    return c;
}

__device__ __forceinline__ void hat(const double* v, double* K) {
    K[0] = 0.0, K[1] = -v[2], K[2] = v[1];
    K[3] = v[2], K[4] = 0.0, K[5] = -v[0];
    K[6] = -v[1], K[7] = v[0], K[8] = 0.0;
}
__device__ __forceinline__ void mm3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void mv3(const double* A, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}
__device__ __forceinline__ double norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// rigid poses as 12 doubles: rows of [R | t]
__device__ __forceinline__ void pose_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 4 + j] = (A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j]) + A[i * 4 + 2] * B[8 + j];
        C[i * 4 + 3] = ((A[i * 4] * B[3] + A[i * 4 + 1] * B[7]) + A[i * 4 + 2] * B[11]) + A[i * 4 + 3];
    }
}
__device__ __forceinline__ void pose_inv(const double* A, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 4 + j] = A[j * 4 + i];
        C[i * 4 + 3] = -((A[i] * A[3] + A[4 + i] * A[7]) + A[8 + i] * A[11]);
    }
}

// unit quaternion (x, y, z, w) of the rotation of a pose by the branch rule of the reference's mat2SO3 (its m = R^T)
__device__ void pose_quat(const double* T, double* q) {
#define PG_M(i, j) T[(j) * 4 + (i)]
    const double m00 = PG_M(0, 0), m01 = PG_M(0, 1), m02 = PG_M(0, 2), m10 = PG_M(1, 0), m11 = PG_M(1, 1), m12 = PG_M(1, 2), m20 = PG_M(2, 0),
                 m21 = PG_M(2, 1), m22 = PG_M(2, 2);
#undef PG_M
    double w, x, y, z, t;
    if (m22 < 1e-5) {
        if (m00 > m11) {
            t = 1 + m00 - m11 - m22, w = m12 - m21, x = t, y = m01 + m10, z = m20 + m02;
        } else {
            t = 1 - m00 + m11 - m22, w = m20 - m02, x = m01 + m10, y = t, z = m12 + m21;
        }
    } else {
        if (m00 < -m11) {
            t = 1 - m00 - m11 + m22, w = m01 - m10, x = m20 + m02, y = m12 + m21, z = t;
        } else {
            t = 1 + m00 + m11 + m22, w = t, x = m12 - m21, y = m20 - m02, z = m01 - m10;
        }
    }
    const double d = 2.0 * sqrt(t);
    w /= d, x /= d, y /= d, z /= d;
    const double n = sqrt(((w * w + x * x) + y * y) + z * z);
    q[0] = x / n, q[1] = y / n, q[2] = z / n, q[3] = w / n;
}

// mat2SE3 + .matrix(): the rotation through its unit quaternion, the translation as it is
__device__ void pose_project(const void* src, int f64, size_t idx, double* T) {
    double in[12];
    if (f64) {
        const double* p = (const double*)src + idx * 16;
#pragma unroll
        for (int i = 0; i < 12; ++i) in[i] = p[i];
    } else {
        const float* p = (const float*)src + idx * 16;
#pragma unroll
        for (int i = 0; i < 12; ++i) in[i] = (double)p[i];
    }
    double q[4];
    pose_quat(in, q);
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    T[0] = 1 - 2 * (y * y + z * z), T[1] = 2 * (x * y - z * w), T[2] = 2 * (x * z + y * w), T[3] = in[3];
    T[4] = 2 * (x * y + z * w), T[5] = 1 - 2 * (x * x + z * z), T[6] = 2 * (y * z - x * w), T[7] = in[7];
    T[8] = 2 * (x * z - y * w), T[9] = 2 * (y * z + x * w), T[10] = 1 - 2 * (x * x + y * y), T[11] = in[11];
}

// xi = Log(T) = (V^-1 t, phi)
__device__ void se3_log(const double* T, double* xi) {
    double q[4];
    pose_quat(T, q);
    if (q[3] < 0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
    const double n = norm3(q), w = q[3];
    double f;
    if (n < PG_SMALL_QUAT) {
        const double u = (n / w) * (n / w);
        f = (2.0 / w) * (1.0 + u * (-1.0 / 3 + u * (1.0 / 5 + u * (-1.0 / 7))));
    } else {
        f = 2.0 * atan2(n, w) / n;
    }
    double phi[3] = {q[0] * f, q[1] * f, q[2] * f};
    const Coef c = coefficients(norm3(phi));
    double K[9], K2[9], Vi[9];
    hat(phi, K);
    mm3(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) Vi[i] = ((i % 4 == 0 ? 1.0 : 0.0) - 0.5 * K[i]) + c.ci * K2[i];
    const double t[3] = {T[3], T[7], T[11]};
    mv3(Vi, t, xi);
    xi[3] = phi[0], xi[4] = phi[1], xi[5] = phi[2];
}

// X <- Exp(xi) X
__device__ void pose_update(const double* xi, double* X) {
    const double* phi = xi + 3;
    const Coef c = coefficients(norm3(phi));
    double K[9], K2[9], E[12], V[9], tv[3];
    hat(phi, K);
    mm3(K, K, K2);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            E[i * 4 + j] = (id + c.a * K[i * 3 + j]) + c.b * K2[i * 3 + j];
            V[i * 3 + j] = (id + c.b * K[i * 3 + j]) + c.c1 * K2[i * 3 + j];
        }
    mv3(V, xi, tv);
    E[3] = tv[0], E[7] = tv[1], E[11] = tv[2];
    double out[12];
    pose_mul(E, X, out);
#pragma unroll
    for (int i = 0; i < 12; ++i) X[i] = out[i];
}

// One edge: r = w Log(P Xa^-1 Xb) -> sum r^2; with `rec` also the record [r 6 | g = G^T r 6 | S 9 | U 9 | M = G^T G 36], where
// G = w Jl^-1(xi) Ad(P Xa^-1) = [[S, U], [0, S]] is d r / d delta_b (and minus d r / d delta_a).
__device__ double edge_residual(const double* P, const double* Xa, const double* Xb, double w, double* rec) {
    double Ai[12], A[12], E[12], xi[6], r[6];
    pose_inv(Xa, Ai);
    pose_mul(P, Ai, A);
    pose_mul(A, Xb, E);
    se3_log(E, xi);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        r[k] = w * xi[k];
        sum += r[k] * r[k];
    }
    if (rec == nullptr) return sum;
    const double *tau = xi, *phi = xi + 3;
    const Coef c = coefficients(norm3(phi));
    double Ph[9], Th[9], PT[9], TP[9], PP[9], PTP[9], PPT[9], TPP[9], PTPP[9], PPTP[9], Q[9], Ji[9];
    hat(phi, Ph), hat(tau, Th);
    mm3(Ph, Th, PT), mm3(Th, Ph, TP), mm3(Ph, Ph, PP);
    mm3(PT, Ph, PTP), mm3(PP, Th, PPT), mm3(Th, PP, TPP), mm3(PTP, Ph, PTPP), mm3(Ph, PTP, PPTP);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Q[i] = ((0.5 * Th[i] + c.c1 * ((PT[i] + TP[i]) + PTP[i])) + c.c2 * ((PPT[i] + TPP[i]) - 3.0 * PTP[i])) + c.c3 * (PTPP[i] + PPTP[i]);
        Ji[i] = ((i % 4 == 0 ? 1.0 : 0.0) - 0.5 * Ph[i]) + c.ci * PP[i];
    }
    double JQ[9], B[9], R[9], tR[9], th[9], S[9], U1[9], U2[9], U[9];
    mm3(Ji, Q, JQ);
    mm3(JQ, Ji, B);                                         // the block is -B
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = A[i * 4 + j];
    const double t[3] = {A[3], A[7], A[11]};
    hat(t, th);
    mm3(th, R, tR);
    mm3(Ji, R, S), mm3(Ji, tR, U1), mm3(B, R, U2);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        U[i] = w * (U1[i] - U2[i]);
        S[i] = w * S[i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[k] = r[k];
    // g = G^T r = [S^T r_t ; U^T r_t + S^T r_p]
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        rec[6 + j] = (S[j] * r[0] + S[3 + j] * r[1]) + S[6 + j] * r[2];
        rec[9 + j] = ((((U[j] * r[0] + U[3 + j] * r[1]) + U[6 + j] * r[2]) + S[j] * r[3]) + S[3 + j] * r[4]) + S[6 + j] * r[5];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) rec[12 + i] = S[i], rec[21 + i] = U[i];
    // M = G^T G = [[S^T S, S^T U], [U^T S, U^T U + S^T S]]
    double* M = rec + 30;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double ss = (S[i] * S[j] + S[3 + i] * S[3 + j]) + S[6 + i] * S[6 + j];
            const double su = (S[i] * U[j] + S[3 + i] * U[3 + j]) + S[6 + i] * U[6 + j];
            const double uu = (U[i] * U[j] + U[3 + i] * U[3 + j]) + U[6 + i] * U[6 + j];
            M[i * 6 + j] = ss;
            M[i * 6 + 3 + j] = su;
            M[(3 + j) * 6 + i] = su;
            M[(3 + i) * 6 + 3 + j] = uu + ss;
        }
    return sum;
}

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }

__global__ __launch_bounds__(PG_TPB) void posegraph_kernel(const PgCfg c) {
    __shared__ double s_tri[PG_LDS_TRI];
    __shared__ double s_b[PG_MAX_N], s_x[PG_MAX_N], s_dg[PG_MAX_N];
    __shared__ double s_red[PG_WAVES];
    __shared__ int s_flag;
    __shared__ uint8_t s_ea[PG_MAX_EDGES], s_eb[PG_MAX_EDGES];

    const int tid = threadIdx.x, wave = tid / MIPSF_WAVE, lane = tid % MIPSF_WAVE, N = c.n_nodes, E = c.n_edges, n = 6 * (N - 1);
    double* X = c.ws + WS_X;
    double* Xs = c.ws + WS_SAVE;
    double* P = c.ws + WS_P;
    double* rec = c.ws + WS_REC;
    double* A = N <= (int)MIPSF_POSEGRAPH_LDS_NODES ? s_tri : c.ws + ws_tri(E);

    // ---- projection, edge table, refusal of a malformed edge
    if (tid == 0) s_flag = 0;
    __syncthreads();
    for (int i = tid; i < N; i += PG_TPB) pose_project(c.anchors, c.input_f64, i, X + i * 12);
    for (int e = tid; e < E; e += PG_TPB) {
        pose_project(c.observations, c.input_f64, e, P + e * 12);
        const int a = c.edges[2 * e], b = c.edges[2 * e + 1];
        const bool ok = a >= 0 && a < N && b >= 0 && b < N && a != b;
        if (!ok) s_flag = 1;
        s_ea[e] = (uint8_t)(ok ? a : 0);
        s_eb[e] = (uint8_t)(ok ? b : 0);
    }
    __syncthreads();
    const bool bad_edge = s_flag != 0;
    __syncthreads();

    auto total_loss = [&](bool record) {
        double v = 0.0;
        for (int e = tid; e < E; e += PG_TPB)
            v += edge_residual(P + e * 12, X + s_ea[e] * 12, X + s_eb[e] * 12, c.weights[e], record ? rec + (size_t)e * PG_EDGE_DOUBLES : nullptr);
        return block_reduce<PG_WAVES>(v, s_red, Add());
    };
    // J^T J without its diagonal (-> A), b = -J^T r (-> s_b, which the solve then consumes) and, with `first`, the clamped diagonal
    // (-> s_dg); one 6x6 block per lane, the edges of a block in ascending index
    auto assemble = [&](bool first) {
        const int blocks = (N - 1) * N / 2;
        for (int blk = tid; blk < blocks; blk += PG_TPB) {
            int p = 0;
            while (tri(p + 1) <= blk) ++p;
            const int q = blk - tri(p), np = p + 1, nq = q + 1;         // block (p, q), q <= p, of nodes np, nq
            double acc[36], g[6];
#pragma unroll
            for (int i = 0; i < 36; ++i) acc[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = 0.0;
            for (int e = 0; e < E; ++e) {
                const int a = s_ea[e], b = s_eb[e];
                const double* r = rec + (size_t)e * PG_EDGE_DOUBLES;
                if (p == q) {
                    if (a != np && b != np) continue;
#pragma unroll
                    for (int i = 0; i < 36; ++i) acc[i] += r[30 + i];
#pragma unroll
                    for (int i = 0; i < 6; ++i) g[i] = b == np ? g[i] - r[6 + i] : g[i] + r[6 + i];
                } else {
                    if (!((a == np && b == nq) || (a == nq && b == np))) continue;
#pragma unroll
                    for (int i = 0; i < 36; ++i) acc[i] -= r[30 + i];
                }
            }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                double* row = A + tri(6 * p + u) + 6 * q;
#pragma unroll
                for (int v = 0; v < 6; ++v)
                    if (p != q || v < u) row[v] = acc[u * 6 + v];
                if (p == q) {
                    if (first) s_dg[6 * p + u] = fmin(fmax(acc[u * 6 + u], c.min_diag), PG_MAX_DIAG);
                    s_b[6 * p + u] = g[u];
                }
            }
        }
        __syncthreads();
    };

    double radius = c.radius, down = 0.5, damping = 1.0 / radius;
    double loss = 0.0, first_loss = 0.0;
    int done = 0, solves = 0, rejections = 0, plateau = 0;
    unsigned status = 0;
    if (bad_edge) {
        status = MIPSF_POSEGRAPH_BAD_EDGE;
    } else {
        loss = first_loss = total_loss(false);
        for (int step = 0; step < c.steps; ++step) {
            const double last = loss;
            total_loss(true);
            assemble(true);
            int rejects = 0;
            while (true) {
                // ---- damp (cumulative over rejections), then A = L L^T in place, right-looking: column j is scaled, copied to LDS
                // (s_x) and taken out of the trailing triangle, whose rows are contiguous, so a wave reads and writes whole
                // lines and PG_BATCH loads are in flight per lane.  Element (i, k) loses L_ij L_kj for j ascending: the order of
                // the textbook inner-product form.  L y = b rides along (y_j = b_j / L_jj as soon as column j is final).
                for (int i = tid; i < n; i += PG_TPB) {
                    const double d = s_dg[i] + s_dg[i] * damping;
                    s_dg[i] = d;
                    A[tri(i) + i] = d;
                }
                __syncthreads();
                ++solves;
                bool failed = false;
                for (int j = 0; j < n; ++j) {
                    const double djj = A[tri(j) + j];               // the same value in every lane: the branch is uniform
                    if (!(djj > 0.0) || !(djj < INFINITY)) {
                        failed = true;
                        break;
                    }
                    const double piv = sqrt(djj), yj = s_b[j] / piv;
                    for (int i = j + 1 + tid; i < n; i += PG_TPB) {
                        const double v = A[tri(i) + j] / piv;
                        A[tri(i) + j] = v;
                        s_x[i] = v;
                        s_b[i] -= v * yj;
                    }
                    __syncthreads();
                    if (tid == 0) {
                        A[tri(j) + j] = piv;
                        s_b[j] = yj;
                    }
                    for (int r0 = j + 1 + wave; r0 < n; r0 += PG_WAVES * PG_BATCH) {
                        const int r_last = min(n - 1, r0 + PG_WAVES * (PG_BATCH - 1));
                        for (int k = j + 1 + lane; k <= r_last; k += MIPSF_WAVE) {
                            const double lk = s_x[k];
                            double a[PG_BATCH];
#pragma unroll
                            for (int u = 0; u < PG_BATCH; ++u) {
                                const int r = r0 + PG_WAVES * u;
                                if (r < n && k <= r) a[u] = A[tri(r) + k];
                            }
#pragma unroll
                            for (int u = 0; u < PG_BATCH; ++u) {
                                const int r = r0 + PG_WAVES * u;
                                if (r < n && k <= r) A[tri(r) + k] = a[u] - s_x[r] * lk;
                            }
                        }
                    }
                    __syncthreads();
                }
                if (failed) {
                    status |= MIPSF_POSEGRAPH_FACTORISATION_FAILED;
                    __syncthreads();
                    break;
                }
                // ---- L^T D = y in place (s_b): row i belongs to lane i % PG_TPB until it is final
                for (int j = n - 1; j >= 0; --j) {
                    if (tid == j % PG_TPB) s_b[j] /= A[tri(j) + j];
                    __syncthreads();
                    const double xj = s_b[j];
                    const double* Lj = A + tri(j);
                    for (int i = tid; i < j; i += PG_TPB) s_b[i] -= Lj[i] * xj;
                }
                if (tid == 0) s_flag = 0;
                __syncthreads();
                // a step that is not finite counts as a failed factorisation (the restatement's rule)
                {
                    int nf = 0;
                    for (int i = tid; i < n; i += PG_TPB) nf |= !(fabs(s_b[i]) < INFINITY);
                    if (nf) s_flag = 1;
                    __syncthreads();
                    if (s_flag) {
                        status |= MIPSF_POSEGRAPH_FACTORISATION_FAILED;
                        __syncthreads();
                        break;
                    }
                }
                // ---- X_i <- Exp(D_i) X_i, the new loss, the quality of the step
                for (int i = 1 + tid; i < N; i += PG_TPB) {
                    double T[12], xi[6];
#pragma unroll
                    for (int k = 0; k < 12; ++k) Xs[i * 12 + k] = T[k] = X[i * 12 + k];
#pragma unroll
                    for (int k = 0; k < 6; ++k) xi[k] = s_b[6 * (i - 1) + k];
                    pose_update(xi, T);
#pragma unroll
                    for (int k = 0; k < 12; ++k) X[i * 12 + k] = T[k];
                }
                __syncthreads();
                loss = total_loss(false);
                double v = 0.0;
                for (int e = tid; e < E; e += PG_TPB) {
                    const double* r = rec + (size_t)e * PG_EDGE_DOUBLES;
                    const double *S = r + 12, *U = r + 21;
                    const int a = s_ea[e], b = s_eb[e];
                    double d[6], u[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = (b > 0 ? s_b[6 * (b - 1) + k] : 0.0) - (a > 0 ? s_b[6 * (a - 1) + k] : 0.0);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        u[i] = ((((S[i * 3] * d[0] + S[i * 3 + 1] * d[1]) + S[i * 3 + 2] * d[2]) + U[i * 3] * d[3]) + U[i * 3 + 1] * d[4]) + U[i * 3 + 2] * d[5];
                        u[3 + i] = (S[i * 3] * d[3] + S[i * 3 + 1] * d[4]) + S[i * 3 + 2] * d[5];
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) v += u[k] * (2.0 * r[k] + u[k]);
                }
                const double den = -block_reduce<PG_WAVES>(v, s_red, Add());
                const double quality = (last - loss) / den;
                if (quality > 0.5) {
                    radius *= 2.0, down = 0.5;
                } else if (quality > 1e-3) {
                    down = 0.5;
                } else {
                    if (quality != quality) status |= MIPSF_POSEGRAPH_NAN_QUALITY;
                    radius *= down, down *= 0.5;
                }
                damping = 1.0 / radius;
                if (last < loss && rejects < c.max_rejects) {
                    for (int i = 12 + tid; i < N * 12; i += PG_TPB) X[i] = Xs[i];
                    loss = last, ++rejects, ++rejections;
                    __syncthreads();
                    assemble(false);                        // the solve overwrote A and b: both again, the damped diagonal is s_dg
                    continue;
                }
                break;
            }
            ++done;
            plateau = (last - loss < c.decreasing) ? plateau + 1 : 0;
            if (plateau >= c.patience) break;
        }
    }
    __syncthreads();
    for (int i = tid; i < N * 16; i += PG_TPB) {
        const int node = i / 16, k = i % 16;
        const double v = k < 12 ? X[node * 12 + k] : (k == 15 ? 1.0 : 0.0);
        c.out64[i] = v;
        c.out32[i] = (float)v;
    }
    if (tid == 0) {
        c.result[0] = first_loss, c.result[1] = loss, c.result[2] = (double)done, c.result[3] = (double)solves;
        c.result[4] = (double)rejections, c.result[5] = radius, c.result[6] = (double)status, c.result[7] = 0.0;
    }
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" uint64_t mipsf_posegraph_workspace_bytes(uint32_t n_nodes, uint32_t n_edges) {
    if (n_nodes < 2 || n_nodes > MIPSF_POSEGRAPH_MAX_NODES || n_edges < 1 || n_edges > MIPSF_POSEGRAPH_MAX_EDGES) return 0;
    const uint64_t n = 6ull * (n_nodes - 1);
    return (ws_tri(n_edges) + (n_nodes > MIPSF_POSEGRAPH_LDS_NODES ? n * (n + 1) / 2 : 0)) * sizeof(double);
}

extern "C" int mipsf_posegraph_optimize(const mipsf_posegraph_args* a, void* stream) {
    MIPSF_ARGS(a, mipsf_posegraph_args, "mipsf_posegraph_optimize");
    MIPSF_REQUIRE(a->n_nodes >= 2 && a->n_nodes <= MIPSF_POSEGRAPH_MAX_NODES, "mipsf_posegraph_optimize: %u nodes, accepted are 2 .. %u", a->n_nodes,
                  MIPSF_POSEGRAPH_MAX_NODES);
    MIPSF_REQUIRE(a->n_edges >= 1 && a->n_edges <= MIPSF_POSEGRAPH_MAX_EDGES, "mipsf_posegraph_optimize: %u edges, accepted are 1 .. %u", a->n_edges,
                  MIPSF_POSEGRAPH_MAX_EDGES);
    MIPSF_REQUIRE(a->anchors && a->edges && a->observations && a->weights && a->anchors_out && a->anchors_out32 && a->result && a->workspace,
                  "mipsf_posegraph_optimize: null pointer");
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 15u) == 0, "mipsf_posegraph_optimize: workspace not 16-byte aligned");
    MIPSF_REQUIRE(a->input_f64 <= 1, "mipsf_posegraph_optimize: input_f64 %u", a->input_f64);
    MIPSF_REQUIRE(a->steps <= 1000 && a->max_rejects <= 1000, "mipsf_posegraph_optimize: steps %u / max_rejects %u above 1000", a->steps, a->max_rejects);
    MIPSF_REQUIRE(a->radius > 0.0 && a->radius < INFINITY && a->min_diag > 0.0 && a->min_diag <= PG_MAX_DIAG && a->decreasing == a->decreasing,
                  "mipsf_posegraph_optimize: radius %g, min_diag %g, decreasing %g", a->radius, a->min_diag, a->decreasing);
    PgCfg c;
    c.anchors = a->anchors, c.edges = a->edges, c.observations = a->observations, c.weights = a->weights;
    c.n_nodes = (int)a->n_nodes, c.n_edges = (int)a->n_edges, c.input_f64 = (int)a->input_f64;
    c.steps = (int)a->steps, c.patience = (int)a->patience, c.max_rejects = (int)a->max_rejects;
    c.decreasing = a->decreasing, c.radius = a->radius, c.min_diag = a->min_diag;
    c.out64 = a->anchors_out, c.out32 = a->anchors_out32, c.result = a->result, c.ws = (double*)a->workspace;
    hipLaunchKernelGGL(posegraph_kernel, dim3(1), dim3(PG_TPB), 0, (hipStream_t)stream, c);
    return check_launch("posegraph_optimize");
}
