// Sub-map management, the geometry (include/mipsf_submap.h; restated by tests/submap_cpu.py):
//   mipsf_submap_frame_stats   two launches: partial surface boxes of the frame, then one workgroup per sub-map
//   mipsf_submap_overlap       two launches: centre distances of the related keyframes, then the overlap masks
// No atomics anywhere: every count is a tree over a workgroup, the surface box goes through at most 256 per-workgroup partials
// that every workgroup of the second launch folds again for itself.
#include "block_dev.h"
#include "../../include/mipsf_submap.h"
#include "submap_dev.h"

namespace mipsf {
namespace {

constexpr int SM_TPB = 256;              // threads of every workgroup but the mask kernel's
constexpr int SM_WAVES = SM_TPB / MIPSF_WAVE;
constexpr int SM_PARTIALS = 256;         // workgroups of the surface-box launch at most; == SM_TPB, one thread folds one partial
constexpr int SM_MASK_TPB = 1024;

struct Lattice {                         // sample_pixels_uniformly: row i -> i * step_h + first_h, column j -> j * step_w + first_w
    uint32_t nh, nw, step_h, first_h, step_w, first_w;
};

inline Lattice make_lattice(uint32_t H, uint32_t W, uint32_t nh, uint32_t nw) {
    Lattice l;
    const uint32_t ih = (H - nh) / (nh + 1), oh = (H - nh) % (nh + 1);
    const uint32_t iw = (W - nw) / (nw + 1), ow = (W - nw) % (nw + 1);
    l.nh = nh, l.nw = nw, l.step_h = ih + 1, l.first_h = ih + oh / 2, l.step_w = iw + 1, l.first_w = iw + ow / 2;
    return l;
}

__device__ __forceinline__ uint32_t lattice_pixel(const Lattice& l, uint32_t q, uint32_t W) {
    const uint32_t i = q / l.nw, j = q - i * l.nw;
    return (i * l.step_h + l.first_h) * W + (j * l.step_w + l.first_w);
}

struct Pose {
    float R[9], t[3];
};

__device__ __forceinline__ Pose load_pose(const float* __restrict__ m) {
    Pose p;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p.R[i * 3 + 0] = m[i * 4 + 0], p.R[i * 3 + 1] = m[i * 4 + 1], p.R[i * 3 + 2] = m[i * 4 + 2];
        p.t[i] = m[i * 4 + 3];
    }
    return p;
}

// p = t + (R d) * depth in float32, the order of mipsf_submap.h
__device__ __forceinline__ void world_point(const Pose& P, const float* __restrict__ row, float p[3]) {
    const float x = row[0], y = row[1], z = row[2], d = row[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float dw = (x * P.R[i * 3 + 0] + y * P.R[i * 3 + 1]) + z * P.R[i * 3 + 2];
        p[i] = P.t[i] + dw * d;
    }
}

__device__ __forceinline__ float min32(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max32(float a, float b) { return b > a ? b : a; }

// the operators of the workgroup trees (block_dev.h); a NaN in b never wins
struct Min32 {
    __device__ __forceinline__ float operator()(float a, float b) const { return min32(a, b); }
};
struct Max32 {
    __device__ __forceinline__ float operator()(float a, float b) const { return max32(a, b); }
};

// sum over a lattice's points: thread t adds points t, t + 256, .. in that order, then block_reduce (the float64 order
// tests/submap_cpu.py spells out: butterfly 32, 16, .. 1 inside a wave, then the waves in ascending order).  SM_TPB threads.
__device__ __forceinline__ void lattice_sum(const Lattice& l, uint32_t W, const float* __restrict__ rows, const Pose& P, double* s,
                                            double out[3]) {
    double acc[3] = {0.0, 0.0, 0.0};
    const uint32_t n = l.nh * l.nw;
    for (uint32_t q = threadIdx.x; q < n; q += SM_TPB) {
        float p[3];
        world_point(P, rows + (size_t)lattice_pixel(l, q, W) * 7, p);
        acc[0] = acc[0] + (double)p[0], acc[1] = acc[1] + (double)p[1], acc[2] = acc[2] + (double)p[2];
    }
    for (int a = 0; a < 3; ++a) out[a] = block_reduce<SM_WAVES>(acc[a], s, Add());
}

// ------------------------------------------------------------------------------------------------ frame statistics, launch 1
// partial[b] = {min x y z, max x y z, count, 0} over the pixels workgroup b strides through
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(SM_TPB) void submap_surface_kernel(const float* __restrict__ rows, const float* __restrict__ pose,
                                                                                  uint32_t n_pix, float near, float far,
                                                                                  uint32_t* __restrict__ partial) {
    __shared__ float s_f[SM_WAVES];
    __shared__ uint32_t s_u[SM_WAVES];
    const Pose P = load_pose(pose);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t count = 0;
    for (uint32_t i = blockIdx.x * SM_TPB + threadIdx.x; i < n_pix; i += gridDim.x * SM_TPB) {
        const float* row = rows + (size_t)i * 7;
        const float d = row[6];
        if (d > near && d < far) {
            float p[3];
            world_point(P, row, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = min32(lo[a], p[a]), hi[a] = max32(hi[a], p[a]);
            ++count;
        }
    }
    uint32_t* out = partial + (size_t)blockIdx.x * 8;
    for (int a = 0; a < 3; ++a) {
        const float m = block_reduce<SM_WAVES>(lo[a], s_f, Min32());
        const float M = block_reduce<SM_WAVES>(hi[a], s_f, Max32());
        if (threadIdx.x == 0) out[a] = __float_as_uint(m), out[3 + a] = __float_as_uint(M);
    }
    const uint32_t c = block_reduce<SM_WAVES>(count, s_u, Add());
    if (threadIdx.x == 0) out[6] = c, out[7] = 0u;
}

struct StatsCfg {
    const float* rows;
    const float* pose;
    const float* boxes;
    const float* max_len;
    const uint32_t* partial;
    uint32_t* record;
    uint32_t W, n_partials, n_boxes;
    float min_cr_len[3];
    Lattice A, B, C;
};

// ------------------------------------------------------------------------------------------------ frame statistics, launch 2
// workgroup i: sub-map i.  Every workgroup folds the partial surface boxes for itself; workgroup 0 also writes the header.
MIPSF_SINGLE_FP32 __global__ __launch_bounds__(SM_TPB) void submap_stats_kernel(StatsCfg c) {
    __shared__ float s_f[SM_WAVES];
    __shared__ uint32_t s_u[SM_WAVES];
    __shared__ double s_d[SM_WAVES];
    __shared__ float s_box[12];          // expanded centre, length; clamped length; (raw comes from global)
    __shared__ uint32_t s_cases;
    const uint32_t tid = threadIdx.x, box = blockIdx.x;
    const Pose P = load_pose(c.pose);

    float lo[3], hi[3];
    const bool have = tid < c.n_partials;
    const uint32_t* part = c.partial + (size_t)(have ? tid : 0) * 8;
    for (int a = 0; a < 3; ++a) {
        lo[a] = block_reduce<SM_WAVES>(have ? __uint_as_float(part[a]) : INFINITY, s_f, Min32());
        hi[a] = block_reduce<SM_WAVES>(have ? __uint_as_float(part[3 + a]) : -INFINITY, s_f, Max32());
    }
    const uint32_t n_valid = block_reduce<SM_WAVES>(have ? part[6] : 0u, s_u, Add());

    float bc[3], bl[3];
    for (int a = 0; a < 3; ++a) bc[a] = c.boxes[box * 6 + a], bl[a] = c.boxes[box * 6 + 3 + a];
    if (tid == 0) {
        float kc[3], kl[3], mx[3], oc[3], ol[3];
        for (int a = 0; a < 3; ++a) {                      // get_frame_surface_bbox: len = max - min, centre = min + 0.5 len
            kl[a] = hi[a] - lo[a];
            kc[a] = lo[a] + 0.5f * kl[a];
            mx[a] = c.max_len[box * 3 + a];
        }
        s_cases = submap::expand_rule(bc, bl, kc, kl, mx, oc, ol);
        for (int a = 0; a < 3; ++a) {
            s_box[a] = oc[a], s_box[3 + a] = ol[a];
            s_box[6 + a] = bl[a] < c.min_cr_len[a] ? c.min_cr_len[a] : bl[a];
        }
    }
    __syncthreads();
    float ec[3], el[3], cl[3];
    for (int a = 0; a < 3; ++a) ec[a] = s_box[a], el[a] = s_box[3 + a], cl[a] = s_box[6 + a];

    uint32_t a_valid = 0, a_clamped = 0, a_expanded = 0, b_raw = 0;
    const uint32_t nA = c.A.nh * c.A.nw, nB = c.B.nh * c.B.nw;
    for (uint32_t q = tid; q < nA; q += SM_TPB) {
        const float* row = c.rows + (size_t)lattice_pixel(c.A, q, c.W) * 7;
        if (row[6] > 0.0f) {
            float p[3];
            world_point(P, row, p);
            ++a_valid;
            a_clamped += submap::inside(p, bc, cl) ? 1u : 0u;
            a_expanded += submap::inside(p, ec, el) ? 1u : 0u;
        }
    }
    for (uint32_t q = tid; q < nB; q += SM_TPB) {
        float p[3];
        world_point(P, c.rows + (size_t)lattice_pixel(c.B, q, c.W) * 7, p);
        b_raw += submap::inside(p, bc, bl) ? 1u : 0u;
    }
    a_valid = block_reduce<SM_WAVES>(a_valid, s_u, Add());
    a_clamped = block_reduce<SM_WAVES>(a_clamped, s_u, Add());
    a_expanded = block_reduce<SM_WAVES>(a_expanded, s_u, Add());
    b_raw = block_reduce<SM_WAVES>(b_raw, s_u, Add());

    uint32_t* out = c.record + MIPSF_SUBMAP_HEADER_WORDS + (size_t)box * MIPSF_SUBMAP_BOX_WORDS;
    if (tid == 0) {
        for (int a = 0; a < 3; ++a) out[a] = __float_as_uint(ec[a]), out[3 + a] = __float_as_uint(el[a]);
        out[6] = a_clamped, out[7] = a_expanded, out[8] = b_raw, out[9] = s_cases, out[10] = 0u, out[11] = 0u;
    }
    if (box == 0) {
        double sum[3];
        lattice_sum(c.C, c.W, c.rows, P, s_d, sum);
        if (tid == 0) {
            uint32_t* h = c.record;
            h[0] = n_valid;
            for (int a = 0; a < 3; ++a) h[1 + a] = __float_as_uint(lo[a]), h[4 + a] = __float_as_uint(hi[a]);
            h[7] = a_valid;
            double* d = reinterpret_cast<double*>(h + 8);
            d[0] = sum[0], d[1] = sum[1], d[2] = sum[2];
            h[14] = c.n_boxes, h[15] = 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ overlap, phase (a)
struct DistCfg {
    const float* rows;
    const float* pose;
    const float* table;
    const int32_t* slots;
    const float* poses;
    double* dist;
    uint32_t W, n_slots, rows_per_slot;
    Lattice C;
};

MIPSF_SINGLE_FP32 __global__ __launch_bounds__(SM_TPB) void submap_dist_kernel(DistCfg c) {
    __shared__ double s_d[SM_WAVES];
    const Pose P = load_pose(c.pose);
    double centre[3];
    lattice_sum(c.C, c.W, c.rows, P, s_d, centre);
    const double n = (double)(c.C.nh * c.C.nw);
    for (int a = 0; a < 3; ++a) centre[a] = centre[a] / n;

    const int32_t slot = c.slots[blockIdx.x];
    if (slot < 0 || (uint32_t)slot >= c.n_slots) {         // uniform over the workgroup
        if (threadIdx.x == 0) c.dist[blockIdx.x] = (double)NAN;
        return;
    }
    const float* kf = c.table + (size_t)slot * c.rows_per_slot * 7;
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t r = threadIdx.x; r < c.rows_per_slot; r += SM_TPB) {
        const float* row = kf + (size_t)r * 7;
        const float d = row[6];
        acc[0] = acc[0] + (double)(row[0] * d), acc[1] = acc[1] + (double)(row[1] * d), acc[2] = acc[2] + (double)(row[2] * d);
    }
    double m[3];
    for (int a = 0; a < 3; ++a) m[a] = block_reduce<SM_WAVES>(acc[a], s_d, Add()) / (double)c.rows_per_slot;
    if (threadIdx.x == 0) {
        const float* M = c.poses + (size_t)blockIdx.x * 16;
        double q = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double w = ((m[0] * (double)M[i * 4 + 0] + m[1] * (double)M[i * 4 + 1]) + m[2] * (double)M[i * 4 + 2]) + (double)M[i * 4 + 3];
            const double e = w - centre[i];
            q = q + e * e;
        }
        c.dist[blockIdx.x] = sqrt(q);
    }
}

// ------------------------------------------------------------------------------------------------ overlap, phase (b)
struct MaskCfg {
    const float* rows;
    const float* pose;
    const float* top_poses;
    uint8_t* top_kf_masks;
    uint8_t* mask_final;
    uint32_t* count;
    float* target_d;
    float* rays_d_cam;
    uint32_t W, k;
    double fx, fy, cx, cy, u_hi, v_hi, edge;
    float box[6];
    Lattice C;
};

MIPSF_SINGLE_FP32 __global__ __launch_bounds__(SM_MASK_TPB) void submap_mask_kernel(MaskCfg c) {
    __shared__ double s_w2c[MIPSF_SUBMAP_MAX_TOP_KF][12];   // rigid inverse: R^T (9), -(R^T t) (3)
    __shared__ uint32_t s_u[SM_MASK_TPB / MIPSF_WAVE];
    const uint32_t tid = threadIdx.x;
    if (tid < c.k) {
        const float* M = c.top_poses + (size_t)tid * 16;
        double* o = s_w2c[tid];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o[i * 3 + j] = (double)M[j * 4 + i];
            o[9 + i] = -(((double)M[0 * 4 + i] * (double)M[3] + (double)M[1 * 4 + i] * (double)M[7]) + (double)M[2 * 4 + i] * (double)M[11]);
        }
    }
    __syncthreads();
    const Pose P = load_pose(c.pose);
    const uint32_t n = c.C.nh * c.C.nw;
    const float bc[3] = {c.box[0], c.box[1], c.box[2]}, bl[3] = {c.box[3], c.box[4], c.box[5]};
    uint32_t count = 0;
    for (uint32_t q = tid; q < n; q += SM_MASK_TPB) {
        const float* row = c.rows + (size_t)lattice_pixel(c.C, q, c.W) * 7;
        float p[3];
        world_point(P, row, p);
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        bool any = false;
        for (uint32_t kk = 0; kk < c.k; ++kk) {
            const double* o = s_w2c[kk];
            const double xc = ((o[0] * x + o[1] * y) + o[2] * z) + o[9];
            const double yc = ((o[3] * x + o[4] * y) + o[5] * z) + o[10];
            const double zc = ((o[6] * x + o[7] * y) + o[8] * z) + o[11];
            const double zz = zc + 1e-5;
            const double u = (c.fx * (-xc) + c.cx * zc) / zz;
            const double v = (c.fy * yc + c.cy * zc) / zz;
            const bool seen = u < c.u_hi && u > c.edge && v < c.v_hi && v > c.edge && zc < 0.0;
            c.top_kf_masks[(size_t)kk * n + q] = seen ? 1 : 0;
            any = any || seen;
        }
        const bool fin = any && submap::inside(p, bc, bl);
        c.mask_final[q] = fin ? 1 : 0;
        count += fin ? 1u : 0u;
        c.target_d[q] = row[6];
        c.rays_d_cam[q * 3 + 0] = row[0], c.rays_d_cam[q * 3 + 1] = row[1], c.rays_d_cam[q * 3 + 2] = row[2];
    }
    count = block_reduce<SM_MASK_TPB / MIPSF_WAVE>(count, s_u, Add());
    if (tid == 0) c.count[0] = count;
}

int check_lattice(const char* who, const char* name, uint32_t H, uint32_t W, uint32_t nh, uint32_t nw) {
    MIPSF_REQUIRE(nh >= 1 && nw >= 1 && nh <= H && nw <= W, "%s: lattice %s is %u x %u, the image is %u x %u", who, name, nh, nw, H, W);
    return 0;
}

}  // namespace
}  // namespace mipsf

using namespace mipsf;

extern "C" int mipsf_submap_frame_stats(const mipsf_submap_frame_stats_args* a, void* stream) {
    static const char* who = "mipsf_submap_frame_stats";
    MIPSF_ARGS(a, mipsf_submap_frame_stats_args, who);
    MIPSF_REQUIRE(a->H >= 1 && a->W >= 1 && (uint64_t)a->H * a->W <= (1ull << 28), "%s: image %u x %u", who, a->H, a->W);
    MIPSF_REQUIRE(a->n_boxes >= 1 && a->n_boxes <= MIPSF_SUBMAP_MAX_BOXES, "%s: %u sub-maps, accepted are 1 .. %u", who, a->n_boxes,
                  MIPSF_SUBMAP_MAX_BOXES);
    if (check_lattice(who, "A", a->H, a->W, a->lat_a_h, a->lat_a_w) || check_lattice(who, "B", a->H, a->W, a->lat_b_h, a->lat_b_w) ||
        check_lattice(who, "C", a->H, a->W, a->lat_c_h, a->lat_c_w))
        return 1;
    MIPSF_REQUIRE(a->rows && a->pose && a->boxes && a->max_len && a->record && a->workspace, "%s: null pointer", who);
    MIPSF_REQUIRE(((uintptr_t)a->workspace & 7u) == 0 && ((uintptr_t)a->record & 7u) == 0, "%s: record / workspace not 8-byte aligned", who);
    const uint32_t n_pix = a->H * a->W;
    const uint32_t blocks = (n_pix + SM_TPB - 1) / SM_TPB < (uint32_t)SM_PARTIALS ? (n_pix + SM_TPB - 1) / SM_TPB : (uint32_t)SM_PARTIALS;
    uint32_t* partial = (uint32_t*)a->workspace;
    hipLaunchKernelGGL(submap_surface_kernel, dim3(blocks), dim3(SM_TPB), 0, (hipStream_t)stream, a->rows, a->pose, n_pix, a->near, a->far, partial);
    if (check_launch("submap_frame_stats (surface box)")) return 1;
    StatsCfg c;
    c.rows = a->rows, c.pose = a->pose, c.boxes = a->boxes, c.max_len = a->max_len, c.partial = partial, c.record = a->record;
    c.W = a->W, c.n_partials = blocks, c.n_boxes = a->n_boxes;
    for (int i = 0; i < 3; ++i) c.min_cr_len[i] = a->min_cr_len[i];
    c.A = make_lattice(a->H, a->W, a->lat_a_h, a->lat_a_w);
    c.B = make_lattice(a->H, a->W, a->lat_b_h, a->lat_b_w);
    c.C = make_lattice(a->H, a->W, a->lat_c_h, a->lat_c_w);
    hipLaunchKernelGGL(submap_stats_kernel, dim3(a->n_boxes), dim3(SM_TPB), 0, (hipStream_t)stream, c);
    return check_launch("submap_frame_stats");
}

extern "C" int mipsf_submap_overlap(const mipsf_submap_overlap_args* a, void* stream) {
    static const char* who = "mipsf_submap_overlap";
    MIPSF_ARGS(a, mipsf_submap_overlap_args, who);
    MIPSF_REQUIRE(a->H >= 1 && a->W >= 1 && (uint64_t)a->H * a->W <= (1ull << 28), "%s: image %u x %u", who, a->H, a->W);
    if (check_lattice(who, "C", a->H, a->W, a->lat_h, a->lat_w)) return 1;
    MIPSF_REQUIRE(a->k <= MIPSF_SUBMAP_MAX_TOP_KF, "%s: %u chosen keyframes, accepted are at most %u", who, a->k, MIPSF_SUBMAP_MAX_TOP_KF);
    MIPSF_REQUIRE(a->n_related <= (1u << 20), "%s: %u related keyframes", who, a->n_related);
    MIPSF_REQUIRE(a->n_related > 0 || a->k > 0, "%s: neither related nor chosen keyframes", who);
    MIPSF_REQUIRE(a->rows && a->pose, "%s: null pointer", who);
    if (a->n_related > 0) {
        MIPSF_REQUIRE(a->table && a->related_slots && a->related_poses && a->dist, "%s: null pointer (phase a)", who);
        MIPSF_REQUIRE(a->n_slots >= 1 && a->rows_per_slot >= 1, "%s: ray table of %u slots x %u rows", who, a->n_slots, a->rows_per_slot);
        MIPSF_REQUIRE(((uintptr_t)a->dist & 7u) == 0, "%s: dist not 8-byte aligned", who);
    }
    if (a->k > 0)
        MIPSF_REQUIRE(a->top_poses && a->top_kf_masks && a->mask_final && a->count && a->target_d && a->rays_d_cam, "%s: null pointer (phase b)", who);
    const Lattice C = make_lattice(a->H, a->W, a->lat_h, a->lat_w);
    if (a->n_related > 0) {
        DistCfg c;
        c.rows = a->rows, c.pose = a->pose, c.table = a->table, c.slots = a->related_slots, c.poses = a->related_poses, c.dist = a->dist;
        c.W = a->W, c.n_slots = a->n_slots, c.rows_per_slot = a->rows_per_slot, c.C = C;
        hipLaunchKernelGGL(submap_dist_kernel, dim3(a->n_related), dim3(SM_TPB), 0, (hipStream_t)stream, c);
        if (check_launch("submap_overlap (distances)")) return 1;
    }
    if (a->k > 0) {
        MaskCfg c;
        c.rows = a->rows, c.pose = a->pose, c.top_poses = a->top_poses, c.top_kf_masks = a->top_kf_masks, c.mask_final = a->mask_final;
        c.count = a->count, c.target_d = a->target_d, c.rays_d_cam = a->rays_d_cam, c.W = a->W, c.k = a->k;
        c.fx = a->fx, c.fy = a->fy, c.cx = a->cx, c.cy = a->cy, c.u_hi = a->cam_W - a->edge, c.v_hi = a->cam_H - a->edge, c.edge = a->edge;
        for (int i = 0; i < 6; ++i) c.box[i] = a->target_box[i];
        c.C = C;
        hipLaunchKernelGGL(submap_mask_kernel, dim3(1), dim3(SM_MASK_TPB), 0, (hipStream_t)stream, c);
        return check_launch("submap_overlap");
    }
    return 0;
}
