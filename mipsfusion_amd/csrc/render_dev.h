// The compositing and loss arithmetic of render.hip, stated ONCE for its three kernels (render_fwd_ray, render_train_kernel,
// render_bwd_kernel): functions of scalars, no loops over samples.  The kernels keep their loops, staging and reductions; that
// they agree bit for bit (-ffp-contract=off: the bits follow the source) follows from calling the same functions.
//
// Reference: model/scene_rep.py:58-103 (sdf2weights, raw2outputs), :211-236 (losses); helper_functions/utils.py:21-49, 71-111.
#pragma once
#include "common.h"

namespace mipsf {

struct RenderCfg {
    float trunc;          // training.trunc
    float band;           // fp32(sc_factor * trunc): z < z_min + band
    float trunc_total;    // fp32(trunc * sc_factor): loss truncation
    float depth_trunc;
    int rgb_missing_nonzero;
    float emd_w;
};

// the wavefront-scope LDS hand-over: what the wave's lanes wrote to LDS before it, every lane may read after it
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------ first crossing
// Both: first k in [0, S-1) with s[k] * s[k+1] < 0, else 0 (torch.argmax of an all-zero row).
// srow: the ray's S SDF values in LDS
__device__ __forceinline__ uint32_t first_crossing(const float* __restrict__ srow, uint32_t S, uint32_t lane) {
    uint32_t found = 0xFFFFFFFFu;
    for (uint32_t base = 0; base + 1 < S; base += MIPSF_WAVE) {
        const uint32_t k = base + lane;
        const bool hit = (k + 1 < S) && (srow[k] * srow[k + 1] < 0.0f);
        const unsigned long long m = __ballot(hit);
        if (m != 0ull) {
            found = base + (uint32_t)(__ffsll((long long)m) - 1);
            break;
        }
    }
    return found == 0xFFFFFFFFu ? 0u : found;
}
// sraw: the ray's S ten-word records in LDS (word 3: SDF); sv[j]: the SDF of this lane's sample lane + 64 j, in registers
template <int KMAX>
__device__ __forceinline__ uint32_t first_crossing_staged(const float* sraw, const float (&sv)[KMAX], uint32_t S, uint32_t lane) {
    uint32_t kc = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        const uint32_t k = lane + (uint32_t)j * MIPSF_WAVE;
        const float nxt = (k + 1 < S) ? sraw[(k + 1) * 10 + 3] : 0.0f;
        const bool hit = (k + 1 < S) && (sv[j] * nxt < 0.0f);
        const unsigned long long m = __ballot(hit);
        if (!found && m != 0ull) kc = (uint32_t)j * MIPSF_WAVE + (uint32_t)(__ffsll((long long)m) - 1), found = true;
    }
    return kc;
}

// ------------------------------------------------------------------ compositing
// One sample's weight before normalisation: u = sigmoid(s / trunc) sigmoid(-s / trunc), kept in front of z_cut only.
struct SampleWeight {
    float u, sg;          // sg = sigmoid(s / trunc): the backward needs it again
    bool keep;
    __device__ __forceinline__ float kept() const { return keep ? u : 0.f; }
};
__device__ __forceinline__ SampleWeight sample_weight(float s, float z, float trunc, float z_cut) {
    SampleWeight w;
    const float q = s / trunc;
    w.sg = sigmoidf_(q);
    w.u = w.sg * sigmoidf_(-q);
    w.keep = z < z_cut;
    return w;
}

// the per-ray outputs from the finished sums (var / disp / acc are optional); writes ray n's entries
__device__ __forceinline__ void store_ray_outputs(uint32_t n, float a_r, float a_g, float a_b, float a_d, float a_v, float a_w,
                                                  float* __restrict__ rgb_out, float* __restrict__ depth_out,
                                                  float* __restrict__ var_out, float* __restrict__ disp_out,
                                                  float* __restrict__ acc_out) {
    rgb_out[3 * n] = a_r, rgb_out[3 * n + 1] = a_g, rgb_out[3 * n + 2] = a_b;
    depth_out[n] = a_d;
    if (var_out) var_out[n] = a_v;
    if (disp_out) {
        // a ray whose weights all underflowed has 0 / 0 here: torch.max keeps the NaN (scene_rep.py:100), fmaxf would drop it
        const float q = a_d / a_w;
        disp_out[n] = 1.0f / (q != q ? q : fmaxf(1e-10f, q));
    }
    if (acc_out) acc_out[n] = a_w;
}

// ------------------------------------------------------------------ losses: one sample
// fm: in front of the truncation band; bm: inside it (rays with a target depth only)
struct BandMasks {
    float fm, bm;
};
__device__ __forceinline__ BandMasks band_masks(float z, float d, float T) {
    const bool front = z < d - T;
    const bool back = z > d + T;
    BandMasks m;
    m.fm = front ? 1.f : 0.f;
    m.bm = (!front && !back && d > 0.f) ? 1.f : 0.f;
    return m;
}
__device__ __forceinline__ float fs_residual(float s, float fm) { return s * fm - fm; }
__device__ __forceinline__ float sdf_residual(float z, float s, float d, float T, float bm) { return (z + s * T) * bm - d * bm; }
// the sample's position in the band as a class index in [0, 4] (EMD terms)
__device__ __forceinline__ float emd_target(float z, float d, float T) { return (((d - z) + T) / (2.f * T)) * 4.f; }

// Forward: the sample's terms are added to the ray's four sums p = {fs_sq, sdf_sq, fs_emd, sdf_emd}.  prob: its five class
// probabilities (read only with emd_w > 0).
__device__ __forceinline__ void loss_terms_add(float z, float s, float d, float T, float emd_w, const float* prob, float (&p)[4]) {
    const BandMasks m = band_masks(z, d, T);
    const float ef = fs_residual(s, m.fm);
    p[0] += ef * ef;
    const float es = sdf_residual(z, s, d, T, m.bm);
    p[1] += es * es;
    if (emd_w > 0.f) {
        const float gt = emd_target(z, d, T);
        float fe = 0.f, se = 0.f;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float pc = prob[c];
            fe += pc * (float)(4 - c) * m.fm;
            se += fabsf(gt - (float)c) * m.bm * pc;
        }
        p[2] += fe;
        p[3] += se;
    }
}

// Backward of the same terms.  gF, gS: d objective / d {fs, sdf}_loss; fs_w, sdf_w: band_weights; NS: samples the losses
// were normalised by.
struct LossGrad {
    float gF, gS, fs_w, sdf_w, NS;
};
// adds to ds (d objective / d sdf) and sets dp (d objective / d class probabilities; stays as it is with emd_w = 0)
__device__ __forceinline__ void loss_terms_grad(float z, float s, float d, float T, float emd_w, const LossGrad& g, float& ds,
                                                float (&dp)[5]) {
    const BandMasks m = band_masks(z, d, T);
    ds += g.gF * g.fs_w * (2.f / g.NS) * m.fm * fs_residual(s, m.fm);
    ds += g.gS * g.sdf_w * (2.f / g.NS) * (m.bm * T) * sdf_residual(z, s, d, T, m.bm);
    if (emd_w > 0.f) {
        const float gt = emd_target(z, d, T);
        const float kf = g.gF * emd_w / (250.f * g.NS), ks = g.gS * emd_w / (5000.f * g.NS);
#pragma unroll
        for (int c = 0; c < 5; ++c) dp[c] = kf * m.fm * (float)(4 - c) + ks * m.bm * fabsf(gt - (float)c);
    }
}

// ------------------------------------------------------------------ losses: one ray
__device__ __forceinline__ bool depth_valid(float d, float depth_trunc) { return (d > 0.f) && (d < depth_trunc); }
// The colour error's weight.  The reference multiplies by (valid | rgb_missing) with rgb_missing cast to bool: ANY non-zero
// value counts every ray, whatever the configured weight is.
__device__ __forceinline__ float colour_weight(bool valid, int rgb_missing_nonzero) { return (valid || rgb_missing_nonzero) ? 1.f : 0.f; }

// row[0..6] = {rgb_sq, depth_sq(valid), fs_sq, sdf_sq, fs_emd, sdf_emd, valid flag} of a ray: a_*: rendered, t_* / d: target,
// p: the sums of loss_terms_add
__device__ __forceinline__ void loss_row(float a_r, float a_g, float a_b, float a_d, float t_r, float t_g, float t_b, float d,
                                         const RenderCfg& rc, const float (&p)[4], float (&row)[7]) {
    const bool valid = depth_valid(d, rc.depth_trunc);
    const float cw = colour_weight(valid, rc.rgb_missing_nonzero);
    const float e0 = a_r * cw - t_r * cw;
    const float e1 = a_g * cw - t_g * cw;
    const float e2 = a_b * cw - t_b * cw;
    const float ed = a_d - d;
    row[0] = e0 * e0 + e1 * e1 + e2 * e2, row[1] = valid ? ed * ed : 0.f;
    row[2] = p[0], row[3] = p[1], row[4] = p[2], row[5] = p[3];
    row[6] = valid ? 1.f : 0.f;
}

// fs_weight, sdf_weight from the batch's front / band counts
__device__ __forceinline__ void band_weights(float n_front, float n_band, float& fs_w, float& sdf_w) {
    const float total = n_front + n_band;
    fs_w = 1.0f - n_front / total;     // 0/0 -> NaN exactly like the reference
    sdf_w = 1.0f - n_band / total;
}

// ------------------------------------------------------------------ backward
// d objective / d one loss: given directly and / or as (d objective / d total) x weight
__device__ __forceinline__ float loss_grad(float g_loss, float g_total, float weight) { return g_loss + g_total * weight; }

// gradients reaching a ray's rendered maps
struct MapGrad {
    float r, g, b, d;
    // d objective / d (one sample's weight)
    __device__ __forceinline__ float at(float c0, float c1, float c2, float z) const { return r * c0 + g * c1 + b * c2 + d * z; }
};
// adds the colour and depth losses' share.  gR, gD: d objective / d {rgb, depth}_loss; n_norm: rays the losses were normalised
// by; n_valid: rays with a valid depth among them
__device__ __forceinline__ void map_grad_add(MapGrad& G, float gR, float gD, float a_r, float a_g, float a_b, float a_d, float t_r,
                                             float t_g, float t_b, float d, const RenderCfg& rc, float n_norm, float n_valid) {
    const bool valid = depth_valid(d, rc.depth_trunc);
    const float cw = colour_weight(valid, rc.rgb_missing_nonzero);
    const float k_rgb = gR * 2.f * cw * cw / (3.f * n_norm);
    G.r += k_rgb * (a_r - t_r);
    G.g += k_rgb * (a_g - t_g);
    G.b += k_rgb * (a_b - t_b);
    if (valid) G.d += gD * 2.f * (a_d - d) / n_valid;
}

// One sample's ten words of d objective / d raw.  w, c0..c2, z, s: the sample (weight, colours after the sigmoid, depth, SDF);
// dot = sum_k G.at(k) wn_k and inv = 1 / (sum of kept u + 1e-8) of its ray; train: with the losses' share lg (d: target depth)
__device__ __forceinline__ void sample_grad_record(float* o, const MapGrad& G, float dot, float inv, const SampleWeight& w, float c0,
                                                   float c1, float c2, float z, float s, float d, const RenderCfg& rc,
                                                   bool train, const LossGrad& lg) {
    const float wn = w.kept() * inv;
    float ds = w.keep ? (G.at(c0, c1, c2, z) - dot) * inv * (w.u * (1.f - 2.f * w.sg) / rc.trunc) : 0.f;
    float dp[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (train) loss_terms_grad(z, s, d, rc.trunc_total, rc.emd_w, lg, ds, dp);
    o[0] = G.r * wn * c0 * (1.f - c0);
    o[1] = G.g * wn * c1 * (1.f - c1);
    o[2] = G.b * wn * c2 * (1.f - c2);
    o[3] = ds;
    o[4] = 0.f;
#pragma unroll
    for (int c = 0; c < 5; ++c) o[5 + c] = dp[c];
}

}  // namespace mipsf
