// The sub-map box arithmetic, stated ONCE for the device (submap.hip) and for the host (host/hostsubmap.cpp, which the CPU
// restatement calls): Manager.py:614-717 localMLP_expand_rule, float32, per axis and literally -- the abs, the `> 0` test and the
// proportional clamp included.  Every unit that includes this is compiled with contraction off: a fused multiply-add anywhere in
// here moves a box face by one ulp, and points of a frame lie exactly on box faces (the boxes are built from the same points).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MIPSF_SUBMAP_HD __host__ __device__ inline
#else
#define MIPSF_SUBMAP_HD inline
#endif

namespace mipsf {
namespace submap {

// which branch an axis took (2 bits would do; one byte per axis in the record)
enum : uint32_t {
    EXPAND_CONTAINED = 0,  // the frame's box lies inside on all six faces: centre and length come back untouched (all three axes)
    EXPAND_FULL = 1,       // len >= max_len: this axis cannot grow
    EXPAND_FREE = 2,       // case 1: the union fits under max_len
    EXPAND_POS = 3,        // case 2.1: clamped, grows on the positive side only
    EXPAND_NEG = 4,        // case 2.2: clamped, grows on the negative side only
    EXPAND_BOTH = 5        // case 3: clamped, both sides, in proportion
};

MIPSF_SUBMAP_HD float abs32(float v) { return v < 0.0f ? -v : v; }

// box (c, l) of a sub-map, surface box (kc, kl) of a frame, the sub-map's max_len (mx) -> (oc, ol); returns the three axes' cases,
// axis a in bits 8a .. 8a+7
MIPSF_SUBMAP_HD uint32_t expand_rule(const float c[3], const float l[3], const float kc[3], const float kl[3], const float mx[3],
                                     float oc[3], float ol[3]) {
    float kmin[3], kmax[3], mmin[3], mmax[3];
    bool grow_neg[3], grow_pos[3], contained = true;
    for (int a = 0; a < 3; ++a) {
        kmin[a] = kc[a] - 0.5f * kl[a], kmax[a] = kc[a] + 0.5f * kl[a];
        mmin[a] = c[a] - 0.5f * l[a], mmax[a] = c[a] + 0.5f * l[a];
        grow_neg[a] = !(kmin[a] >= mmin[a]);
        grow_pos[a] = !(kmax[a] <= mmax[a]);
        contained = contained && !grow_neg[a] && !grow_pos[a];
    }
    if (contained) {
        for (int a = 0; a < 3; ++a) oc[a] = c[a], ol[a] = l[a];
        return 0u;
    }
    uint32_t cases = 0u;
    for (int a = 0; a < 3; ++a) {
        const float lo = kmin[a] < mmin[a] ? kmin[a] : mmin[a];
        const float hi = kmax[a] > mmax[a] ? kmax[a] : mmax[a];
        uint32_t which;
        if (l[a] >= mx[a]) {
            oc[a] = c[a], ol[a] = l[a];
            which = EXPAND_FULL;
        } else if (hi - lo <= mx[a]) {
            ol[a] = hi - lo;
            oc[a] = lo + 0.5f * ol[a];
            which = EXPAND_FREE;
        } else if (!(grow_neg[a] && grow_pos[a])) {
            const float pos = abs32(hi - mmax[a]);
            const float room = mx[a] - l[a];
            if (pos > 0.0f) {
                oc[a] = c[a] + 0.5f * room;
                which = EXPAND_POS;
            } else {
                oc[a] = c[a] - 0.5f * room;
                which = EXPAND_NEG;
            }
            ol[a] = mx[a];
        } else {
            const float pos = abs32(hi - mmax[a]), neg = abs32(mmin[a] - lo);
            const float room = mx[a] - l[a];
            const float pos_clamp = room * pos / (pos + neg);
            const float neg_clamp = room * neg / (pos + neg);
            const float hi_new = mmax[a] + pos_clamp, lo_new = mmin[a] - neg_clamp;
            ol[a] = hi_new - lo_new;
            oc[a] = lo_new + 0.5f * ol[a];
            which = EXPAND_BOTH;
        }
        cases |= which << (8 * a);
    }
    return cases;
}

// strictly inside the box centre -+ 0.5 * len, the faces formed in float32 (geometry_helper.py:193-201 pts_in_bbox)
MIPSF_SUBMAP_HD bool inside(const float p[3], const float c[3], const float l[3]) {
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        const float lo = c[a] - 0.5f * l[a], hi = c[a] + 0.5f * l[a];
        in = in && p[a] > lo && p[a] < hi;
    }
    return in;
}

}  // namespace submap
}  // namespace mipsf
