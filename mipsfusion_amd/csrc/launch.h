// Host-only launch helpers of the training units: a run-time selector becomes a compile-time tag, and a kernel is granted its
// dynamic LDS.  An entry point nests with_layout / with_bool / with_int around one generic lambda that names the kernel
// instantiation once (`constexpr auto kern = some_kernel<LAY.value, ...>;`), so a new variant is one tag and one line.
#pragma once
#include <type_traits>

#include "common.h"

namespace mipsf {

template <int V>
using int_tag = std::integral_constant<int, V>;
constexpr std::true_type yes{};
constexpr std::false_type no{};

// f(tag of the selector's value); f is a generic lambda that returns the entry point's int.  The selector was checked before:
// any value but the first ones takes the last tag.
template <class F>
int with_layout(int layout, F&& f) {
    return layout == MIPSF_FEAT_AOS ? f(int_tag<MIPSF_FEAT_AOS>{}) : f(int_tag<MIPSF_FEAT_LEVEL_MAJOR>{});
}
template <class F>
int with_bool(bool b, F&& f) {
    return b ? f(yes) : f(no);
}
template <int A, int B, int C, class F>
int with_int(int v, F&& f) {
    return v == A ? f(int_tag<A>{}) : v == B ? f(int_tag<B>{}) : f(int_tag<C>{});
}

// Kernel may be launched with `bytes` of dynamic LDS?  Per kernel instantiation and per device the largest size granted so far
// is remembered and only a larger one is asked for; a refusal is not remembered and leaves HIP's error for the caller to report
// or to clear.  (Two threads racing here both set the attribute to a size that covers their launch: benign.)
template <auto Kernel>
bool grant_lds(uint32_t bytes) {
    static uint32_t granted_dev[MAX_DEVICES] = {};
    uint32_t& granted = granted_dev[device_slot()];
    if (bytes <= granted) return true;
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    granted = bytes;
    return true;
}
// what a launch that cannot do without its LDS returns on a refusal
inline int lds_refused(uint32_t bytes) {
    set_error("cannot raise dynamic LDS to %d bytes", (int)bytes);
    return 4;
}

}  // namespace mipsf
