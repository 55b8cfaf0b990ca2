// Host build of the sub-map box arithmetic (../submap_dev.h, the header submap.hip compiles for the device): the CPU restatement
// (tests/submap_cpu.py) calls the rule through here, so there is no second statement of it.  Built with -ffp-contract=off.
#include "../submap_dev.h"
#include "mipsf_host.h"

extern "C" uint32_t mipsf_submap_expand_host(const float* box, const float* surface, const float* max_len, float* out) {
    return mipsf::submap::expand_rule(box, box + 3, surface, surface + 3, max_len, out, out + 3);
}
