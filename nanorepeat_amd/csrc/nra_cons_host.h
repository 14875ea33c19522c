// nra_cons_host.h -- host-side pieces shared by the two callers of the banded tract alignment (nra_consensus_host.cpp,
// nra_split_host.cpp): the pointer budget of a launch and what a band class proves.
#ifndef NRA_CONS_HOST_H
#define NRA_CONS_HOST_H
#include "nra_host_util.h"

namespace nra_cons {

const int64_t kPtrBudget = int64_t(1) << 30;    // traceback pointer bytes per launch (one tract beyond it goes alone)

// what band class c_idx (c = 1 << c_idx) proves for a tract of n bases on a backbone of t: -1 if it holds no band
inline int proven(int c_idx, int n, int t)
{
    const int extra = 64 * (1 << c_idx) - 1 - std::abs(t - n);
    return extra < 0 ? -1 : std::abs(t - n) + 2 * (extra / 2);
}

// the traceback pointer bytes a launch may use: kPtrBudget, or NRA_TEST_CONS_PTR_BYTES (tests force small chunks)
inline int64_t ptr_budget() { return nra_host::test_bytes("NRA_TEST_CONS_PTR_BYTES", kPtrBudget); }

// the band class a tract of n bases is first aligned in on a backbone of t
inline int start_class(int n, int t, int max_dist)
{
    const int want = std::min(max_dist, std::abs(t - n) + n / 6 + 8);
    int cls = 0;
    while (cls < NRA_CONS_CLASSES - 1 && proven(cls, n, t) < want) ++cls;
    return cls;
}

}  // namespace nra_cons

#endif  // NRA_CONS_HOST_H
