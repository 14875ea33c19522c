// nra_consensus.hip -- allele consensus: banded unit-cost alignment of tracts to their group's backbone, column votes,
// and the next backbone (gfx950).
//
//   k_cons_align<C>  one wave per tract: the banded DP of nra_cons_dp.h (cons_band_align<C>, shared with the pileup of
//                    nra_split.hip).  When the banded distance proves exact (include/nanorepeat_amd.h) and is at most
//                    max_dist, lane 0 walks back from (n, t) and adds the tract's votes to its group's tables with
//                    integer atomics (integer adds commute: the tables do not depend on the order).
//   k_cons_build     one wave per group: 64 backbone positions per step, each lane decides what its slot and its column
//                    emit, the output positions come from two ballots, and the wave notes whether the backbone changed.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 18 and tests/consensus_ref.py.  No floating point.
#include "nra_cons_dp.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(32)

template <int C>
__global__ __launch_bounds__(WAVE) void k_cons_align(int n_items, const NraConsItem* __restrict__ items,
                                                     const NraConsGroup* __restrict__ groups,
                                                     const uint8_t* __restrict__ seqs,
                                                     const uint8_t* __restrict__ backbones, uint4* __restrict__ ptrs,
                                                     int32_t* __restrict__ tabs, int32_t* __restrict__ voters,
                                                     int32_t* __restrict__ status, int max_dist)
{
    const int it = blockIdx.x;
    if (it >= n_items) return;
    const int lane = threadIdx.x;
    const NraConsItem item = items[it];
    const NraConsGroup grp = groups[item.group];
    const int n = item.n, t = grp.t;
    const uint8_t* s = seqs + item.seq;
    uint4* pblk = ptrs + item.ptr;
    int kend = 0;
    const int dist = cons_band_align<C>(n, t, s, backbones + grp.bb, pblk, lane, max_dist, kend);
    if (dist < 0) {                           // NRA_CONS_WIDEN or NRA_CONS_LEFT_OUT
        if (lane == 0) status[it] = dist;
        return;
    }
    __threadfence();                          // the other lanes' pointer stores, before lane 0 loads them
    __syncthreads();
    if (lane != 0) return;

    // ---- traceback on one lane
    int32_t* tab = tabs + grp.tab;
    int i = n, j = t, k = kend;
    long long have = -1, have_s = -1;
    uint4 pw = make_uint4(0, 0, 0, 0), sw = make_uint4(0, 0, 0, 0);
    int run_base = -1;                        // the insertion run of slot j: its base nearest the tract's start so far
    while (i > 0 || j > 0) {
        const uint32_t op = cons_walk_op<C>(pblk, n, i, j, k, have, pw);
        const int base = op != 2u ? cons_walk_base(s, i, have_s, sw) : 0;
        if (op == 1u) {
            run_base = base;
            --i;
            ++k;
            continue;
        }
        if (run_base >= 0) {
            if (run_base < 4) atomicAdd(tab + (size_t)j * NRA_CONS_TAB + 5 + run_base, 1);
            run_base = -1;
        }
        if (op == 0u) {
            if (base < 4) atomicAdd(tab + (size_t)(j - 1) * NRA_CONS_TAB + base, 1);
            --i;
            --j;
        } else {
            atomicAdd(tab + (size_t)(j - 1) * NRA_CONS_TAB + 4, 1);
            --j;
            --k;
        }
    }
    if (run_base >= 0 && run_base < 4) atomicAdd(tab + 5 + run_base, 1);      // a run that ends in slot 0
    atomicAdd(voters + item.group, 1);
    status[it] = dist;
}

__global__ __launch_bounds__(WAVE) void k_cons_build(int n_groups, const NraConsGroup* __restrict__ groups,
                                                     const uint8_t* __restrict__ backbones,
                                                     const int32_t* __restrict__ tabs,
                                                     const int32_t* __restrict__ voters,
                                                     uint8_t* __restrict__ new_backbones, int32_t* __restrict__ support,
                                                     int32_t* __restrict__ res)
{
    const int g = blockIdx.x;
    if (g >= n_groups) return;
    const int lane = threadIdx.x;
    const NraConsGroup grp = groups[g];
    const int t = grp.t, mv = voters[g];
    if (mv == 0) {                            // nobody voted: the host keeps the backbone it has
        if (lane == 0) { res[3 * g] = t; res[3 * g + 1] = 0; res[3 * g + 2] = 0; }
        return;
    }
    const uint8_t* b = backbones + grp.bb;
    const int32_t* tab = tabs + grp.tab;
    uint8_t* nb = new_backbones + grp.nb;
    int32_t* sup = support + grp.nb;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
    bool changed = false;
    for (int j0 = 0; j0 <= t; j0 += WAVE) {
        const int j = j0 + lane;
        bool e1 = false, e2 = false;
        int c1 = 0, s1 = 0, c2 = 0, s2 = 0;
        if (j <= t) {
            const int32_t* row = tab + (size_t)j * NRA_CONS_TAB;
            int tot = 0;
            for (int c = 0; c < 4; ++c) {
                const int v = row[5 + c];
                tot += v;
                if (v > s1) { s1 = v; c1 = c; }                  // a tie keeps the smaller code
            }
            e1 = 2 * tot > mv;
            if (j < t) {
                const int own = b[j];
                int mx = row[0];
                for (int c = 1; c < 5; ++c) mx = imax(mx, row[c]);
                c2 = 4;
                for (int c = 4; c >= 0; --c) c2 = row[c] == mx ? c : c2;      // the smallest tied code, deleted last
                if (row[own] == mx) c2 = own;
                s2 = mx;
                e2 = c2 != 4;
            }
        }
        const unsigned long long m1 = __ballot(e1), m2 = __ballot(e2);
        int pos = base + __popcll(m1 & below) + __popcll(m2 & below);
        if (e1) {
            nb[pos] = (uint8_t)c1;
            sup[pos] = s1;
            changed |= pos >= t || b[pos] != c1;
            ++pos;
        }
        if (e2) {
            nb[pos] = (uint8_t)c2;
            sup[pos] = s2;
            changed |= pos >= t || b[pos] != c2;
        }
        base += __popcll(m1) + __popcll(m2);
    }
    const bool any = __ballot(changed) != 0ull || base != t;
    if (lane == 0) { res[3 * g] = base; res[3 * g + 1] = any ? 1 : 0; res[3 * g + 2] = mv; }
}

template <int C>
static int launch_cons_align(hipStream_t st, int n_items, const NraConsItem* items, const NraConsGroup* groups,
                             const uint8_t* seqs, const uint8_t* backbones, uint4* ptrs, int32_t* tabs, int32_t* voters,
                             int32_t* status, int max_dist)
{
    k_cons_align<C><<<dim3((unsigned)n_items), WAVE, 0, st>>>(n_items, items, groups, seqs, backbones, ptrs, tabs, voters,
                                                             status, max_dist);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_cons_align(hipStream_t st, int c, int n_items, const NraConsItem* items,
                                     const NraConsGroup* groups, const uint8_t* seqs, const uint8_t* backbones,
                                     uint4* ptrs, int32_t* tabs, int32_t* voters, int32_t* status, int max_dist)
{
    if (n_items <= 0) return (int)hipSuccess;
    switch (c) {
    case 1: return launch_cons_align<1>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 2: return launch_cons_align<2>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 4: return launch_cons_align<4>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 8: return launch_cons_align<8>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 16: return launch_cons_align<16>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    default: return (int)hipErrorInvalidValue;
    }
}

extern "C" int nra_launch_cons_build(hipStream_t st, int n_groups, const NraConsGroup* groups, const uint8_t* backbones,
                                     const int32_t* tabs, const int32_t* voters, uint8_t* new_backbones, int32_t* support,
                                     int32_t* res)
{
    if (n_groups <= 0) return (int)hipSuccess;
    k_cons_build<<<dim3((unsigned)n_groups), WAVE, 0, st>>>(n_groups, groups, backbones, tabs, voters, new_backbones,
                                                           support, res);
    return (int)hipGetLastError();
}

#endif  // part 32
