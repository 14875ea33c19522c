// nra_segment_host.cpp -- C ABI of the motif-run alignment (nra_tract_segments): argument checks, the motif sets as state
// masks, and the lane plan of nra_lane_host.h (tracts ordered by state class, then tract length; chunks that bound the
// traceback pointers' device memory) with the launches of k_segment (nra_segment.hip).
#include "nra_lane_host.h"

#include <cstdint>
#include <new>

using namespace nra_host;

namespace {

// the kernel's state class for a set of S states
int state_class(int S) { return S <= 8 ? 8 : S <= 16 ? 16 : 32; }

}  // namespace

extern "C" {

int nra_tract_segments(int device, int32_t n_sets, const int32_t* set_motif_off, const char* motifs,
                       const int64_t* motif_off, int32_t n_tracts, const char* seqs, const int64_t* seq_off,
                       const int32_t* tract_set, int32_t switch_cost, int32_t* edits, int32_t* start_phase,
                       int32_t* start_motif, uint8_t* path, uint8_t* motif_of)
{
    if (n_sets < 1) return fail(NRA_E_ARG, "n_sets must be >= 1");
    if (!set_motif_off || !motifs || !motif_off) return fail(NRA_E_ARG, "set_motif_off, motifs or motif_off is NULL");
    if (n_tracts < 0) return fail(NRA_E_ARG, "negative tract count");
    if (switch_cost <= 0) return fail(NRA_E_ARG, "switch_cost must be >= 1");
    if (switch_cost > NRA_SEG_MAX_SWITCH) return fail(NRA_E_RANGE, "switch_cost is larger than 1000");
    if (set_motif_off[0] < 0 || motif_off[0] < 0) return fail(NRA_E_ARG, "negative offset");
    std::vector<int> states((size_t)n_sets);
    for (int32_t q = 0; q < n_sets; ++q) {
        const int64_t M = (int64_t)set_motif_off[q + 1] - set_motif_off[q];
        if (M < 1) return fail(NRA_E_ARG, "set " + std::to_string(q) + " is empty");
        if (M > NRA_SEG_MAX_MOTIFS) return fail(NRA_E_RANGE, "set " + std::to_string(q) + " has more than 8 motifs");
        // no limit on one motif: the sum over the set is the limit
        if (int rc = check_motifs(set_motif_off[q], set_motif_off[q + 1], motifs, motif_off, INT64_MAX)) return rc;
        const int64_t S = motif_off[set_motif_off[q + 1]] - motif_off[set_motif_off[q]];
        if (S > NRA_SEG_MAX_STATES)
            return fail(NRA_E_RANGE, "set " + std::to_string(q) + " has more than 32 motif bases in all");
        states[(size_t)q] = (int)S;
    }
    if (n_tracts > 0) {
        if (!seq_off || !tract_set || !edits || !start_phase || !start_motif) return fail(NRA_E_ARG, "NULL tract array");
        if (int rc = check_tract_offsets(n_tracts, seq_off, NRA_STRUCT_MAX_N, "tract")) return rc;
        for (int32_t r = 0; r < n_tracts; ++r)
            if (tract_set[r] < 0 || tract_set[r] >= n_sets) return fail(NRA_E_ARG, "tract_set out of range");
        if (seq_off[n_tracts] > seq_off[0] && (!seqs || !path || !motif_of))
            return fail(NRA_E_ARG, "seqs, path or motif_of is NULL");
    }
    if (int rc = use_device(device, n_tracts > 0)) return rc;
    if (n_tracts == 0) return NRA_OK;
    try {
        // state masks: state g = (motif m, phase j) in (m, j) order; eq[c] bit g <=> u_m[(j - 1) mod p_m] has code c
        std::vector<NraSegSet> ss((size_t)n_sets);
        for (int32_t q = 0; q < n_sets; ++q) {
            NraSegSet& x = ss[(size_t)q];
            std::memset(&x, 0, sizeof(x));
            x.S = states[(size_t)q];
            int g = 0;
            for (int32_t m = set_motif_off[q]; m < set_motif_off[q + 1]; ++m) {
                const char* u = motifs + motif_off[m];
                const int p = (int)(motif_off[m + 1] - motif_off[m]);
                x.first |= 1u << g;
                x.last |= 1u << (g + p - 1);
                for (int j = 0; j < p; ++j, ++g) x.eq[kBase.of[(unsigned char)u[(j + p - 1) % p]]] |= 1u << g;
            }
        }
        DevBuf<NraSegSet> d_sets;
        NRA_HIP_TRY(d_sets.alloc(ss.size()));
        NRA_HIP_TRY(hipMemcpy(d_sets.p, ss.data(), ss.size() * sizeof(NraSegSet), hipMemcpyHostToDevice));

        auto cls_of = [&](int32_t r) { return state_class(states[(size_t)tract_set[r]]); };
        auto words_of = [](int SC) { return NRA_SEG_WORDS(SC); };
        const std::vector<int32_t> order = lane_order(n_tracts, seq_off, cls_of);
        const LaneOut out{4, {edits, start_phase, start_motif}, {path, motif_of}};
        for (const Chunk& ck : lane_chunks(order, seq_off, cls_of, words_of,
                                           test_bytes("NRA_TEST_SEG_PTR_BYTES", kPtrBudget))) {
            const size_t n = ck.last - ck.first;
            const int rc = run_lanes(order.data() + ck.first, n, seqs, seq_off, tract_set, words_of(ck.cls), out,
                                     "k_segment",
                                     [&](const NraStructRead* rd, const uint8_t* codes, uint32_t* ptr,
                                         uint8_t* const* planes, int32_t* res) {
                                         return nra_launch_segment(nullptr, ck.cls, (int)n, rd, d_sets.p, codes,
                                                                   switch_cost, ptr, planes[0], planes[1], res);
                                     });
            if (rc != NRA_OK) return rc;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "tract segments: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
