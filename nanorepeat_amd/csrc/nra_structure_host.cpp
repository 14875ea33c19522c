// nra_structure_host.cpp -- C ABI of the repeat structure alignment (nra_read_structure): argument checks, the motif
// masks, and the lane plan of nra_lane_host.h (reads ordered by phase capacity, then tract length; chunks that bound the
// traceback pointers' device memory) with the launches of k_structure (nra_structure.hip).
#include "nra_lane_host.h"

#include <new>

using namespace nra_host;

extern "C" {

int nra_read_structure(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off, int32_t n_reads,
                       const char* seqs, const int64_t* seq_off, const int32_t* read_motif, int32_t* edits,
                       int32_t* start_phase, uint8_t* path)
{
    if (n_motifs < 1) return fail(NRA_E_ARG, "n_motifs must be >= 1");
    if (!motifs || !motif_off) return fail(NRA_E_ARG, "motifs or motif_off is NULL");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (motif_off[0] < 0) return fail(NRA_E_ARG, "negative motif offset");
    if (int rc = check_motifs(0, n_motifs, motifs, motif_off, NRA_STRUCT_MAX_P)) return rc;
    if (n_reads > 0) {
        if (!seq_off || !read_motif || !edits || !start_phase) return fail(NRA_E_ARG, "NULL read array");
        if (int rc = check_tract_offsets(n_reads, seq_off, NRA_STRUCT_MAX_N, "read")) return rc;
        for (int32_t r = 0; r < n_reads; ++r)
            if (read_motif[r] < 0 || read_motif[r] >= n_motifs) return fail(NRA_E_ARG, "read_motif out of range");
        if (seq_off[n_reads] > seq_off[0] && (!seqs || !path)) return fail(NRA_E_ARG, "seqs or path is NULL");
    }
    if (int rc = use_device(device, n_reads > 0)) return rc;
    if (n_reads == 0) return NRA_OK;
    try {
        const std::vector<NraStructMotif> mo = motif_masks(n_motifs, motifs, motif_off);
        DevBuf<NraStructMotif> d_mo;
        NRA_HIP_TRY(d_mo.alloc(mo.size()));
        NRA_HIP_TRY(hipMemcpy(d_mo.p, mo.data(), mo.size() * sizeof(NraStructMotif), hipMemcpyHostToDevice));

        auto cap_of = [&](int32_t r) { return capacity((int)(motif_off[read_motif[r] + 1] - motif_off[read_motif[r]])); };
        auto words_of = [](int P) { return NRA_STRUCT_WORDS(P); };
        const std::vector<int32_t> order = lane_order(n_reads, seq_off, cap_of);
        const LaneOut out{2, {edits, start_phase}, {path}};
        for (const Chunk& ck : lane_chunks(order, seq_off, cap_of, words_of,
                                           test_bytes("NRA_TEST_STRUCT_PTR_BYTES", kPtrBudget))) {
            const size_t n = ck.last - ck.first;
            const int rc = run_lanes(order.data() + ck.first, n, seqs, seq_off, read_motif, words_of(ck.cls), out,
                                     "k_structure",
                                     [&](const NraStructRead* rd, const uint8_t* codes, uint32_t* ptr,
                                         uint8_t* const* planes, int32_t* res) {
                                         return nra_launch_structure(nullptr, ck.cls, (int)n, rd, d_mo.p, codes, ptr,
                                                                     planes[0], res);
                                     });
            if (rc != NRA_OK) return rc;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "read structure: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
