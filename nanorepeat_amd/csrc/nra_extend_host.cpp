// nra_extend_host.cpp -- C ABI of the anchored wraparound extension (nra_extend_tracts): argument checks, the motif
// masks, and one run of the lane plan of nra_lane_host.h over all reads (ordered by phase capacity, then tract length):
// one upload of all tracts, one launch of k_extend (nra_extend.hip) per capacity, one download of the four results per
// read.  Nothing is kept per row, so a call is never chunked.
#include "nra_lane_host.h"

#include <new>

using namespace nra_host;

extern "C" {

int nra_extend_tracts(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off, int32_t n_reads,
                      const char* seqs, const int64_t* seq_off, const int32_t* read_motif, int32_t match,
                      int32_t mismatch, int32_t gap, int32_t* score, int32_t* end, int32_t* end_phase,
                      int32_t* motif_bases)
{
    if (n_motifs < 1) return fail(NRA_E_ARG, "n_motifs must be >= 1");
    if (!motifs || !motif_off) return fail(NRA_E_ARG, "motifs or motif_off is NULL");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (match < 1 || match > 127) return fail(NRA_E_ARG, "match must be in 1..127");
    if (mismatch < 0 || mismatch > 127) return fail(NRA_E_ARG, "mismatch must be in 0..127");
    if (gap < 1 || gap > 127) return fail(NRA_E_ARG, "gap must be in 1..127");
    if (motif_off[0] < 0) return fail(NRA_E_ARG, "negative motif offset");
    if (int rc = check_motifs(0, n_motifs, motifs, motif_off, NRA_STRUCT_MAX_P)) return rc;
    if (n_reads > 0) {
        if (!seq_off || !read_motif || !score || !end || !end_phase || !motif_bases)
            return fail(NRA_E_ARG, "NULL read array");
        if (int rc = check_tract_offsets(n_reads, seq_off, NRA_STRUCT_MAX_N, "read")) return rc;
        for (int32_t r = 0; r < n_reads; ++r)
            if (read_motif[r] < 0 || read_motif[r] >= n_motifs) return fail(NRA_E_ARG, "read_motif out of range");
        if (seq_off[n_reads] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device, n_reads > 0)) return rc;
    if (n_reads == 0) return NRA_OK;
    try {
        const std::vector<NraStructMotif> mo = motif_masks(n_motifs, motifs, motif_off);
        DevBuf<NraStructMotif> d_mo;
        NRA_HIP_TRY(d_mo.alloc(mo.size()));
        NRA_HIP_TRY(hipMemcpy(d_mo.p, mo.data(), mo.size() * sizeof(NraStructMotif), hipMemcpyHostToDevice));

        auto cap_of = [&](int32_t r) { return capacity((int)(motif_off[read_motif[r] + 1] - motif_off[read_motif[r]])); };
        const std::vector<int32_t> order = lane_order(n_reads, seq_off, cap_of);
        const size_t n = order.size();
        const LaneOut out{4, {score, end, end_phase, motif_bases}, {}};
        return run_lanes(order.data(), n, seqs, seq_off, read_motif, 0, out, "k_extend",
                         [&](const NraStructRead* rd, const uint8_t* codes, uint32_t*, uint8_t* const*, int32_t* res) {
                             for (size_t i = 0; i < n;) {                 // one launch per capacity
                                 const int P = cap_of(order[i]);
                                 size_t j = i;
                                 while (j < n && cap_of(order[j]) == P) ++j;
                                 const int e = nra_launch_extend(nullptr, P, (int)(j - i), rd + i, d_mo.p, codes, match,
                                                                 mismatch, gap, res + 4 * i);
                                 if (e != 0) return e;
                                 i = j;
                             }
                             return 0;
                         });
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "extend tracts: host allocation failed");
    }
}

}  // extern "C"
