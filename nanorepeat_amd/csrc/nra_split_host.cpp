// nra_split_host.cpp -- C ABI of the allele split (nra_allele_split): argument checks, the alignment launches of
// k_split_align (by band class, tracts sorted by length, chunked under the budget of traceback pointer memory, repeated
// in the next class for the tracts whose band could not decide: the consensus host's scheme, one round), then one launch
// of k_split_count and one of k_split_phase for all groups, and the results back (nra_split.hip).
#include "nra_cons_host.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;
using namespace nra_cons;

namespace {

struct Work {
    int32_t tract, group, cls;
};

struct Host {
    std::vector<uint64_t> seq;                 // byte offset of a tract's codes
    std::vector<int32_t> n;                    // its length
    std::vector<int64_t> row;                  // byte offset of its row, -1 without one
    std::vector<uint8_t> codes, bbs;
    std::vector<NraSplitGroup> groups;
    int64_t row_bytes = 0, col_total = 0, mat_bytes = 0, site_total = 0;
};

int run(const Host& H, std::vector<int64_t>& rowtab, int32_t n_tracts, const int64_t* group_off, int max_dist,
        const NraSplitParams& prm, std::vector<NraSplitGroup>& dg, int32_t* label, int32_t* dist,
        std::vector<int32_t>& res, std::vector<int32_t>& sites, std::vector<uint8_t>& mats, int64_t* stats)
{
    const int64_t ptr_budget = nra_cons::ptr_budget();
    const size_t ng = dg.size();
    DevBuf<uint8_t> d_codes, d_bb, d_rows, d_ab, d_mats;
    DevBuf<NraSplitGroup> d_groups;
    DevBuf<NraSplitItem> d_items;
    DevBuf<NraSplitBlock> d_blocks;
    DevBuf<uint4> d_ptr;
    DevBuf<int64_t> d_rowtab;
    DevBuf<int32_t> d_status, d_nb, d_pos, d_key, d_labels, d_sites, d_res;
    NRA_HIP_TRY(d_codes.ensure(H.codes.size()));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, H.codes.data(), H.codes.size(), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_bb.ensure(H.bbs.size()));
    NRA_HIP_TRY(hipMemcpy(d_bb.p, H.bbs.data(), H.bbs.size(), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_groups.ensure(ng));
    NRA_HIP_TRY(hipMemcpy(d_groups.p, dg.data(), ng * sizeof(NraSplitGroup), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_rows.ensure((size_t)H.row_bytes));

    // ---- step 1: every tract that |t - n| does not rule out, in the class the consensus would start it in
    std::vector<Work> work, next;
    std::vector<NraSplitItem> items;
    std::vector<int32_t> status;
    for (size_t g = 0; g < ng; ++g)
        for (int64_t r = group_off[g]; r < group_off[g + 1]; ++r) {
            if (H.row[r] < 0) {                    // the distance is at least |t - n| > max_dist
                stats[13] += 1;
                continue;
            }
            work.push_back(Work{(int32_t)r, (int32_t)g, start_class(H.n[r], dg[g].t, max_dist)});
        }
    while (!work.empty()) {
        std::sort(work.begin(), work.end(), [&](const Work& x, const Work& y) {
            if (x.cls != y.cls) return x.cls < y.cls;
            if (H.n[x.tract] != H.n[y.tract]) return H.n[x.tract] > H.n[y.tract];
            return x.tract < y.tract;
        });
        next.clear();
        for (size_t i = 0; i < work.size();) {
            const int cls = work[i].cls, c = 1 << cls, rows_per_piece = 64 / c;
            items.clear();
            int64_t pieces = 0;
            size_t j = i;
            while (j < work.size() && work[j].cls == cls) {
                const int32_t r = work[j].tract;
                const int64_t pc = (int64_t)((H.n[r] + rows_per_piece - 1) / rows_per_piece) * 64;
                if (j > i && (pieces + pc) * 16 > ptr_budget) break;
                items.push_back(NraSplitItem{H.seq[r], (uint64_t)pieces, (uint64_t)H.row[r], H.n[r], work[j].group});
                pieces += pc;
                stats[cls] += 1;
                stats[5 + cls] += H.n[r];
                ++j;
            }
            const size_t ni = items.size();
            stats[11] += 1;
            stats[14] = std::max<int64_t>(stats[14], pieces * 16);
            NRA_HIP_TRY(d_items.ensure(ni));
            NRA_HIP_TRY(d_status.ensure(ni));
            NRA_HIP_TRY(d_ptr.ensure((size_t)pieces));
            NRA_HIP_TRY(hipMemcpy(d_items.p, items.data(), ni * sizeof(NraSplitItem), hipMemcpyHostToDevice));
            const int e = nra_launch_split_align(nullptr, c, (int)ni, d_items.p, d_groups.p, d_codes.p, d_bb.p, d_ptr.p,
                                                 d_rows.p, d_status.p, max_dist);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_split_align: ") + hipGetErrorString((hipError_t)e));
            NRA_HIP_TRY(hipStreamSynchronize(nullptr));
            status.resize(ni);
            NRA_HIP_TRY(hipMemcpy(status.data(), d_status.p, ni * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < ni; ++q) {
                const Work& wk = work[i + q];
                if (status[q] == NRA_CONS_WIDEN) {
                    if (cls + 1 >= NRA_CONS_CLASSES) return fail(NRA_E_DEVICE, "allele split: the widest band did not decide");
                    stats[12] += 1;
                    next.push_back(Work{wk.tract, wk.group, cls + 1});
                } else if (status[q] >= 0) {
                    dist[wk.tract] = status[q];
                    rowtab[wk.tract] = H.row[wk.tract];
                    dg[wk.group].mv += 1;
                }
            }
            i = j;
        }
        work.swap(next);
    }

    // ---- steps 2 to 4
    std::vector<NraSplitBlock> blocks;
    for (size_t g = 0; g < ng; ++g)
        if (dg[g].mv > 0)
            for (int32_t c0 = 0; c0 < dg[g].t; c0 += NRA_SPLIT_THREADS) blocks.push_back(NraSplitBlock{(int32_t)g, c0});
    NRA_HIP_TRY(hipMemcpy(d_groups.p, dg.data(), ng * sizeof(NraSplitGroup), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_rowtab.ensure((size_t)n_tracts));
    if (n_tracts > 0)
        NRA_HIP_TRY(hipMemcpy(d_rowtab.p, rowtab.data(), (size_t)n_tracts * sizeof(int64_t), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_blocks.ensure(blocks.size()));
    if (!blocks.empty())
        NRA_HIP_TRY(hipMemcpy(d_blocks.p, blocks.data(), blocks.size() * sizeof(NraSplitBlock), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_nb.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_ab.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_pos.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_key.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_mats.ensure((size_t)H.mat_bytes));
    NRA_HIP_TRY(d_labels.ensure((size_t)n_tracts));
    NRA_HIP_TRY(d_sites.ensure((size_t)H.site_total * NRA_SPLIT_SITE_INTS));
    NRA_HIP_TRY(d_res.ensure(ng * NRA_SPLIT_RES_INTS));
    int e = nra_launch_split_count(nullptr, (int)blocks.size(), d_blocks.p, d_groups.p, d_rowtab.p, d_rows.p, prm, d_nb.p,
                                   d_ab.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_split_count: ") + hipGetErrorString((hipError_t)e));
    e = nra_launch_split_phase(nullptr, (int)ng, d_groups.p, d_rowtab.p, d_rows.p, prm, d_nb.p, d_ab.p, d_pos.p, d_key.p,
                               d_mats.p, d_labels.p, d_sites.p, d_res.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_split_phase: ") + hipGetErrorString((hipError_t)e));
    NRA_HIP_TRY(hipStreamSynchronize(nullptr));
    res.resize(ng * NRA_SPLIT_RES_INTS);
    sites.resize((size_t)H.site_total * NRA_SPLIT_SITE_INTS);
    mats.resize((size_t)H.mat_bytes);
    NRA_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (!sites.empty())
        NRA_HIP_TRY(hipMemcpy(sites.data(), d_sites.p, sites.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (!mats.empty()) NRA_HIP_TRY(hipMemcpy(mats.data(), d_mats.p, mats.size(), hipMemcpyDeviceToHost));
    if (n_tracts > 0)
        NRA_HIP_TRY(hipMemcpy(label, d_labels.p, (size_t)n_tracts * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_allele_split(int device, int32_t n_groups, const int64_t* group_off, int32_t n_tracts, const char* seqs,
                     const int64_t* seq_off, const char* backbones, const int64_t* bb_off, int32_t max_dist,
                     int32_t min_count, int32_t min_share_pct, int32_t min_purity_pct, int32_t min_sites,
                     int32_t max_sites, int32_t max_iter, int32_t* label, int32_t* dist, int32_t* group_res,
                     int64_t site_cap, int32_t* sites, int64_t* site_off, int64_t sym_cap, uint8_t* site_sym,
                     int64_t* sym_off, int64_t* stats)
{
    if (n_groups < 0 || n_tracts < 0) return fail(NRA_E_ARG, "negative group or tract count");
    if (!group_off || !site_off || !sym_off) return fail(NRA_E_ARG, "group_off, site_off or sym_off is NULL");
    if (n_groups > 0 && (!group_res || !bb_off)) return fail(NRA_E_ARG, "group_res or bb_off is NULL");
    if (n_tracts > 0 && (!label || !dist)) return fail(NRA_E_ARG, "label or dist is NULL");
    if (max_dist < 0) return fail(NRA_E_ARG, "max_dist must be >= 0");
    if (max_dist > NRA_CONS_MAX_DIST) return fail(NRA_E_RANGE, "max_dist is larger than 1000");
    if (min_count < 1 || min_sites < 1) return fail(NRA_E_ARG, "min_count and min_sites must be >= 1");
    if (min_share_pct < 1 || min_purity_pct < 1) return fail(NRA_E_ARG, "percentages must be >= 1");
    if (min_share_pct > 100 || min_purity_pct > 100) return fail(NRA_E_RANGE, "a percentage is larger than 100");
    if (max_sites < 1 || max_iter < 1) return fail(NRA_E_ARG, "max_sites and max_iter must be >= 1");
    if (max_sites > NRA_SPLIT_MAX_SITES) return fail(NRA_E_RANGE, "max_sites is larger than 4096");
    if (max_iter > NRA_SPLIT_MAX_ITER) return fail(NRA_E_RANGE, "max_iter is larger than 64");
    if (site_cap < 0 || sym_cap < 0 || (site_cap > 0 && !sites) || (sym_cap > 0 && !site_sym))
        return fail(NRA_E_ARG, "sites or site_sym is NULL");
    if (group_off[0] != 0 || group_off[n_groups] != n_tracts)
        return fail(NRA_E_ARG, "group_off must run from 0 to n_tracts");
    for (int32_t g = 0; g < n_groups; ++g)
        if (group_off[g + 1] < group_off[g]) return fail(NRA_E_ARG, "group offsets must not decrease");
    if (n_tracts > 0) {
        if (!seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
        if (int rc = check_tract_offsets(n_tracts, seq_off, NRA_CONS_MAX_N, "tract")) return rc;
        if (seq_off[n_tracts] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (n_groups > 0) {
        if (int rc = check_tract_offsets(n_groups, bb_off, NRA_CONS_MAX_N, "backbone", "backbone")) return rc;
        if (bb_off[n_groups] > bb_off[0] && !backbones) return fail(NRA_E_ARG, "backbones is NULL");
        for (int64_t i = bb_off[0]; i < bb_off[n_groups]; ++i)
            if (kBase.of[(unsigned char)backbones[i]] > 3) return fail(NRA_E_ARG, "a backbone base is not A, C, G or T");
    }
    if (int rc = use_device(device, n_groups > 0)) return rc;
    int64_t st[NRA_SPLIT_N_STATS] = {0};
    site_off[0] = 0;
    sym_off[0] = 0;
    if (n_groups == 0) {
        if (stats) std::memcpy(stats, st, sizeof(st));
        return NRA_OK;
    }
    try {
        Host H;
        H.seq.resize((size_t)n_tracts);
        H.n.resize((size_t)n_tracts);
        H.row.assign((size_t)n_tracts, -1);
        int64_t code_bytes = 0;
        for (int32_t r = 0; r < n_tracts; ++r) {
            H.seq[r] = (uint64_t)code_bytes;
            H.n[r] = (int32_t)(seq_off[r + 1] - seq_off[r]);
            code_bytes += round_up(H.n[r], 16);
        }
        H.codes.assign((size_t)code_bytes + 16, (uint8_t)NRA_CONS_CODE_OTHER);
        for (int32_t r = 0; r < n_tracts; ++r) encode(H.codes.data() + H.seq[r], seqs + seq_off[r], H.n[r]);
        std::vector<NraSplitGroup> dg((size_t)n_groups);
        int64_t bb_bytes = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            const int64_t t = bb_off[g + 1] - bb_off[g], m = group_off[g + 1] - group_off[g];
            const int64_t k = std::min<int64_t>(max_sites, t);
            dg[g] = NraSplitGroup{(uint64_t)bb_bytes, (uint64_t)group_off[g], (uint64_t)H.col_total, (uint64_t)H.mat_bytes,
                                  (uint64_t)H.site_total, (int32_t)t, (int32_t)m, 0, (int32_t)group_off[g]};
            bb_bytes += round_up(t + 1, 16);
            H.col_total += t;
            H.mat_bytes += k * m;
            H.site_total += k;
            for (int64_t r = group_off[g]; r < group_off[g + 1]; ++r)
                if (std::abs((int64_t)H.n[r] - t) <= max_dist) {
                    H.row[r] = H.row_bytes;
                    H.row_bytes += round_up(t, 16);
                }
        }
        H.bbs.assign((size_t)bb_bytes, (uint8_t)NRA_CONS_CODE_PAD);
        for (int32_t g = 0; g < n_groups; ++g)
            for (int64_t i = 0; i < dg[g].t; ++i) H.bbs[dg[g].bb + i] = kBase.of[(unsigned char)backbones[bb_off[g] + i]];
        for (int32_t r = 0; r < n_tracts; ++r) dist[r] = -1;
        std::vector<int64_t> rowtab((size_t)n_tracts, -1);
        std::vector<int32_t> res, dsites;
        std::vector<uint8_t> mats;
        const NraSplitParams prm{min_count, min_share_pct, min_purity_pct, min_sites, max_sites, max_iter};
        const int rc = run(H, rowtab, n_tracts, group_off, max_dist, prm, dg, label, dist, res, dsites, mats, st);
        if (rc != NRA_OK) return rc;
        int64_t n_sites = 0, n_sym = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            n_sites += res[(size_t)g * NRA_SPLIT_RES_INTS + 5];
            n_sym += (int64_t)res[(size_t)g * NRA_SPLIT_RES_INTS + 5] * dg[g].m;
        }
        if (n_sites > site_cap || n_sym > sym_cap)
            return fail(NRA_E_RANGE, "the sites need " + std::to_string(n_sites) + " records and " + std::to_string(n_sym) +
                                         " symbols, site_cap is " + std::to_string(site_cap) + ", sym_cap " +
                                         std::to_string(sym_cap));
        int64_t so = 0, yo = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            const int32_t* r8 = res.data() + (size_t)g * NRA_SPLIT_RES_INTS;
            const int64_t S = r8[5];
            std::memcpy(group_res + (size_t)g * NRA_SPLIT_RES_INTS, r8, NRA_SPLIT_RES_INTS * sizeof(int32_t));
            if (S > 0) {
                std::memcpy(sites + so * NRA_SPLIT_SITE_INTS, dsites.data() + dg[g].site * NRA_SPLIT_SITE_INTS,
                            (size_t)S * NRA_SPLIT_SITE_INTS * sizeof(int32_t));
                std::memcpy(site_sym + yo, mats.data() + dg[g].mat, (size_t)(S * dg[g].m));
            }
            so += S;
            yo += S * dg[g].m;
            site_off[g + 1] = so;
            sym_off[g + 1] = yo;
            st[10] += S;
            st[15] += r8[0];
        }
        if (stats) std::memcpy(stats, st, sizeof(st));
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "allele split: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
