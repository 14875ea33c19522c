// nra_flank_host.cpp -- C ABI of the flank haplotypes (nra_flank_phase): argument checks, the alignment launches of
// k_flank_align (one item per row and side; by band class, segments sorted by length, chunked under the budget of
// traceback pointer memory, repeated in the next class for the sides whose band could not decide: the split host's
// scheme), then one launch of k_flank_count and one of k_split_phase for all groups, and the results back with the
// device columns mapped to group columns (nra_flank.hip, nra_split.hip).
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
    int32_t seg, cls;                          // seg = 2 row + side
};

struct Host {
    std::vector<uint64_t> seq;                 // byte offset of a segment's codes
    std::vector<int32_t> n;                    // its length
    std::vector<int64_t> row;                  // byte offset of its side's part of the row
    std::vector<int32_t> group_of;             // of a row
    std::vector<uint64_t> bb;                  // byte offset of a side's codes, [2 g + side]
    std::vector<int32_t> t;                    // a side's columns
    std::vector<int32_t> lpad;                 // device column of a group's right side: round_up(tL, 16)
    std::vector<uint8_t> codes, bbs;
    int64_t row_bytes = 0, col_total = 0, mat_bytes = 0, site_total = 0;
};

// the band class a segment of n bases starts in: the smallest that proves min(max_dist, n / 32 + 8)
int flank_start_class(int n, int max_dist)
{
    const int want = std::min(max_dist, n / 32 + 8);
    int cls = 0;
    while (cls < NRA_CONS_CLASSES - 1 && 32 * (1 << cls) - 1 < want) ++cls;
    return cls;
}

int run(const Host& H, std::vector<int64_t>& rowtab, int32_t n_rows, int max_dist, int skip, const NraSplitParams& prm,
        std::vector<NraSplitGroup>& dg, int32_t* label, int32_t* dist, int32_t* end, std::vector<int32_t>& res,
        std::vector<int32_t>& sites, std::vector<uint8_t>& mats, int64_t* stats)
{
    const int64_t ptr_budget = nra_cons::ptr_budget();
    const size_t ng = dg.size();
    DevBuf<uint8_t> d_codes, d_bb, d_rows, d_ab, d_mats;
    DevBuf<NraSplitGroup> d_groups;
    DevBuf<NraFlankItem> d_items;
    DevBuf<NraSplitBlock> d_blocks;
    DevBuf<uint4> d_ptr;
    DevBuf<int64_t> d_rowtab;
    DevBuf<int32_t> d_status, d_nb, d_pos, d_key, d_labels, d_sites, d_res, d_lpad;
    NRA_HIP_TRY(d_codes.ensure(H.codes.size()));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, H.codes.data(), H.codes.size(), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_bb.ensure(H.bbs.size()));
    NRA_HIP_TRY(hipMemcpy(d_bb.p, H.bbs.data(), H.bbs.size(), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_rows.ensure((size_t)H.row_bytes));
    if (H.row_bytes > 0) NRA_HIP_TRY(hipMemset(d_rows.p, NRA_FLANK_SYM_NONE, (size_t)H.row_bytes));

    // ---- the pileup: every segment of at least one base
    std::vector<Work> work, next;
    std::vector<NraFlankItem> items;
    std::vector<int32_t> status;
    std::vector<uint8_t> aligned((size_t)n_rows, 0);
    for (int32_t q = 0; q < 2 * n_rows; ++q)
        if (H.n[q] > 0) work.push_back(Work{q, flank_start_class(H.n[q], max_dist)});
    while (!work.empty()) {
        std::sort(work.begin(), work.end(), [&](const Work& x, const Work& y) {
            if (x.cls != y.cls) return x.cls < y.cls;
            if (H.n[x.seg] != H.n[y.seg]) return H.n[x.seg] > H.n[y.seg];
            return x.seg < y.seg;
        });
        next.clear();
        for (size_t i = 0; i < work.size();) {
            const int cls = work[i].cls, c = 1 << cls, rows_per_piece = 64 / c;
            items.clear();
            int64_t pieces = 0;
            size_t j = i;
            while (j < work.size() && work[j].cls == cls) {
                const int32_t q = work[j].seg, side = 2 * H.group_of[q >> 1] + (q & 1);
                const int64_t pc = (int64_t)((H.n[q] + rows_per_piece - 1) / rows_per_piece) * 64;
                if (j > i && (pieces + pc) * 16 > ptr_budget) break;
                items.push_back(NraFlankItem{H.seq[q], (uint64_t)pieces, (uint64_t)H.row[q], H.bb[side], H.n[q], H.t[side]});
                pieces += pc;
                stats[cls] += 1;
                stats[5 + cls] += H.n[q];
                ++j;
            }
            const size_t ni = items.size();
            stats[11] += 1;
            stats[14] = std::max<int64_t>(stats[14], pieces * 16);
            NRA_HIP_TRY(d_items.ensure(ni));
            NRA_HIP_TRY(d_status.ensure(2 * ni));
            NRA_HIP_TRY(d_ptr.ensure((size_t)pieces));
            NRA_HIP_TRY(hipMemcpy(d_items.p, items.data(), ni * sizeof(NraFlankItem), hipMemcpyHostToDevice));
            const int e = nra_launch_flank_align(nullptr, c, (int)ni, d_items.p, d_codes.p, d_bb.p, d_ptr.p, d_rows.p,
                                                 d_status.p, max_dist);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_flank_align: ") + hipGetErrorString((hipError_t)e));
            NRA_HIP_TRY(hipStreamSynchronize(nullptr));
            status.resize(2 * ni);
            NRA_HIP_TRY(hipMemcpy(status.data(), d_status.p, 2 * ni * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < ni; ++q) {
                const Work& wk = work[i + q];
                const int32_t st = status[2 * q];
                if (st == NRA_CONS_WIDEN) {
                    if (cls + 1 >= NRA_CONS_CLASSES) return fail(NRA_E_DEVICE, "flank phase: the widest band did not decide");
                    stats[12] += 1;
                    next.push_back(Work{wk.seg, cls + 1});
                } else if (st >= 0) {
                    dist[wk.seg] = st;
                    end[wk.seg] = status[2 * q + 1];
                    aligned[wk.seg >> 1] = 1;
                }
            }
            i = j;
        }
        work.swap(next);
    }
    for (int32_t r = 0; r < n_rows; ++r)
        if (aligned[r]) {
            rowtab[r] = H.row[2 * r];
            dg[H.group_of[r]].mv += 1;
        }

    // ---- the sites, the haplotypes, the verdict
    std::vector<NraSplitBlock> blocks;
    for (size_t g = 0; g < ng; ++g)
        if (dg[g].mv > 0)
            for (int32_t c0 = 0; c0 < dg[g].t; c0 += NRA_SPLIT_THREADS) blocks.push_back(NraSplitBlock{(int32_t)g, c0});
    NRA_HIP_TRY(d_groups.ensure(ng));
    NRA_HIP_TRY(hipMemcpy(d_groups.p, dg.data(), ng * sizeof(NraSplitGroup), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_lpad.ensure(ng));
    NRA_HIP_TRY(hipMemcpy(d_lpad.p, H.lpad.data(), ng * sizeof(int32_t), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_rowtab.ensure((size_t)n_rows));
    if (n_rows > 0)
        NRA_HIP_TRY(hipMemcpy(d_rowtab.p, rowtab.data(), (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_blocks.ensure(blocks.size()));
    if (!blocks.empty())
        NRA_HIP_TRY(hipMemcpy(d_blocks.p, blocks.data(), blocks.size() * sizeof(NraSplitBlock), hipMemcpyHostToDevice));
    NRA_HIP_TRY(d_nb.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_ab.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_pos.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_key.ensure((size_t)H.col_total));
    NRA_HIP_TRY(d_mats.ensure((size_t)H.mat_bytes));
    NRA_HIP_TRY(d_labels.ensure((size_t)n_rows));
    NRA_HIP_TRY(d_sites.ensure((size_t)H.site_total * NRA_SPLIT_SITE_INTS));
    NRA_HIP_TRY(d_res.ensure(ng * NRA_SPLIT_RES_INTS));
    int e = nra_launch_flank_count(nullptr, (int)blocks.size(), d_blocks.p, d_groups.p, d_lpad.p, d_rowtab.p, d_rows.p, prm,
                                   skip, d_nb.p, d_ab.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_flank_count: ") + hipGetErrorString((hipError_t)e));
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
    if (n_rows > 0) NRA_HIP_TRY(hipMemcpy(label, d_labels.p, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_flank_phase(int device, int32_t n_groups, const int64_t* group_off, int32_t n_rows, const char* segs,
                    const int64_t* seg_off, const char* backbones, const int64_t* bb_off, int32_t max_dist, int32_t skip,
                    int32_t min_count, int32_t min_share_pct, int32_t min_purity_pct, int32_t min_sites,
                    int32_t max_sites, int32_t max_iter, int32_t* label, int32_t* dist, int32_t* end,
                    int32_t* group_res, int64_t site_cap, int32_t* sites, int64_t* site_off, int64_t sym_cap,
                    uint8_t* site_sym, int64_t* sym_off, int64_t* stats)
{
    if (n_groups < 0 || n_rows < 0) return fail(NRA_E_ARG, "negative group or row count");
    if (n_groups > (1 << 29) || n_rows > (1 << 29)) return fail(NRA_E_RANGE, "too many groups or rows");
    if (!group_off || !site_off || !sym_off) return fail(NRA_E_ARG, "group_off, site_off or sym_off is NULL");
    if (n_groups > 0 && (!group_res || !bb_off)) return fail(NRA_E_ARG, "group_res or bb_off is NULL");
    if (n_rows > 0 && (!label || !dist || !end)) return fail(NRA_E_ARG, "label, dist or end is NULL");
    if (max_dist < 0) return fail(NRA_E_ARG, "max_dist must be >= 0");
    if (max_dist > NRA_FLANK_MAX_DIST) return fail(NRA_E_RANGE, "max_dist is larger than 500");
    if (skip < 0) return fail(NRA_E_ARG, "skip must be >= 0");
    if (min_count < 1 || min_sites < 1) return fail(NRA_E_ARG, "min_count and min_sites must be >= 1");
    if (min_share_pct < 1 || min_purity_pct < 1) return fail(NRA_E_ARG, "percentages must be >= 1");
    if (min_share_pct > 100 || min_purity_pct > 100) return fail(NRA_E_RANGE, "a percentage is larger than 100");
    if (max_sites < 1 || max_iter < 1) return fail(NRA_E_ARG, "max_sites and max_iter must be >= 1");
    if (max_sites > NRA_SPLIT_MAX_SITES) return fail(NRA_E_RANGE, "max_sites is larger than 4096");
    if (max_iter > NRA_SPLIT_MAX_ITER) return fail(NRA_E_RANGE, "max_iter is larger than 64");
    if (site_cap < 0 || sym_cap < 0 || (site_cap > 0 && !sites) || (sym_cap > 0 && !site_sym))
        return fail(NRA_E_ARG, "sites or site_sym is NULL");
    if (group_off[0] != 0 || group_off[n_groups] != n_rows) return fail(NRA_E_ARG, "group_off must run from 0 to n_rows");
    for (int32_t g = 0; g < n_groups; ++g)
        if (group_off[g + 1] < group_off[g]) return fail(NRA_E_ARG, "group offsets must not decrease");
    if (n_rows > 0) {
        if (!seg_off) return fail(NRA_E_ARG, "seg_off is NULL");
        if (int rc = check_tract_offsets(2 * n_rows, seg_off, NRA_CONS_MAX_N, "segment", "segment")) return rc;
        if (seg_off[2 * n_rows] > seg_off[0] && !segs) return fail(NRA_E_ARG, "segs is NULL");
    }
    if (n_groups > 0) {
        if (int rc = check_tract_offsets(2 * n_groups, bb_off, NRA_CONS_MAX_N, "backbone", "backbone side")) return rc;
        if (bb_off[2 * n_groups] > bb_off[0] && !backbones) return fail(NRA_E_ARG, "backbones is NULL");
        for (int64_t i = bb_off[0]; i < bb_off[2 * n_groups]; ++i)
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
        const int32_t n_segs = 2 * n_rows;
        H.seq.resize((size_t)n_segs);
        H.n.resize((size_t)n_segs);
        H.row.assign((size_t)n_segs, 0);
        H.group_of.resize((size_t)n_rows);
        int64_t code_bytes = 0;
        for (int32_t q = 0; q < n_segs; ++q) {
            H.seq[q] = (uint64_t)code_bytes;
            H.n[q] = (int32_t)(seg_off[q + 1] - seg_off[q]);
            code_bytes += round_up(H.n[q], 16);
        }
        H.codes.assign((size_t)code_bytes + 16, (uint8_t)NRA_CONS_CODE_OTHER);
        for (int32_t q = 0; q < n_segs; ++q) encode(H.codes.data() + H.seq[q], segs + seg_off[q], H.n[q]);
        std::vector<NraSplitGroup> dg((size_t)n_groups);
        H.bb.resize(2 * (size_t)n_groups);
        H.t.resize(2 * (size_t)n_groups);
        H.lpad.resize((size_t)n_groups);
        int64_t bb_bytes = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            const int64_t tl = bb_off[2 * g + 1] - bb_off[2 * g], tr = bb_off[2 * g + 2] - bb_off[2 * g + 1];
            const int64_t lpad = round_up(tl, 16), td = lpad + tr, m = group_off[g + 1] - group_off[g];
            const int64_t k = std::min<int64_t>(max_sites, tl + tr);
            H.t[2 * g] = (int32_t)tl;
            H.t[2 * g + 1] = (int32_t)tr;
            H.lpad[g] = (int32_t)lpad;
            H.bb[2 * g] = (uint64_t)bb_bytes;
            bb_bytes += round_up(tl + 1, 16);
            H.bb[2 * g + 1] = (uint64_t)bb_bytes;
            bb_bytes += round_up(tr + 1, 16);
            dg[g] = NraSplitGroup{0, (uint64_t)group_off[g], (uint64_t)H.col_total, (uint64_t)H.mat_bytes,
                                  (uint64_t)H.site_total, (int32_t)td, (int32_t)m, 0, (int32_t)group_off[g]};
            H.col_total += td;
            H.mat_bytes += k * m;
            H.site_total += k;
            for (int64_t r = group_off[g]; r < group_off[g + 1]; ++r) {
                H.group_of[r] = g;
                H.row[2 * r] = H.row_bytes;
                H.row[2 * r + 1] = H.row_bytes + lpad;
                H.row_bytes += round_up(td, 16);
            }
        }
        H.bbs.assign((size_t)bb_bytes, (uint8_t)NRA_CONS_CODE_PAD);
        for (int32_t s = 0; s < 2 * n_groups; ++s)
            for (int64_t i = 0; i < H.t[s]; ++i) H.bbs[H.bb[s] + i] = kBase.of[(unsigned char)backbones[bb_off[s] + i]];
        for (int32_t q = 0; q < n_segs; ++q) {
            dist[q] = H.n[q] > 0 ? -1 : -2;
            end[q] = 0;
        }
        std::vector<int64_t> rowtab((size_t)n_rows, -1);
        std::vector<int32_t> res, dsites;
        std::vector<uint8_t> mats;
        const NraSplitParams prm{min_count, min_share_pct, min_purity_pct, min_sites, max_sites, max_iter};
        const int rc = run(H, rowtab, n_rows, max_dist, skip, prm, dg, label, dist, end, res, dsites, mats, st);
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
                const int32_t shift = H.lpad[g] - H.t[2 * g];     // device column -> group column on the right side
                for (int64_t q = so; q < so + S; ++q)
                    if (sites[q * NRA_SPLIT_SITE_INTS] >= H.lpad[g]) sites[q * NRA_SPLIT_SITE_INTS] -= shift;
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
        return fail(NRA_E_NOMEM, "flank phase: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
