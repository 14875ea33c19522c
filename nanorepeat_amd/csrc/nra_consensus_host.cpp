// nra_consensus_host.cpp -- C ABI of the allele consensus (nra_tract_consensus): argument checks, the round-0
// backbones, and the rounds: per round the alignment launches of k_cons_align (by band class, tracts sorted by length,
// chunked under a budget of traceback pointer memory, repeated in the next class for the tracts whose band could not
// decide), one launch of k_cons_build, and the new backbones back (nra_consensus.hip).  The tracts are packed and
// uploaded once; groups that are done drop out of the next round.
#include "nra_cons_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;
using namespace nra_cons;

namespace {

struct Tract {
    uint64_t seq;              // byte offset of its codes on the device
    int32_t n;
    int32_t cls;               // the class that decided it in the round before, -1: none yet
};

struct Group {
    std::vector<int32_t> tracts;    // indices into the packed tracts (empty tracts dropped)
    std::vector<uint8_t> bb;
    std::vector<int32_t> sup;
    int32_t rounds = 0, conv = 0, voted = 0, left = 0;
    bool active = false;
};

struct Work {
    int32_t tract, slot, cls;
};

int run(int32_t n_groups, std::vector<Group>& groups, std::vector<Tract>& tracts, const std::vector<uint8_t>& codes,
        int max_dist, int max_rounds, int64_t* stats)
{
    const int64_t ptr_budget = nra_cons::ptr_budget();
    DevBuf<uint8_t> d_codes, d_bb, d_nb;
    DevBuf<NraConsGroup> d_groups;
    DevBuf<NraConsItem> d_items;
    DevBuf<uint4> d_ptr;
    DevBuf<int32_t> d_tabs, d_voters, d_status, d_sup, d_res;
    NRA_HIP_TRY(d_codes.ensure(codes.size()));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));

    std::vector<int32_t> act;
    std::vector<NraConsGroup> dg;
    std::vector<uint8_t> bbs, nbs;
    std::vector<int32_t> sups, res, status;
    std::vector<Work> work, next;
    std::vector<NraConsItem> items;
    for (int round = 1; round <= max_rounds; ++round) {
        act.clear();
        for (int32_t g = 0; g < n_groups; ++g)
            if (groups[g].active) act.push_back(g);
        if (act.empty()) break;
        stats[10] += 1;
        const size_t na = act.size();
        dg.assign(na, NraConsGroup{});
        int64_t bb_bytes = 0, nb_bytes = 0, tab_ints = 0;
        for (size_t a = 0; a < na; ++a) {
            const int64_t t = (int64_t)groups[act[a]].bb.size();
            dg[a].bb = (uint64_t)bb_bytes;
            dg[a].nb = (uint64_t)nb_bytes;
            dg[a].tab = (uint64_t)tab_ints;
            dg[a].t = (int32_t)t;
            bb_bytes += round_up(t + 1, 16);
            nb_bytes += round_up(2 * t + 2, 16);
            tab_ints += (t + 1) * NRA_CONS_TAB;
        }
        bbs.assign((size_t)bb_bytes, (uint8_t)NRA_CONS_CODE_PAD);
        for (size_t a = 0; a < na; ++a) {
            const Group& g = groups[act[a]];
            if (!g.bb.empty()) std::memcpy(bbs.data() + dg[a].bb, g.bb.data(), g.bb.size());
        }
        NRA_HIP_TRY(d_bb.ensure(bbs.size()));
        NRA_HIP_TRY(d_nb.ensure((size_t)nb_bytes));
        NRA_HIP_TRY(d_sup.ensure((size_t)nb_bytes));
        NRA_HIP_TRY(d_groups.ensure(na));
        NRA_HIP_TRY(d_tabs.ensure((size_t)tab_ints));
        NRA_HIP_TRY(d_voters.ensure(na));
        NRA_HIP_TRY(d_res.ensure(3 * na));
        NRA_HIP_TRY(hipMemcpy(d_bb.p, bbs.data(), bbs.size(), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_groups.p, dg.data(), na * sizeof(NraConsGroup), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemset(d_tabs.p, 0, (size_t)tab_ints * sizeof(int32_t)));
        NRA_HIP_TRY(hipMemset(d_voters.p, 0, na * sizeof(int32_t)));

        // the alignments of the round: every tract of every active group, in the class that decided it last time
        work.clear();
        for (size_t a = 0; a < na; ++a) {
            const int t = dg[a].t;
            for (int32_t r : groups[act[a]].tracts) {
                const int n = tracts[r].n, ad = std::abs(t - n);
                if (ad > max_dist) {              // the distance is at least |t - n|
                    stats[13] += 1;
                    continue;
                }
                int cls = tracts[r].cls;
                if (cls < 0 || proven(cls, n, t) < 0) cls = start_class(n, t, max_dist);
                tracts[r].cls = -1;
                work.push_back(Work{r, (int32_t)a, cls});
            }
        }
        while (!work.empty()) {
            std::sort(work.begin(), work.end(), [&](const Work& x, const Work& y) {
                if (x.cls != y.cls) return x.cls < y.cls;
                if (tracts[x.tract].n != tracts[y.tract].n) return tracts[x.tract].n > tracts[y.tract].n;
                return x.tract < y.tract;
            });
            next.clear();
            for (size_t i = 0; i < work.size();) {
                const int cls = work[i].cls, c = 1 << cls, rows_per_piece = 64 / c;
                items.clear();
                int64_t pieces = 0;
                size_t j = i;
                while (j < work.size() && work[j].cls == cls) {
                    const Tract& tr = tracts[work[j].tract];
                    const int64_t pc = (int64_t)((tr.n + rows_per_piece - 1) / rows_per_piece) * 64;
                    if (j > i && (pieces + pc) * 16 > ptr_budget) break;
                    items.push_back(NraConsItem{tr.seq, (uint64_t)pieces, tr.n, work[j].slot});
                    pieces += pc;
                    stats[cls] += 1;
                    stats[5 + cls] += tr.n;
                    ++j;
                }
                const size_t ni = items.size();
                stats[11] += 1;
                stats[14] = std::max<int64_t>(stats[14], pieces * 16);
                NRA_HIP_TRY(d_items.ensure(ni));
                NRA_HIP_TRY(d_status.ensure(ni));
                NRA_HIP_TRY(d_ptr.ensure((size_t)pieces));
                NRA_HIP_TRY(hipMemcpy(d_items.p, items.data(), ni * sizeof(NraConsItem), hipMemcpyHostToDevice));
                const int e = nra_launch_cons_align(nullptr, c, (int)ni, d_items.p, d_groups.p, d_codes.p, d_bb.p, d_ptr.p,
                                                    d_tabs.p, d_voters.p, d_status.p, max_dist);
                if (e != 0) return fail(NRA_E_DEVICE, std::string("k_cons_align: ") + hipGetErrorString((hipError_t)e));
                NRA_HIP_TRY(hipStreamSynchronize(nullptr));
                status.resize(ni);
                NRA_HIP_TRY(hipMemcpy(status.data(), d_status.p, ni * sizeof(int32_t), hipMemcpyDeviceToHost));
                for (size_t q = 0; q < ni; ++q) {
                    const Work& wk = work[i + q];
                    if (status[q] == NRA_CONS_WIDEN) {
                        if (cls + 1 >= NRA_CONS_CLASSES) return fail(NRA_E_DEVICE, "consensus: the widest band did not decide");
                        stats[12] += 1;
                        next.push_back(Work{wk.tract, wk.slot, cls + 1});
                    } else if (status[q] >= 0) {
                        tracts[wk.tract].cls = cls;
                    }
                }
                i = j;
            }
            work.swap(next);
        }

        const int e = nra_launch_cons_build(nullptr, (int)na, d_groups.p, d_bb.p, d_tabs.p, d_voters.p, d_nb.p, d_sup.p,
                                            d_res.p);
        if (e != 0) return fail(NRA_E_DEVICE, std::string("k_cons_build: ") + hipGetErrorString((hipError_t)e));
        NRA_HIP_TRY(hipStreamSynchronize(nullptr));
        res.resize(3 * na);
        nbs.resize((size_t)nb_bytes);
        sups.resize((size_t)nb_bytes);
        NRA_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(nbs.data(), d_nb.p, nbs.size(), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(sups.data(), d_sup.p, sups.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t a = 0; a < na; ++a) {
            Group& g = groups[act[a]];
            const int32_t len = res[3 * a], changed = res[3 * a + 1], mv = res[3 * a + 2];
            g.rounds = round;
            if (mv == 0) {
                g.conv = 0;
                g.voted = 0;
                g.left = (int32_t)g.tracts.size();
                g.active = false;
                continue;
            }
            g.bb.assign(nbs.begin() + dg[a].nb, nbs.begin() + dg[a].nb + len);
            g.sup.assign(sups.begin() + dg[a].nb, sups.begin() + dg[a].nb + len);
            g.voted = mv;
            g.left = (int32_t)g.tracts.size() - mv;
            if (!changed) {
                g.conv = 1;
                g.active = false;
            }
        }
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_tract_consensus(int device, int32_t n_groups, const int64_t* group_off, int32_t n_tracts, const char* seqs,
                        const int64_t* seq_off, int32_t max_dist, int32_t max_rounds, int64_t cons_cap,
                        char* consensus, int32_t* support, int64_t* cons_off, int32_t* group_res, int64_t* stats)
{
    if (n_groups < 0 || n_tracts < 0) return fail(NRA_E_ARG, "negative group or tract count");
    if (!group_off || !cons_off) return fail(NRA_E_ARG, "group_off or cons_off is NULL");
    if (n_groups > 0 && !group_res) return fail(NRA_E_ARG, "group_res is NULL");
    if (max_dist < 0) return fail(NRA_E_ARG, "max_dist must be >= 0");
    if (max_dist > NRA_CONS_MAX_DIST) return fail(NRA_E_RANGE, "max_dist is larger than 1000");
    if (max_rounds < 1) return fail(NRA_E_ARG, "max_rounds must be >= 1");
    if (max_rounds > NRA_CONS_MAX_ROUNDS) return fail(NRA_E_RANGE, "max_rounds is larger than 64");
    if (cons_cap < 0 || (cons_cap > 0 && (!consensus || !support))) return fail(NRA_E_ARG, "consensus or support is NULL");
    if (group_off[0] != 0 || group_off[n_groups] != n_tracts)
        return fail(NRA_E_ARG, "group_off must run from 0 to n_tracts");
    for (int32_t g = 0; g < n_groups; ++g)
        if (group_off[g + 1] < group_off[g]) return fail(NRA_E_ARG, "group offsets must not decrease");
    if (n_tracts > 0) {
        if (!seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
        if (int rc = check_tract_offsets(n_tracts, seq_off, NRA_CONS_MAX_N, "tract")) return rc;
        if (seq_off[n_tracts] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device, n_groups > 0)) return rc;
    int64_t st[NRA_CONS_N_STATS] = {0};
    cons_off[0] = 0;
    if (n_groups == 0) {
        if (stats) std::memcpy(stats, st, sizeof(st));
        return NRA_OK;
    }
    try {
        std::vector<Tract> tracts((size_t)n_tracts);
        int64_t code_bytes = 0;
        for (int32_t r = 0; r < n_tracts; ++r) {
            tracts[r].seq = (uint64_t)code_bytes;
            tracts[r].n = (int32_t)(seq_off[r + 1] - seq_off[r]);
            tracts[r].cls = -1;
            code_bytes += round_up(tracts[r].n, 16);
        }
        std::vector<uint8_t> codes((size_t)code_bytes + 16, (uint8_t)NRA_CONS_CODE_OTHER);
        for (int32_t r = 0; r < n_tracts; ++r) encode(codes.data() + tracts[r].seq, seqs + seq_off[r], tracts[r].n);
        std::vector<Group> groups((size_t)n_groups);
        bool any = false;
        for (int32_t g = 0; g < n_groups; ++g) {
            Group& G = groups[g];
            for (int64_t r = group_off[g]; r < group_off[g + 1]; ++r)
                if (tracts[r].n > 0) G.tracts.push_back((int32_t)r);
            if (G.tracts.empty()) continue;
            // round 0: the tract of median length, element (m - 1) / 2 of the order by (length, position)
            std::vector<int32_t> order(G.tracts);
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return tracts[a].n < tracts[b].n; });
            const Tract& med = tracts[order[(order.size() - 1) / 2]];
            for (int32_t i = 0; i < med.n; ++i)
                if (codes[med.seq + i] < 4) G.bb.push_back(codes[med.seq + i]);
            G.sup.assign(G.bb.size(), 0);
            G.active = true;
            any = true;
        }
        if (any) {
            const int rc = run(n_groups, groups, tracts, codes, max_dist, max_rounds, st);
            if (rc != NRA_OK) return rc;
        }
        int64_t total = 0;
        for (int32_t g = 0; g < n_groups; ++g) total += (int64_t)groups[g].bb.size();
        if (total > cons_cap)
            return fail(NRA_E_RANGE, "the consensuses need " + std::to_string(total) + " bases, cons_cap is " +
                                         std::to_string(cons_cap));
        int64_t o = 0;
        for (int32_t g = 0; g < n_groups; ++g) {
            const Group& G = groups[g];
            for (size_t i = 0; i < G.bb.size(); ++i) {
                consensus[o + (int64_t)i] = "ACGT"[G.bb[i] & 3];
                support[o + (int64_t)i] = G.sup[i];
            }
            o += (int64_t)G.bb.size();
            cons_off[g + 1] = o;
            group_res[4 * g] = G.rounds;
            group_res[4 * g + 1] = G.conv;
            group_res[4 * g + 2] = G.voted;
            group_res[4 * g + 3] = G.left;
        }
        if (stats) std::memcpy(stats, st, sizeof(st));
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "tract consensus: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
