// nra_plan2d.cpp -- the plan of a joint (2D) cell list (nra_plan2d.h), in the order set_cells_common runs its two stages,
// the plans of the flank sweeps ahead of a list and of a refinement, and the digest of a sequence of such steps.
// Host only: no hip* call, no getenv.
#include "nra_plan2d.h"

#include <cmath>

namespace {

int fail(int code, const std::string& msg) { return nra_set_error(code, msg.c_str()); }

// first index i in [0, count] with start + i * step >= x  (numpy.searchsorted(grid, x, side="left") on the grid values)
int32_t grid_lower_bound(int32_t start, int32_t step, int32_t count, double x)
{
    if (count <= 0) return 0;
    double f = std::ceil((x - (double)start) / (double)step);
    int64_t i = f < 0 ? 0 : (f > (double)count ? count : (int64_t)f);
    while (i > 0 && (double)start + (double)(i - 1) * step >= x) --i;           // rounding of the quotient
    while (i < count && (double)start + (double)i * step < x) ++i;
    return (int32_t)i;
}

}  // namespace

int route_grid(int32_t n_reads, int32_t start1, int32_t step1, int32_t count1, const double* lo1, const double* hi1,
               int32_t start2, int32_t step2, int32_t count2, const double* lo2, const double* hi2,
               std::vector<GridRow>& rows, int64_t& n_cells, std::vector<GridRow>* keep)
{
    if (n_reads < 0 || step1 <= 0 || step2 <= 0 || count1 < 0 || count2 < 0 || start1 < 0 || start2 < 0)
        return fail(NRA_E_ARG, "bad grid (steps > 0, starts and counts >= 0)");
    if (n_reads > 0 && (!lo1 || !hi1 || !lo2 || !hi2)) return fail(NRA_E_ARG, "NULL grid bound array");
    if ((int64_t)start1 + (int64_t)step1 * count1 > 0x3fffffff || (int64_t)start2 + (int64_t)step2 * count2 > 0x3fffffff)
        return fail(NRA_E_RANGE, "grid values too large");
    rows.assign((size_t)n_reads, GridRow{0, 0, 0, 0});
    n_cells = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (!(lo1[r] < hi1[r]) || !(lo2[r] < hi2[r])) continue;         // (also drops NaN bounds)
        const int32_t a1 = grid_lower_bound(start1, step1, count1, lo1[r]), b1 = grid_lower_bound(start1, step1, count1, hi1[r]);
        const int32_t a2 = grid_lower_bound(start2, step2, count2, lo2[r]), b2 = grid_lower_bound(start2, step2, count2, hi2[r]);
        if (b1 <= a1 || b2 <= a2) continue;
        rows[(size_t)r] = GridRow{start1 + a1 * step1, b1 - a1, start2 + a2 * step2, b2 - a2};
        n_cells += (int64_t)(b1 - a1) * (b2 - a2);
    }
    if (keep) {
        // What a finer grid inside the same bounds can ask of a read: every count k with lo <= k < hi -- and, the way the
        // reference refines (within one coarse step of a size between the coarse grid's first and last value), nothing
        // more than one step below the first or above the last of the read's values.  A unit-step axis keeps its own.
        keep->assign((size_t)n_reads, GridRow{0, 0, 0, 0});
        auto span = [](int32_t first, int32_t n, int32_t step, double lo, double hi, int32_t& a, int32_t& count) {
            const int32_t last = first + (n - 1) * step;
            int64_t ka = first, kb = last;
            if (step > 1) {
                const double cl = std::ceil(lo), ch = std::ceil(hi);
                const int64_t klo = cl < 0 ? 0 : (cl > 1e9 ? (int64_t)1e9 : (int64_t)cl);
                const int64_t khi = ch > 1e9 ? (int64_t)1e9 : (int64_t)ch - 1;
                ka = std::max<int64_t>(std::max<int64_t>(klo, (int64_t)first - step), 0);
                kb = std::min<int64_t>(khi, (int64_t)last + step - 1);
                ka = std::min<int64_t>(ka, first); kb = std::max<int64_t>(kb, last);
            }
            a = (int32_t)ka; count = (int32_t)(kb - ka + 1);
        };
        for (int32_t r = 0; r < n_reads; ++r) {
            const GridRow& g = rows[(size_t)r];
            if (g.n1 <= 0 || g.n2 <= 0) continue;
            GridRow& k = (*keep)[(size_t)r];
            span(g.k1lo, g.n1, step1, lo1[r], hi1[r], k.k1lo, k.n1);
            span(g.k2lo, g.n2, step2, lo2[r], hi2[r], k.k2lo, k.n2);
        }
    }
    return NRA_OK;
}

// ---- what is fixed when the reads are packed ----------------------------------------------------
void plan_2d_reads(const std::vector<NraDevRead>& reads, int32_t left_len, int32_t right_len, const nra_scoring_t* sc,
                   int32_t flags, Reads2D& out)
{
    const int32_t n_reads = (int32_t)reads.size();
    // Reads longer than one register block (3072 bases), or whose scores do not fit the int32 cells of the
    // joint sweeps, are scored cell by cell in chained row blocks with int64 cells (rare: a long amplicon).
    out.chained_reads.assign((size_t)n_reads, 0);
    for (int32_t r = 0; r < n_reads; ++r)
        out.chained_reads[r] = reads[r].qlen > NRA_MAX_QLEN_1BLOCK || max_score(sc, reads[r].qlen) > kScoreCapPk16;
    // rows-per-lane bucket of every read (measured on config 3, 5000 reads, R = 13..28: folding buckets of
    // fewer than 2048 reads into the next within 4 rows beats (1024, 2) and wider spans), and its partner
    std::vector<std::vector<int32_t>> by_bucket((size_t)kNumR);
    for (int32_t r = 0; r < n_reads; ++r)
        if (reads[r].qlen > 0 && !out.chained_reads[r]) by_bucket[rows_for_qlen(reads[r].qlen)].push_back(r);
    fold_small_buckets(by_bucket, 2048, 4);
    out.jbucket.assign((size_t)n_reads, -1);
    out.jpair_of.assign((size_t)n_reads, -1);
    out.jpairs.clear();
    uint64_t ints = 0;
    for (int bi = 0; bi < kNumR; ++bi) {
        const auto& v = by_bucket[bi];
        for (size_t i = 0; i < v.size(); i += 2) {
            NraJointPairTask t{};
            t.read_a = v[i]; t.read_b = i + 1 < v.size() ? v[i + 1] : -1;
            t.state = ints;
            ints += (uint64_t)NRA_JOINT_NPSTATE(kRList[bi]) * 64;
            out.jpair_of[t.read_a] = (int32_t)out.jpairs.size();
            if (t.read_b >= 0) out.jpair_of[t.read_b] = (int32_t)out.jpairs.size();
            out.jpairs.push_back(t);
        }
        for (int32_t r : v) out.jbucket[r] = bi;
    }
    // the packed cells hold what the 1D sweeps hold (nra_pk16.h), without the doubling of the origin bit
    const int o1 = sc->gap_open1 + sc->gap_ext1, o2 = sc->gap_open2 + sc->gap_ext2;
    const bool fits = o1 >= sc->mismatch && o1 >= sc->sc_ambi && sc->match + o1 <= 127 && sc->gap_ext1 <= 256 &&
                      sc->gap_ext2 <= 256 && o2 + sc->mismatch + sc->sc_ambi <= 700 &&
                      (flags & (NRA_F_BRUTE_FORCE | NRA_F_NO_JOINT_PACK)) == 0 && ints * 4 <= (4ull << 30);
    auto cols_ok = [&](int64_t flank) {
        const int64_t c = NRA_JOINT_PACKED_COLS(flank);
        return c >= NRA_JOINT_PACKED_MIN_COLS && max_score(sc, std::min<int64_t>(c, NRA_MAX_QLEN_1BLOCK)) <= 27000;
    };
    out.jpack_l = fits && ints > 0 && cols_ok(left_len);
    out.jpack_r = fits && ints > 0 && cols_ok(right_len);
    out.jpack_ints = ints;
}

void commit_2d(Carried2D& cd, Pending2D& pd)
{
    for (const auto& pr2 : pd.rev) cd.rev_strand[(size_t)pr2.first] = pr2.second;
    pd.rev.clear();
    for (const auto& pr2 : pd.lst) cd.lst_strand[(size_t)pr2.first] = pr2.second;
    pd.lst.clear();
    for (const auto& pr2 : pd.rpk) cd.rpk_strand[(size_t)pr2.first] = pr2.second;
    pd.rpk.clear();
    if (pd.keep) { cd.keep_valid = true; pd.keep = false; }      // ... and so do the column states
}

// ---- the plan of one list -----------------------------------------------------------------------
namespace {

const int kChainBucket = kNumR;

// what the steps of a plan share
struct Ctx {
    const Reads2D& rd;
    const Cells2D& cl;
    Carried2D& cd;
    Pending2D* pd;             // stage 1 only
    Plan2D& p;
    int32_t flags;
    int colsL, colsR;
    int32_t n_reads() const { return (int32_t)p.cnt.size(); }
    const NraDevRegion& d() const { return p.dregs[0]; }
    // k1 / k2 of a read's i-th listed cell
    int32_t k1_of(int32_t r, uint32_t i) const
    {
        if (!cl.grid) return cl.cell_k1[p.first[r] + i];
        const GridRow& g = cl.grid->rows[(size_t)r];
        return g.k1lo + (int32_t)(i / (uint32_t)g.n2) * cl.grid->step1;
    }
    int32_t k2_of(int32_t r, uint32_t i) const
    {
        if (!cl.grid) return cl.cell_k2[p.first[r] + i];
        const GridRow& g = cl.grid->rows[(size_t)r];
        return g.k2lo + (int32_t)(i % (uint32_t)g.n2) * cl.grid->step2;
    }
    bool swept(int32_t r) const { return p.cnt[r] > 0 && p.reads[r].qlen > 0 && !rd.chained_reads[r]; }
};

int count_cells(const Cells2D& cl, int32_t n_reads, Plan2D& p)
{
    std::vector<uint32_t>& first = p.first;
    std::vector<uint32_t>& cnt = p.cnt;
    first.assign((size_t)n_reads, 0); cnt.assign((size_t)n_reads, 0);
    int32_t k1max = 0, k2max = 0;
    if (cl.grid) {
        uint32_t c = 0;
        for (int32_t r = 0; r < n_reads; ++r) {
            const GridRow& g = cl.grid->rows[(size_t)r];
            first[r] = c; cnt[r] = (uint32_t)g.n1 * (uint32_t)g.n2;
            c += cnt[r];
            if (cnt[r]) {
                k1max = std::max(k1max, g.k1lo + (g.n1 - 1) * cl.grid->step1);
                k2max = std::max(k2max, g.k2lo + (g.n2 - 1) * cl.grid->step2);
            }
        }
    } else
    for (int64_t c = 0; c < cl.n_cells; ++c) {
        const int32_t r = cl.cell_read[c];
        if (r < 0 || r >= n_reads || (c > 0 && r < cl.cell_read[c - 1]) || cl.cell_k1[c] < 0 || cl.cell_k2[c] < 0)
            return fail(NRA_E_ARG, "cells must be grouped by read, k >= 0");
        if (cnt[r] == 0) first[r] = (uint32_t)c;
        cnt[r]++;
        k1max = std::max(k1max, cl.cell_k1[c]);
        k2max = std::max(k2max, cl.cell_k2[c]);
    }
    p.k1max = k1max; p.k2max = k2max;
    return NRA_OK;
}

// ---- Kept column states (routed grids with every strand given, MID scans).  A grid's sweeps leave a column state at
// every repeat count a finer grid inside the same bounds can ask for (grid->keep), not only at its own values: such a
// later grid -- the reference's round 3 after round 2 -- then needs no flank, prefix or reverse sweep at all, only
// the MID scans and the combine.  joint_keep: 0 = nothing kept, 1 = this list sweeps and keeps, 2 = no sweeps.
void decide_keep(Ctx& c, const Region2D& reg, const KeepInputs& ki)
{
    Plan2D& p = c.p;
    Carried2D& cd = c.cd;
    const JointGrid* grid = c.cl.grid;
    const int8_t* read_strand = c.cl.read_strand;
    const int32_t n_reads = c.n_reads();
    const int32_t left_len = (int32_t)reg.left.size(), unit1_len = (int32_t)reg.unit1.size(), mid_len = (int32_t)reg.mid.size(),
                  unit2_len = (int32_t)reg.unit2.size(), right_len = (int32_t)reg.right.size();
    int32_t k1max_pool = p.k1max, k2max_pool = p.k2max;
    int keep = 0;
    uint64_t keep_bytes = 0;
    if (grid && grid->keep && !p.brute && p.all_strands_given && c.cl.n_cells > 0 &&
        (c.flags & (NRA_F_JOINT_TAILS | NRA_F_JOINT_NO_CHAIN | NRA_F_JOINT_NO_KEEP)) == 0) {
        bool reuse = cd.keep_valid && cd.keep_rows.size() == (size_t)n_reads;
        for (int32_t r = 0; reuse && r < n_reads; ++r) {
            if (!c.swept(r)) continue;
            const GridRow& g = grid->rows[(size_t)r];
            const NraGridRow& k = cd.keep_rows[(size_t)r];
            if (cd.keep_strand[(size_t)r] != read_strand[r] || k.n1 <= 0 || k.n2 <= 0 || g.k1lo < k.k1lo ||
                g.k1lo + (g.n1 - 1) * grid->step1 > k.k1lo + k.n1 - 1 || g.k2lo < k.k2lo ||
                g.k2lo + (g.n2 - 1) * grid->step2 > k.k2lo + k.n2 - 1)
                reuse = false;
        }
        if (reuse) {
            keep = 2;
            // a refinement may follow (nra_batch2d_refine): its MID scans read the template up to the last kept count
            for (int32_t r = 0; r < n_reads; ++r)
                if (c.swept(r)) {
                    const NraGridRow& k = cd.keep_rows[(size_t)r];
                    k1max_pool = std::max(k1max_pool, k.k1lo + k.n1 - 1); k2max_pool = std::max(k2max_pool, k.k2lo + k.n2 - 1);
                }
        } else {
            uint64_t bytes = 0;
            int32_t k1hi = p.k1max, k2hi = p.k2max;
            for (int32_t r = 0; r < n_reads; ++r) {
                if (!c.swept(r)) continue;
                const GridRow& k = grid->keep[(size_t)r];
                bytes += ((uint64_t)k.n1 * NRA_JOINT_NSTATE(kRList[c.rd.jbucket[r]]) + (uint64_t)k.n2 * 3 * kRList[c.rd.jbucket[r]]) * 256;
                k1hi = std::max(k1hi, k.k1lo + k.n1 - 1); k2hi = std::max(k2hi, k.k2lo + k.n2 - 1);
            }
            const int64_t tl_keep = (int64_t)left_len + (int64_t)unit1_len * k1hi + mid_len + (int64_t)unit2_len * k2hi + right_len;
            // ... within the budget, and within half of what the device has left (what the arena holds already counts as free)
            // (NRA_JOINT_KEEP_BUDGET_GB in the environment overrides the built-in budget; 0 keeps nothing)
            bool fits = bytes <= ki.budget && tl_keep <= NRA_MAX_TLEN && !ki.keep_off;
            keep_bytes = bytes;
            if (fits) {
                uint64_t free_b = 0;
                if (bytes > ki.held) {
                    p.device_asked = true;
                    fits = ki.device_free(free_b) && bytes - ki.held <= free_b / 2;
                }
            }
            if (fits) { keep = 1; k1max_pool = k1hi; k2max_pool = k2hi; }
        }
    }
    if (keep != 2) cd.keep_valid = false;       // what was kept is replaced (1) or not looked at again (0)
    c.pd->keep = keep == 1;
    p.keep = keep; p.keep_bytes = keep_bytes; p.k1max_pool = k1max_pool; p.k2max_pool = k2max_pool;
    if (keep == 1) {
        cd.keep_rows.assign(grid->keep, grid->keep + n_reads);
        cd.keep_strand.assign(read_strand, read_strand + n_reads);
        cd.keep_state_off.assign((size_t)n_reads, 0);
        cd.keep_rs_off.assign((size_t)n_reads, 0);
        cd.keep_ra_off.assign((size_t)n_reads, 0);
    }
}

void build_pool(const Region2D& reg, bool reads_have_n, Plan2D& p)
{
    const int32_t left_len = (int32_t)reg.left.size(), unit1_len = (int32_t)reg.unit1.size(), mid_len = (int32_t)reg.mid.size(),
                  unit2_len = (int32_t)reg.unit2.size(), right_len = (int32_t)reg.right.size();
    std::vector<uint8_t>& pool = p.pool;
    bool has_n = reads_have_n;
    NraDevRegion d{};
    d.p1_off = pool_append(pool, reg.left.data(), left_len, reg.unit1.data(), unit1_len, p.k1max_pool, has_n);
    d.p2_off = pool_append(pool, reg.mid.data(), mid_len, reg.unit2.data(), unit2_len, p.k2max_pool, has_n);
    d.p3_off = pool_append(pool, reg.right.data(), right_len, nullptr, 0, 0, has_n);
    {   // rev(R) + rev(u2)^k2max: the reverse sweeps (the extended ones run on into the second repeat)
        std::string rr(reg.right), ru(reg.unit2);
        std::reverse(rr.begin(), rr.end());
        std::reverse(ru.begin(), ru.end());
        d.pr_off = pool_append(pool, rr.data(), right_len, ru.data(), unit2_len, p.k2max_pool, has_n);
    }
    d.l1 = left_len; d.m1 = unit1_len; d.l2 = mid_len; d.m2 = unit2_len; d.l3 = right_len;
    pool.push_back(0);
    p.has_n = has_n;
    p.dregs.assign(1, d);
}

// resume != 0: the first NRA_JOINT_PACKED_COLS columns were swept by k_joint_pk16, the wave state it left is the pair's
void resume_packed(NraJointTask& t, const NraJointPairTask& pair, int32_t r)
{
    t.resume = 1; t.pstate = pair.state; t.phalf = pair.read_b == r ? 1 : 0;
}

// the packed sweep of rev(R) up to the window: once per pair and strand, kept for later cell lists
void packed_r(Ctx& c, Bucket& bk, int32_t pi)
{
    Plan2D& p = c.p;
    const int8_t* read_strand = c.cl.read_strand;
    const NraJointPairTask& pair = c.rd.jpairs[(size_t)pi];
    if (p.pair_r[pi]) return;
    bool need = false;
    for (int32_t q : {pair.read_a, pair.read_b})
        if (q >= 0 && (read_strand == nullptr || read_strand[q] == 0 || c.cd.rpk_strand[q] != read_strand[q])) need = true;
    if (!need) return;
    p.pair_r[pi] = 1; p.jrpk.push_back(pair); bk.cells_sweep += (int64_t)2 * 64 * bk.R * c.colsR;
    for (int32_t q : {pair.read_a, pair.read_b}) {
        if (q < 0) continue;
        c.cd.rpk_strand[q] = 0;
        c.pd->rpk.push_back({q, read_strand ? read_strand[q] : (int8_t)0});
    }
}

// the sweeps of one read that depend on the read and its strand only
void strand_sweeps(Ctx& c, Bucket& bk, int32_t r)
{
    Plan2D& p = c.p;
    Carried2D& cd = c.cd;
    const NraDevRegion& d = c.d();
    const JointGrid* grid = c.cl.grid;
    const int8_t* read_strand = c.cl.read_strand;
    const int keep = p.keep;
    // one reverse sweep over R per read and strand, kept for later cell lists of the batch
    const int8_t given = read_strand ? read_strand[r] : 0;
    const int32_t pi = c.rd.jpair_of[r];
    const NraJointPairTask& pair = c.rd.jpairs[(size_t)pi];
    const bool stale = given == 0 || cd.rev_strand[r] != given;     // nothing kept for this read and strand
    if (keep == 2) {
        // every column state this list needs was kept: no sweep on either side
        p.rs_off[(size_t)r] = cd.keep_rs_off[(size_t)r]; p.ra_off[(size_t)r] = cd.keep_ra_off[(size_t)r];
    } else if (p.joint_v2) {
        // the reverse sweep runs on over rev(u2)^k2hi and leaves a column state per k2 of the read (of its
        // kept range, keep == 1); the packed sweep of rev(R) up to the window is kept in any case
        const GridRow& gr = grid->rows[(size_t)r];
        const int32_t k2lo = keep == 1 ? grid->keep[(size_t)r].k2lo : gr.k2lo, k2n = keep == 1 ? grid->keep[(size_t)r].n2 : gr.n2,
                      k2step = keep == 1 ? 1 : grid->step2;
        NraJointTask tb{}; tb.read = r; tb.k2lo = k2lo; tb.k2step = k2step; tb.n2 = k2n;
        tb.state = p.rs_total; tb.out = (int32_t)p.ra_total;
        p.rs_off[(size_t)r] = p.rs_total; p.ra_off[(size_t)r] = (int32_t)p.ra_total;
        if (keep == 1) { cd.keep_rs_off[(size_t)r] = p.rs_total; cd.keep_ra_off[(size_t)r] = (int32_t)p.ra_total; }
        p.rs_total += (uint64_t)k2n * 3 * 64 * (uint64_t)bk.R; p.ra_total += k2n;
        if (c.rd.jpack_r) {
            resume_packed(tb, pair, r);
            packed_r(c, bk, pi);
        }
        p.jbwd.push_back(tb);
        bk.cells_sweep += joint_cells(bk.R, d.l3 - (c.rd.jpack_r ? c.colsR : 0) + d.m2 * (k2lo + k2step * (k2n - 1)), p.reads[r].qlen);
        if (stale) { cd.rev_strand[r] = 0; c.pd->rev.push_back({r, given}); }
    } else if (stale) {
        NraJointTask tb{}; tb.read = r; tb.k2step = 1; tb.n2 = 1;
        if (c.rd.jpack_r) {
            resume_packed(tb, pair, r);
            packed_r(c, bk, pi);
        }
        p.jbwd.push_back(tb);
        bk.cells_sweep += joint_cells(bk.R, d.l3 - (c.rd.jpack_r ? c.colsR : 0), p.reads[r].qlen);
        cd.rev_strand[r] = 0;
        c.pd->rev.push_back({r, given});
    }
    // the L side up to the window: swept once per pair and strand, kept for later cell lists
    if (keep != 2 && c.rd.jpack_l && (given == 0 || cd.lst_strand[r] != given) && !p.pair_l[pi]) {
        p.pair_l[pi] = 1; p.jlpk.push_back(pair); bk.cells_sweep += (int64_t)2 * 64 * bk.R * c.colsL;
        for (int32_t q : {pair.read_a, pair.read_b}) {
            if (q < 0) continue;
            cd.lst_strand[q] = 0;
            c.pd->lst.push_back({q, read_strand ? read_strand[q] : (int8_t)0});
        }
    }
}

// ---- part 1: what depends on the reads and their strands only -- the reverse sweeps over R and the packed
// sweeps of the flanks outside the scoring window -- plus the strand probes.  With every strand given these
// kernels are enqueued right here, before the (longer) list of prefix and tail sweeps is built and uploaded:
// the host's share of a round then runs beside the device's first third of it.
void strand_bucket(Ctx& c, int bi)
{
    Plan2D& p = c.p;
    const NraDevRegion& d = c.d();
    Bucket bk;
    bk.chain = bi == kChainBucket;
    bk.R = bk.chain ? NRA_CHAIN_R : kRList[bi];
    bk.pair_off = p.pair_tasks.size();
    bk.jbwd_off = p.jbwd.size();
    bk.jlpk_off = p.jlpk.size(); bk.jrpk_off = p.jrpk.size();
    bk.probe_off = p.probe_tasks.size();
    const bool per_cell = p.brute || bk.chain;      // one DP per (read, cell) instead of the joint sweeps
    for (int32_t r : p.by_bucket[bi]) {
        if (!per_cell) strand_sweeps(c, bk, r);
        // strand probe against the read's first listed cell: half A = template, half B = its revcomp
        // (no probe runs when every strand is given)
        if (!bk.chain) {
            if (!p.all_strands_given) {
                NraPairTask t{};
                t.read = r; t.k1a = t.k1b = c.k1_of(r, 0); t.k2a = t.k2b = c.k2_of(r, 0);
                t.out_a = 2 * r; t.out_b = 2 * r + 1; t.flags = 3;     // B = reverse complement; raw scores
                p.pair_tasks.push_back(t);
                bk.cells_pair += 2 * sweep_cells(bk.R, d.l1 + d.m1 * t.k1a + d.l2 + d.m2 * t.k2a + d.l3);
            }
        } else {
            // chained: the read and a reverse-complemented shadow of it against the same template
            NraDevRead shadow = p.reads[r];
            shadow.rc = 1;
            const int32_t sh = (int32_t)p.reads.size();
            p.reads.push_back(shadow);
            p.probe_tasks.push_back(NraTask{r, c.k1_of(r, 0), c.k2_of(r, 0), 2 * r});
            p.probe_tasks.push_back(NraTask{sh, c.k1_of(r, 0), c.k2_of(r, 0), 2 * r + 1});
        }
    }
    bk.n_pair = (int)(p.pair_tasks.size() - bk.pair_off);
    bk.n_jbwd = (int)(p.jbwd.size() - bk.jbwd_off);
    bk.n_jlpk = (int)(p.jlpk.size() - bk.jlpk_off);
    bk.n_jrpk = (int)(p.jrpk.size() - bk.jrpk_off);
    bk.n_probe = (int)(p.probe_tasks.size() - bk.probe_off);
    p.probe_count.push_back(bk.n_probe);
    p.buckets.push_back(bk);
    p.bucket_ids.push_back(bi);
}

}  // namespace

int plan_2d_strands(const Region2D& reg, const std::vector<NraDevRead>& host_reads, bool reads_have_n, const Reads2D& rd,
                    int32_t flags, const Cells2D& cl, const KeepInputs& ki, PhaseClock& clk, Carried2D& cd, Pending2D& pd,
                    Plan2D& p)
{
    const int32_t n_reads = (int32_t)host_reads.size();
    pd.clear();
    p.reads = host_reads;                                      // + the shadows of chained reads, below
    {
        const int rc = count_cells(cl, n_reads, p);
        if (rc) return rc;
    }
    const int32_t left_len = (int32_t)reg.left.size(), unit1_len = (int32_t)reg.unit1.size(), mid_len = (int32_t)reg.mid.size(),
                  unit2_len = (int32_t)reg.unit2.size(), right_len = (int32_t)reg.right.size();
    const int64_t win = (int64_t)unit1_len * p.k1max + mid_len + (int64_t)unit2_len * p.k2max + 20;
    if (6 * win >= 32768) return fail(NRA_E_RANGE, "repeat window too long for the 16-bit window score");
    p.tlmax = (int64_t)left_len + win - 20 + right_len;
    if (p.tlmax > NRA_MAX_TLEN) return fail(NRA_E_RANGE, "template too long");

    Ctx c{rd, cl, cd, &pd, p, flags, NRA_JOINT_PACKED_COLS(left_len), NRA_JOINT_PACKED_COLS(right_len)};
    // junction decomposition needs a base left of the window and two bases of R
    p.brute = (flags & NRA_F_BRUTE_FORCE) != 0 || left_len < 1 || right_len < 2;
    p.all_strands_given = cl.read_strand != nullptr && n_reads > 0;
    if (cl.read_strand)
        for (int32_t r = 0; r < n_reads; ++r) if (p.cnt[r] > 0 && cl.read_strand[r] == 0) p.all_strands_given = false;
    decide_keep(c, reg, ki);

    clk.mark("2D cells: first/count");
    build_pool(reg, reads_have_n, p);

    // (the rows-per-lane bucket of a read was fixed when the reads were packed)
    // (measured and dropped: a bucket as 2 - 4 sub-buckets with kernel chains of their own -- the short kernels at the
    // end of one chain beside the long ones of the next -- is slower, 7.1 -> 7.7 / 8.7 / 10.5 ms of device time on config 3)
    p.by_bucket.assign((size_t)kChainBucket + 1, {});
    bool empty_reads_listed = false;
    for (int32_t r = 0; r < n_reads; ++r) {
        if (p.cnt[r] > 0 && p.reads[r].qlen == 0) empty_reads_listed = true;
        if (p.cnt[r] == 0 || p.reads[r].qlen == 0) continue;
        p.by_bucket[rd.chained_reads[r] ? kChainBucket : rd.jbucket[r]].push_back(r);
    }
    const std::vector<int32_t>& chain_reads = p.by_bucket[kChainBucket];
    p.pair_l.assign(rd.jpairs.size(), 0); p.pair_r.assign(rd.jpairs.size(), 0);
    // a routed grid: every read's cells are a full product (k1 values) x (one k2 progression) -> junction at the end
    // of mid.  The state kept from earlier cell lists differs between the two forms: switching drops it.
    p.joint_v2 = cl.grid != nullptr && !p.brute && (flags & NRA_F_JOINT_TAILS) == 0;
    p.joint_chain = p.joint_v2 && (flags & NRA_F_JOINT_NO_CHAIN) == 0;
    // k_joint_combine writes every cell of its reads, found or not: the cell arrays need no clearing unless some
    // cells belong to no combine task (empty reads, reads scored cell by cell)
    p.cells_need_clear = !p.joint_v2 || empty_reads_listed || !chain_reads.empty();
    if (p.joint_v2 != cd.joint_v2_prev) {
        std::fill(cd.rev_strand.begin(), cd.rev_strand.end(), (int8_t)0);
        cd.joint_v2_prev = p.joint_v2;
    }
    p.rs_off.assign((size_t)n_reads, 0);
    p.ra_off.assign((size_t)n_reads, 0);
    // wave states of one group of reads (NRA_F_TEST_CHAIN: one read per group, to exercise the reuse)
    // The buckets run concurrently, each in its own part of the state buffer.
    size_t n_nonempty = 0;
    for (const auto& v : p.by_bucket) n_nonempty += v.empty() ? 0 : 1;
    p.state_cap = (flags & NRA_F_TEST_CHAIN) ? 1 : (uint64_t)NRA_JOINT_STATE_CAP_INTS / std::max<size_t>(n_nonempty, 1);
    if (!p.brute) {
        p.jbwd.reserve((size_t)n_reads); p.jpre.reserve((size_t)n_reads); p.jcomb.reserve(p.joint_v2 ? (size_t)n_reads : 0);
        p.jtail.reserve((size_t)n_reads * 2);
    }
    for (int bi = kChainBucket; bi >= 0; --bi)
        if (!p.by_bucket[bi].empty()) strand_bucket(c, bi);
    if (!chain_reads.empty()) {
        size_t chain_cells = 0;
        for (int32_t r : chain_reads) chain_cells += p.cnt[r];
        p.chain_cap = (int)((p.tlmax + 127) / 64 * 64 + 64);
        p.payload_strips = chain_strips(std::max(chain_cells, p.probe_tasks.size()), NRA_CHAIN_STRIPS,
                                        (size_t)6 * 8 * (size_t)p.chain_cap);
    }
    return NRA_OK;
}

namespace {

// A read's MID scans as several tasks of at most kMidscanChunk k1 values: a wave's scans are one dependent chain (load a
// column state, 1 + |mid| columns of two lane scans each, store), so more, shorter waves hide it better than one wave per
// read (config 3, round 3: 5 k1 values per read).  The pieces differ in where their lists, outputs and slots begin only.
void push_midscan(std::vector<NraJointTask>& jtail, const NraJointTask& whole, uint64_t ints_per_k1)
{
    for (int32_t c = 0; c < whole.nk1; c += kMidscanChunk) {
        NraJointTask t = whole;
        t.k1_off = whole.k1_off + c; t.nk1 = std::min<int32_t>(kMidscanChunk, whole.nk1 - c);
        t.out = whole.out + c; t.pstate = whole.pstate + (uint64_t)c * ints_per_k1;
        jtail.push_back(t);
    }
}

// the read's combine task: n1 x n2 cells from the column states on either side of the junction
void push_combine(Ctx& c, const Bucket& bk, int32_t r, int32_t rs_first, int32_t rs_stride)
{
    Plan2D& p = c.p;
    const GridRow& gr = c.cl.grid->rows[(size_t)r];
    const uint64_t q3 = (uint64_t)3 * (uint64_t)p.reads[r].qlen;
    NraJointCombineTask ct{};
    ct.read = r; ct.n1 = gr.n1; ct.n2 = gr.n2; ct.out = (int32_t)p.first[r];
    ct.fb = (int32_t)p.fb_total; ct.ra = p.ra_off[(size_t)r]; ct.fs = p.fs_total; ct.rs = p.rs_off[(size_t)r];
    ct.rs_first = rs_first; ct.rs_stride = rs_stride; ct.rs_plane = 64 * bk.R;
    p.jcomb.push_back(ct);
    p.fs_total += (uint64_t)gr.n1 * q3; p.fb_total += gr.n1;
}

// algorithmic cells of a product grid: the sum of the template lengths in closed form
int64_t product_alg_cells(const Ctx& c, int32_t r)
{
    const NraDevRegion& d = c.d();
    const GridRow& gr = c.cl.grid->rows[(size_t)r];
    const int64_t n1 = gr.n1, n2 = gr.n2;
    const int64_t sum_k1 = n1 * gr.k1lo + (int64_t)c.cl.grid->step1 * n1 * (n1 - 1) / 2;
    const int64_t sum_k2 = n2 * gr.k2lo + (int64_t)c.cl.grid->step2 * n2 * (n2 - 1) / 2;
    return (int64_t)c.p.reads[r].qlen * (n1 * n2 * ((int64_t)d.l1 + d.l2 + d.l3) + d.m1 * sum_k1 * n2 + d.m2 * sum_k2 * n1);
}

// the open group of a bucket and how much of the state buffer it uses
struct Open {
    JointGroup g;
    uint64_t used = 0, state_max = 0;
};

// kept column states: the prefix sweep (keep == 1; none at all, keep == 2) leaves one at EVERY count
// of the read's kept range, the MID scans take the grid's own from among them
void kept_read(Ctx& c, Bucket& bk, Open& o, int32_t r, const std::vector<int32_t>& ks)
{
    Plan2D& p = c.p;
    const NraDevRegion& d = c.d();
    const JointGrid* grid = c.cl.grid;
    const int keep = p.keep;
    const uint64_t slot = (uint64_t)NRA_JOINT_NSTATE(bk.R) * 64;
    const NraJointPairTask& pair = c.rd.jpairs[(size_t)c.rd.jpair_of[r]];
    const GridRow& gr = grid->rows[(size_t)r];
    const NraGridRow kr = keep == 1 ? grid->keep[(size_t)r] : c.cd.keep_rows[(size_t)r];
    const uint64_t q3 = (uint64_t)3 * (uint64_t)p.reads[r].qlen;
    NraJointTask t{}; t.read = r; t.k1_off = (int32_t)p.k1list.size(); t.nk1 = gr.n1;
    t.k1 = kr.k1lo; t.k2step = 1;
    t.out = (int32_t)p.fb_total; t.pstate = p.fs_total;
    p.k1list.insert(p.k1list.end(), ks.begin(), ks.end());
    bk.cells_sweep += (int64_t)64 * bk.R * gr.n1 * (1 + d.l2);
    if (keep == 1) {
        NraJointTask tp{}; tp.read = r; tp.k1_off = (int32_t)p.k1list.size(); tp.nk1 = kr.n1;
        tp.state = o.used; tp.k2step = 1;
        if (c.rd.jpack_l) resume_packed(tp, pair, r);
        p.jpre.push_back(tp);
        for (int32_t i = 0; i < kr.n1; ++i) p.k1list.push_back(kr.k1lo + i);
        bk.cells_sweep += (int64_t)64 * bk.R * (d.l1 + d.m1 * (kr.k1lo + kr.n1 - 1) - 1 - (c.rd.jpack_l ? c.colsL : 0));
        bk.cells_sweep += (int64_t)64 * bk.R * (1 + std::min(63, std::max(p.reads[r].qlen - 1, 0) / bk.R));   // its drain
        t.state = o.used;                         // (bucket-relative like tp.state: both move to the bucket's base below)
        o.used += slot * (uint64_t)kr.n1;
        o.state_max = std::max(o.state_max, o.used);
    } else
        t.state = c.cd.keep_state_off[(size_t)r] | (1ull << 63);      // absolute already (marked; unmarked below)
    push_midscan(p.jtail, t, q3);
    push_combine(c, bk, r, gr.k2lo - kr.k2lo, grid->step2);
    // algorithmic cells (closed form, as below)
    p.alg_cells += product_alg_cells(c, r);
}

// one prefix sweep over L + u1^k1max per read that leaves the wave state at each of the read's k1
// values; one tail sweep per run of cells with the same k1 and k2 in arithmetic progression (how
// the grid rounds list them)
void swept_read(Ctx& c, Bucket& bk, Open& o, int32_t r, const std::vector<int32_t>& ks)
{
    Plan2D& p = c.p;
    const NraDevRegion& d = c.d();
    const JointGrid* grid = c.cl.grid;
    const int32_t *cell_k1 = c.cl.cell_k1, *cell_k2 = c.cl.cell_k2;
    const std::vector<uint32_t>&first = p.first, &cnt = p.cnt;
    const uint64_t slot = (uint64_t)NRA_JOINT_NSTATE(bk.R) * 64;
    const NraJointPairTask& pair = c.rd.jpairs[(size_t)c.rd.jpair_of[r]];
    JointGroup& g = o.g;
    if (o.used > 0 && o.used + slot * ks.size() > p.state_cap) {      // close the group (never with kept states: budgeted above)
        g.n_pre = (int)(p.jpre.size() - g.pre_off); g.n_tail = (int)(p.jtail.size() - g.tail_off);
        p.jgroups.push_back(g);
        g.pre_off = p.jpre.size(); g.tail_off = p.jtail.size();
        o.used = 0;
    }
    const uint64_t used = o.used;
    NraJointTask tp{}; tp.read = r; tp.k1_off = (int32_t)p.k1list.size(); tp.nk1 = (int32_t)ks.size();
    tp.state = used; tp.k2step = 1;
    if (c.rd.jpack_l) resume_packed(tp, pair, r);
    p.jpre.push_back(tp);
    bk.cells_sweep += (int64_t)64 * bk.R * (d.l1 + d.m1 * ks.back() - 1 - (c.rd.jpack_l ? c.colsL : 0));
    if (p.joint_v2) {
        // one MID sweep per k1 (the last prefix column + mid; leaves its column state and B(k1)), and the
        // read's combine task: n1 x n2 cells from the column states on either side of the junction
        const GridRow& gr = grid->rows[(size_t)r];
        const uint64_t q3 = (uint64_t)3 * (uint64_t)p.reads[r].qlen;
        if (p.joint_chain) {
            // the MID part of all the read's k1 in one wave, column by column (k_joint_midscan)
            NraJointTask t{}; t.read = r; t.k1_off = tp.k1_off; t.nk1 = tp.nk1;
            t.k1 = gr.k1lo; t.k2step = grid->step1;          // slot i of `state` holds k1lo + i * step1
            t.out = (int32_t)p.fb_total; t.state = used; t.pstate = p.fs_total;
            push_midscan(p.jtail, t, q3);
            bk.cells_sweep += (int64_t)64 * bk.R * gr.n1 * (1 + d.l2);
            bk.cells_sweep += (int64_t)64 * bk.R * (1 + std::min(63, std::max(p.reads[r].qlen - 1, 0) / bk.R));   // the prefix sweep's own drain
        } else
        for (int32_t i = 0; i < gr.n1; ++i) {
            NraJointTask t{}; t.read = r; t.k1 = ks[(size_t)i]; t.k2step = 1;
            t.out = (int32_t)(p.fb_total + i);
            t.state = used + slot * (uint64_t)i;
            t.pstate = p.fs_total + (uint64_t)i * q3;
            p.jtail.push_back(t);
            bk.cells_sweep += joint_cells(bk.R, 1 + d.l2, p.reads[r].qlen);
        }
        push_combine(c, bk, r, 0, 1);
    } else if (grid) {
        // one tail sweep per k1: the read's k2 values are one arithmetic progression
        const GridRow& gr = grid->rows[(size_t)r];
        for (int32_t i = 0; i < gr.n1; ++i) {
            NraJointTask t{}; t.read = r; t.k1 = ks[(size_t)i]; t.k2lo = gr.k2lo; t.k2step = grid->step2; t.n2 = gr.n2;
            t.out = (int32_t)(first[r] + (uint32_t)i * (uint32_t)gr.n2);
            t.state = used + slot * (uint64_t)i;
            p.jtail.push_back(t);
            bk.cells_sweep += joint_cells(bk.R, 1 + d.l2 + d.m2 * (t.k2lo + t.k2step * (t.n2 - 1)), p.reads[r].qlen);
        }
    } else
    for (uint32_t cc = first[r]; cc < first[r] + cnt[r];) {
        NraJointTask t{}; t.read = r; t.k1 = cell_k1[cc]; t.k2lo = cell_k2[cc]; t.k2step = 1; t.n2 = 1;
        t.out = (int32_t)cc;
        uint32_t e = cc + 1;
        if (e < first[r] + cnt[r] && cell_k1[e] == t.k1 && cell_k2[e] > t.k2lo) {
            t.k2step = cell_k2[e] - t.k2lo;
            while (e < first[r] + cnt[r] && cell_k1[e] == t.k1 &&
                   cell_k2[e] == t.k2lo + t.k2step * (int32_t)(e - cc)) ++e;
        }
        t.n2 = (int32_t)(e - cc);
        t.state = used + slot * (uint64_t)(std::lower_bound(ks.begin(), ks.end(), t.k1) - ks.begin());
        p.jtail.push_back(t);
        bk.cells_sweep += joint_cells(bk.R, 1 + d.l2 + d.m2 * (t.k2lo + t.k2step * (t.n2 - 1)), p.reads[r].qlen);
        cc = e;
    }
    p.k1list.insert(p.k1list.end(), ks.begin(), ks.end());
    o.used += slot * ks.size();
    o.state_max = std::max(o.state_max, o.used);
}

// algorithmic cells: the rectangle of every (read, cell) alignment; per-cell buckets: the payload queue
void listed_cells(Ctx& c, Bucket& bk, int32_t r, bool per_cell)
{
    Plan2D& p = c.p;
    const NraDevRegion& d = c.d();
    int64_t tl_sum = 0;
    for (uint32_t i = 0; i < p.cnt[r]; ++i) {
        const int32_t k1 = c.k1_of(r, i), k2 = c.k2_of(r, i);
        const int tl = d.l1 + d.m1 * k1 + d.l2 + d.m2 * k2 + d.l3;
        tl_sum += tl;
        if (per_cell) {
            p.queue_tasks.push_back(NraTask{r, k1, k2, (int32_t)(p.first[r] + i)});
            bk.cells_queue += sweep_cells(bk.R, tl);
        }
    }
    p.alg_cells += (int64_t)p.reads[r].qlen * tl_sum;
}

// ---- part 2: the sweeps that depend on the cell list
void cells_bucket(Ctx& c, size_t bidx, std::vector<int32_t>& ks)
{
    Plan2D& p = c.p;
    const JointGrid* grid = c.cl.grid;
    const int bi = p.bucket_ids[bidx];
    Bucket& bk = p.buckets[bidx];
    bk.queue_off = p.queue_tasks.size();
    bk.comb_off = p.jcomb.size();
    const bool per_cell = p.brute || bk.chain;
    Open o;
    o.g.R = bk.R; o.g.bucket = (int)bidx; o.g.pre_off = p.jpre.size(); o.g.tail_off = p.jtail.size();
    const size_t bucket_pre0 = p.jpre.size(), bucket_tail0 = p.jtail.size();
    for (int32_t r : p.by_bucket[bi]) {
        if (!per_cell) {
            ks.clear();                                      // the read's distinct k1 values, ascending
            if (grid) {
                const GridRow& gr = grid->rows[(size_t)r];
                for (int32_t i = 0; i < gr.n1; ++i) ks.push_back(gr.k1lo + i * grid->step1);
                if (p.keep != 0) {
                    kept_read(c, bk, o, r, ks);
                    continue;
                }
            } else {
                ks.assign(c.cl.cell_k1 + p.first[r], c.cl.cell_k1 + p.first[r] + p.cnt[r]);
                if (!std::is_sorted(ks.begin(), ks.end())) std::sort(ks.begin(), ks.end());
                ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
            }
            swept_read(c, bk, o, r, ks);
        }
        if (grid && !per_cell) p.alg_cells += product_alg_cells(c, r);
        else listed_cells(c, bk, r, per_cell);
    }
    if (!per_cell) {
        JointGroup& g = o.g;
        g.n_pre = (int)(p.jpre.size() - g.pre_off); g.n_tail = (int)(p.jtail.size() - g.tail_off);
        if (g.n_pre > 0 || g.n_tail > 0) p.jgroups.push_back(g);
        for (size_t i = bucket_pre0; i < p.jpre.size(); ++i) {
            p.jpre[i].state += p.state_base;
            if (p.keep == 1) c.cd.keep_state_off[(size_t)p.jpre[i].read] = p.jpre[i].state;
        }
        for (size_t i = bucket_tail0; i < p.jtail.size(); ++i) {
            if (p.jtail[i].state >> 63) p.jtail[i].state &= ~(1ull << 63);      // a kept state: absolute
            else p.jtail[i].state += p.state_base;
        }
        p.state_base += o.state_max;
    }
    bk.n_queue = (int)(p.queue_tasks.size() - bk.queue_off);
    bk.queue_cap = (size_t)bk.n_queue;
    bk.n_comb = (int)(p.jcomb.size() - bk.comb_off);
    p.queue_count.push_back(bk.n_queue);
}

}  // namespace

void plan_2d_cells(const std::vector<NraDevRead>& host_reads, const Reads2D& rd, const Cells2D& cl, size_t n_q2bit_words,
                   int64_t warm_cells, Carried2D& cd, Plan2D& p)
{
    const int32_t n_reads = (int32_t)host_reads.size();
    const NraDevRegion& d = p.dregs[0];
    Ctx c{rd, cl, cd, nullptr, p, 0, NRA_JOINT_PACKED_COLS(d.l1), NRA_JOINT_PACKED_COLS(d.l3)};
    std::vector<int32_t> ks;
    for (size_t bidx = 0; bidx < p.buckets.size(); ++bidx) cells_bucket(c, bidx, ks);

    p.stats.n_alignments = cl.n_cells;
    p.stats.algorithmic_cells = p.alg_cells;
    int64_t ex = 0;
    for (const Bucket& bk : p.buckets) ex += bk.cells_pair + bk.cells_queue + bk.cells_sweep;
    ex += warm_cells;
    p.stats.executed_cells = ex;
    p.stats.algorithmic_bytes = (int64_t)n_q2bit_words * 4 + (int64_t)p.pool.size() + cl.n_cells * 8 + (int64_t)n_reads * 25;
    int64_t packed_ints = 0;
    for (const Bucket& bk : p.buckets) packed_ints += (int64_t)(bk.n_jlpk + bk.n_jrpk) * NRA_JOINT_NPSTATE(bk.R) * 64;
    p.stats.intermediate_bytes = p.brute ? 0 : 2 * ((int64_t)p.state_base * 4 + packed_ints * 4 +
                                                    (p.joint_v2 ? (int64_t)(p.rs_total + p.fs_total) * 4 : (int64_t)n_q2bit_words * 16 * 3 * 4));
}

// ---- the flank sweeps ahead of a cell list ------------------------------------------------------
void plan_2d_flanks(const Reads2D& rd, const Carried2D& cd, const int8_t* read_strand, int32_t left_len, int32_t right_len,
                    FlankPlan& out)
{
    std::vector<FlankPart>& parts = out.parts;
    std::vector<NraJointPairTask>& mt = out.tasks;
    for (size_t i = 0; i < rd.jpairs.size();) {
        const int bi = rd.jbucket[(size_t)rd.jpairs[i].read_a];
        FlankPart part{kRList[bi], mt.size(), 0, 0};
        for (; i < rd.jpairs.size() && rd.jbucket[(size_t)rd.jpairs[i].read_a] == bi; ++i) {
            const NraJointPairTask& pair = rd.jpairs[i];
            bool all = true, stale_l = false, stale_r = false;
            for (int32_t q : {pair.read_a, pair.read_b}) {
                if (q < 0) continue;
                if (read_strand[q] == 0) all = false;
                if (cd.lst_strand[(size_t)q] != read_strand[q]) stale_l = true;
                if (cd.rpk_strand[(size_t)q] != read_strand[q]) stale_r = true;
            }
            if (!all) continue;
            for (int32_t q : {pair.read_a, pair.read_b}) {
                if (q < 0) continue;
                if (rd.jpack_l && stale_l) out.l_done.push_back({q, read_strand[q]});
                if (rd.jpack_r && stale_r) out.r_done.push_back({q, read_strand[q]});
            }
            if (rd.jpack_l && stale_l) { NraJointPairTask t = pair; t.state |= 1ull << 63; mt.push_back(t); part.n_l++; }
            if (rd.jpack_r && stale_r) { mt.push_back(pair); part.n_r++; }
        }
        if (part.n_l || part.n_r) parts.push_back(part);
    }
    std::reverse(parts.begin(), parts.end());                  // the longest reads first, like the cell lists' buckets
    const int colsL = NRA_JOINT_PACKED_COLS(left_len), colsR = NRA_JOINT_PACKED_COLS(right_len);
    for (const FlankPart& pt : parts)
        out.cells += (int64_t)pt.n_l * 2 * 64 * pt.R * colsL + (int64_t)pt.n_r * 2 * 64 * pt.R * colsR;
}

void commit_2d_flanks(Carried2D& cd, const FlankPlan& fp)
{
    for (const auto& pr2 : fp.l_done) cd.lst_strand[(size_t)pr2.first] = pr2.second;
    for (const auto& pr2 : fp.r_done) cd.rpk_strand[(size_t)pr2.first] = pr2.second;
}

// ---- the refinement behind a routed grid --------------------------------------------------------
int check_2d_refine(bool run_open, const Forms2D& f, const Carried2D& cd, const std::vector<Bucket>& buckets, int32_t n_reads,
                    int32_t buf1, int32_t buf2, const double* lo1, const double* hi1, const double* lo2, const double* hi2)
{
    if (!run_open || !f.joint_v2 || !f.joint_chain || f.keep == 0 || !cd.keep_valid ||
        f.brute || !f.all_strands_given || cd.keep_rows.size() != (size_t)n_reads)
        return fail(NRA_E_STATE, "no refinement: it follows nra_batch_run of a routed grid (nra_batch2d_set_grid, every strand "
                                 "given) whose column states are kept, before anything waits for that run");
    for (const Bucket& bk : buckets)
        if (bk.chain) return fail(NRA_E_STATE, "no refinement: reads beyond one register block are scored cell by cell");
    // Every count a read's refinement can ask for -- within buf of a size between its first and last grid value, inside
    // [lo, hi) -- has to be among the counts column states were kept at.  True by construction behind the grid that kept
    // them when buf = its steps and [lo, hi) = its bounds; not necessarily behind a grid that itself ran from states an
    // EARLIER grid kept, or with other buffers / bounds: then the caller takes the two-call path.
    if (cd.cur_rows.size() != (size_t)n_reads) return fail(NRA_E_STATE, "no refinement: the current cell list is not a routed grid");
    for (int32_t r = 0; r < n_reads; ++r) {
        const NraGridRow& g = cd.cur_rows[(size_t)r];
        const NraGridRow& k = cd.keep_rows[(size_t)r];
        if (g.n1 <= 0 || g.n2 <= 0 || k.n1 <= 0 || k.n2 <= 0) continue;
        auto fits = [](int32_t first, int32_t n, int32_t step, int32_t buf, double lo, double hi, int32_t klo, int32_t kn) {
            if (!(lo < hi)) return true;
            const int64_t last = (int64_t)first + (int64_t)(n - 1) * step;
            const double cl = std::ceil(lo), ch = std::ceil(hi);
            const int64_t need_lo = std::max<int64_t>({cl < 0 ? 0 : (cl > 1e9 ? (int64_t)1e9 : (int64_t)cl), (int64_t)first - buf, 0});
            const int64_t need_hi = std::min<int64_t>(ch > 1e9 ? (int64_t)1e9 : (int64_t)ch - 1, last + buf - 1);
            return need_hi < need_lo || (need_lo >= klo && need_hi <= (int64_t)klo + kn - 1);
        };
        if (!fits(g.k1lo, g.n1, cd.cur_step1, buf1, lo1[r], hi1[r], k.k1lo, k.n1) ||
            !fits(g.k2lo, g.n2, cd.cur_step2, buf2, lo2[r], hi2[r], k.k2lo, k.n2))
            return fail(NRA_E_STATE, "no refinement: a read's refinement could ask for repeat counts no column state was kept at");
    }
    return NRA_OK;
}

// static tasks: what a read's refinement needs whatever its round-2 size turns out to be
int plan_2d_refine(const std::vector<NraDevRead>& host_reads, const Reads2D& rd, const Carried2D& cd,
                   const std::vector<Bucket>& buckets, int32_t buf1, int32_t buf2, RefinePlan& out)
{
    const int32_t n_reads = (int32_t)host_reads.size();
    const size_t nb = buckets.size();
    const int cap1 = 2 * buf1, cap2 = 2 * buf2;
    const int64_t cap = (int64_t)cap1 * cap2;
    std::vector<std::vector<NraJointTask>> mid(nb);
    std::vector<std::vector<NraJointCombineTask>> comb(nb);
    std::vector<int> bucket_of_R((size_t)NRA_MAX_R + 1, -1);
    for (size_t i = 0; i < nb; ++i) bucket_of_R[(size_t)buckets[i].R] = (int)i;
    std::vector<uint32_t>& first = out.first;
    std::vector<int32_t>& rowspad = out.rowspad;
    first.assign((size_t)n_reads, 0);
    rowspad.assign((size_t)n_reads, 0);
    uint64_t fs_total = 0; int64_t fb_total = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        first[(size_t)r] = (uint32_t)((int64_t)r * cap);
        const NraGridRow& k = cd.keep_rows[(size_t)r];
        if (k.n1 <= 0 || k.n2 <= 0 || host_reads[(size_t)r].qlen <= 0 || rd.chained_reads[(size_t)r]) continue;
        const int R = kRList[rd.jbucket[(size_t)r]];
        const int bi = bucket_of_R[(size_t)R];
        if (bi < 0) return fail(NRA_E_STATE, "no refinement: a read's bucket did not run");
        rowspad[(size_t)r] = 64 * R;
        const uint64_t q3 = (uint64_t)3 * (uint64_t)host_reads[(size_t)r].qlen;
        for (int c = 0; c < cap1; c += kMidscanChunk) {
            NraJointTask t{}; t.read = r; t.k1_off = c; t.nk1 = std::min(kMidscanChunk, cap1 - c);
            t.k1 = k.k1lo; t.k2step = 1; t.state = cd.keep_state_off[(size_t)r];
            t.pstate = fs_total + (uint64_t)c * q3; t.out = (int32_t)(fb_total + c);
            mid[(size_t)bi].push_back(t);
        }
        NraJointCombineTask ct{};
        ct.read = r; ct.out = (int32_t)first[(size_t)r]; ct.fb = (int32_t)fb_total; ct.ra = cd.keep_ra_off[(size_t)r];
        ct.fs = fs_total; ct.rs = cd.keep_rs_off[(size_t)r]; ct.rs_first = k.k2lo; ct.rs_stride = 1; ct.rs_plane = 64 * R;
        comb[(size_t)bi].push_back(ct);
        fs_total += (uint64_t)cap1 * q3; fb_total += cap1;
    }
    out.mid_off.assign(nb + 1, 0); out.comb_off.assign(nb + 1, 0);
    for (size_t i = 0; i < nb; ++i) {
        out.mid_off[i] = out.mid.size(); out.comb_off[i] = out.comb.size();
        out.mid.insert(out.mid.end(), mid[i].begin(), mid[i].end());
        out.comb.insert(out.comb.end(), comb[i].begin(), comb[i].end());
    }
    out.mid_off[nb] = out.mid.size(); out.comb_off[nb] = out.comb.size();
    out.fs_total = fs_total; out.fb_total = fb_total;
    return NRA_OK;
}

// ---- digest -------------------------------------------------------------------------------------
namespace {

void feed_joint_task(Fnv& f, const NraJointTask& x)
{
    f.put(x.read); f.put(x.k1); f.put(x.k2lo); f.put(x.k2step); f.put(x.n2); f.put(x.out); f.put(x.k1_off); f.put(x.nk1);
    f.put(x.state); f.put(x.pstate); f.put(x.phalf); f.put(x.resume);
}
void feed_combine_task(Fnv& f, const NraJointCombineTask& x)
{
    f.put(x.read); f.put(x.n1); f.put(x.n2); f.put(x.out); f.put(x.fb); f.put(x.ra); f.put(x.rs_first); f.put(x.rs_stride);
    f.put(x.fs); f.put(x.rs); f.put(x.rs_plane);
}
void feed_pair(Fnv& f, const NraJointPairTask& x) { f.put(x.read_a); f.put(x.read_b); f.put(x.state); }
void feed_task(Fnv& f, const NraTask& x) { f.put(x.read); f.put(x.k1); f.put(x.k2); f.put(x.out); }
void feed_row(Fnv& f, const NraGridRow& x) { f.put(x.k1lo); f.put(x.n1); f.put(x.k2lo); f.put(x.n2); }
void feed_done(Fnv& f, const std::pair<int32_t, int8_t>& x) { f.put(x.first); f.put(x.second); }

struct KeyValues {
    std::string v;
    void add(const char* k, int64_t x) { if (!v.empty()) v += ' '; v += k; v += '='; v += std::to_string(x); }
};

}  // namespace

void digest_2d_reads(Digest& d, const Reads2D& rd)
{
    d.num("jpack_l", rd.jpack_l);
    d.num("jpack_r", rd.jpack_r);
    d.num("jpack_ints", (int64_t)rd.jpack_ints);
    d.array("chained_reads", rd.chained_reads);
    d.array("jbucket", rd.jbucket);
    d.array("jpair_of", rd.jpair_of);
    d.array("jpairs", rd.jpairs, feed_pair);
}

void digest_2d_carried(Digest& d, const Carried2D& cd)
{
    d.num("keep_valid", cd.keep_valid);
    d.num("joint_v2_prev", cd.joint_v2_prev);
    d.num("cur_step1", cd.cur_rows.empty() ? 0 : cd.cur_step1);
    d.num("cur_step2", cd.cur_rows.empty() ? 0 : cd.cur_step2);
    d.array("rev_strand", cd.rev_strand);
    d.array("lst_strand", cd.lst_strand);
    d.array("rpk_strand", cd.rpk_strand);
    d.array("keep_rows", cd.keep_rows, feed_row);
    d.array("keep_strand", cd.keep_strand);
    d.array("keep_state_off", cd.keep_state_off);
    d.array("keep_rs_off", cd.keep_rs_off);
    d.array("keep_ra_off", cd.keep_ra_off);
    d.array("cur_rows", cd.cur_rows, feed_row);
}

void digest_2d_cells(Digest& d, const Plan2D& p, const Pending2D& pd, size_t expect)
{
    d.num("keep", p.keep);
    d.num("keep_bytes", (int64_t)p.keep_bytes);
    d.num("device_asked", p.device_asked);
    d.num("brute", p.brute);
    d.num("joint_v2", p.joint_v2);
    d.num("joint_chain", p.joint_chain);
    d.num("cells_need_clear", p.cells_need_clear);
    d.num("all_strands_given", p.all_strands_given);
    d.num("has_n", p.has_n);
    d.num("k1max", p.k1max_pool);
    d.num("k2max", p.k2max_pool);
    d.num("rs_total", (int64_t)p.rs_total);
    d.num("ra_total", p.ra_total);
    d.num("fs_total", (int64_t)p.fs_total);
    d.num("fb_total", p.fb_total);
    d.num("state_total", (int64_t)p.state_base);
    d.num("state_cap", (int64_t)p.state_cap);
    d.num("chain_cap", p.chain_cap);
    d.num("payload_strips", p.payload_strips);
    d.num("expect", (int64_t)expect);
    d.num("n_alignments", p.stats.n_alignments);
    d.num("algorithmic_cells", p.stats.algorithmic_cells);
    d.num("executed_cells", p.stats.executed_cells);
    d.num("algorithmic_bytes", p.stats.algorithmic_bytes);
    d.num("intermediate_bytes", p.stats.intermediate_bytes);
    d.num("n_buckets", (int64_t)p.buckets.size());
    for (size_t i = 0; i < p.buckets.size(); ++i) {
        const Bucket& b = p.buckets[i];
        KeyValues kv;
        kv.add("id", p.bucket_ids[i]); kv.add("R", b.R); kv.add("chain", b.chain);
        kv.add("n_pair", b.n_pair); kv.add("pair_off", (int64_t)b.pair_off);
        kv.add("n_probe", b.n_probe); kv.add("probe_off", (int64_t)b.probe_off);
        kv.add("n_jbwd", b.n_jbwd); kv.add("jbwd_off", (int64_t)b.jbwd_off);
        kv.add("n_jlpk", b.n_jlpk); kv.add("jlpk_off", (int64_t)b.jlpk_off);
        kv.add("n_jrpk", b.n_jrpk); kv.add("jrpk_off", (int64_t)b.jrpk_off);
        kv.add("n_queue", b.n_queue); kv.add("queue_off", (int64_t)b.queue_off); kv.add("queue_cap", (int64_t)b.queue_cap);
        kv.add("n_comb", b.n_comb); kv.add("comb_off", (int64_t)b.comb_off);
        kv.add("cells_pair", b.cells_pair); kv.add("cells_queue", b.cells_queue); kv.add("cells_sweep", b.cells_sweep);
        d.line(("bucket" + std::to_string(i)).c_str(), kv.v);
    }
    d.num("n_groups", (int64_t)p.jgroups.size());
    for (size_t i = 0; i < p.jgroups.size(); ++i) {
        const JointGroup& g = p.jgroups[i];
        KeyValues kv;
        kv.add("R", g.R); kv.add("bucket", g.bucket); kv.add("n_pre", g.n_pre); kv.add("n_tail", g.n_tail);
        kv.add("pre_off", (int64_t)g.pre_off); kv.add("tail_off", (int64_t)g.tail_off);
        d.line(("group" + std::to_string(i)).c_str(), kv.v);
    }
    d.array("first", p.first);
    d.array("cnt", p.cnt);
    d.array("pool", p.pool);
    d.array("dregs", p.dregs, [](Fnv& f, const NraDevRegion& x) {
        f.put(x.p1_off); f.put(x.p2_off); f.put(x.p3_off); f.put(x.pr_off);
        f.put(x.l1); f.put(x.m1); f.put(x.l2); f.put(x.m2); f.put(x.l3);
    });
    d.array("reads", p.reads, [](Fnv& f, const NraDevRead& x) { f.put(x.qoff); f.put(x.qlen); f.put(x.region); f.put(x.rc); });
    d.array("pair_tasks", p.pair_tasks, [](Fnv& f, const NraPairTask& x) {
        f.put(x.read); f.put(x.k1a); f.put(x.k2a); f.put(x.k1b); f.put(x.k2b); f.put(x.out_a); f.put(x.out_b); f.put(x.flags);
    });
    d.array("probe_tasks", p.probe_tasks, feed_task);
    d.array("probe_count", p.probe_count);
    d.array("jbwd", p.jbwd, feed_joint_task);
    d.array("jlpk", p.jlpk, feed_pair);
    d.array("jrpk", p.jrpk, feed_pair);
    d.array("queue_tasks", p.queue_tasks, feed_task);
    d.array("queue_count", p.queue_count);
    d.array("jpre", p.jpre, feed_joint_task);
    d.array("jtail", p.jtail, feed_joint_task);
    d.array("k1list", p.k1list);
    d.array("jcomb", p.jcomb, feed_combine_task);
    d.num("keep_pending", pd.keep);
    d.array("rev_pending", pd.rev, feed_done);
    d.array("lst_pending", pd.lst, feed_done);
    d.array("rpk_pending", pd.rpk, feed_done);
}

void digest_2d_flanks(Digest& d, const FlankPlan& fp)
{
    d.num("warm_cells", fp.cells);
    d.num("n_parts", (int64_t)fp.parts.size());
    for (size_t i = 0; i < fp.parts.size(); ++i) {
        const FlankPart& pt = fp.parts[i];
        KeyValues kv;
        kv.add("R", pt.R); kv.add("off", (int64_t)pt.off); kv.add("n_l", (int64_t)pt.n_l); kv.add("n_r", (int64_t)pt.n_r);
        d.line(("part" + std::to_string(i)).c_str(), kv.v);
    }
    d.array("warm_tasks", fp.tasks, feed_pair);
    d.array("l_done", fp.l_done, feed_done);
    d.array("r_done", fp.r_done, feed_done);
}

void digest_2d_refine(Digest& d, const RefinePlan& rp, size_t expect, int64_t n_cands)
{
    d.num("fs_total", (int64_t)rp.fs_total);
    d.num("fb_total", rp.fb_total);
    d.num("expect", (int64_t)expect);
    d.num("rf_n_cands", n_cands);
    d.array("mid_off", rp.mid_off);
    d.array("comb_off", rp.comb_off);
    d.array("rf_first", rp.first);
    d.array("rf_rowspad", rp.rowspad);
    d.array("rf_mid", rp.mid, feed_joint_task);
    d.array("rf_comb", rp.comb, feed_combine_task);
}

namespace {

// a batch as nra_plan2d_digest plays it
struct Played {
    Region2D reg;
    const std::vector<NraDevRead>& host_reads;
    bool reads_have_n;
    size_t n_q2bit_words;
    int32_t flags;
    Reads2D rd;
    Carried2D cd;
    Pending2D pd;
    std::vector<Bucket> buckets;
    Forms2D forms{0, false, false, false, false};
    bool run_open = false, refined = false;    // the last step enqueued a run nothing has waited for / with a refinement
    bool warm_pending = false;
    int64_t warm_cells = 0;
    uint64_t held = 0;                         // what the last keeping step asked for
    int32_t n_reads() const { return (int32_t)host_reads.size(); }
};

int play_cells(Played& b, const nra_plan2d_step_t& s, const Cells2D& cl, Digest& d)
{
    if (!cells_2d_countable(cl.n_cells)) return fail(NRA_E_RANGE, "too many cells");
    b.buckets.clear();
    const int64_t warm_cells = b.warm_pending ? b.warm_cells : 0;
    KeepInputs ki;
    ki.budget = (uint64_t)s.keep_budget;
    ki.held = b.held;
    ki.device_free = [&](uint64_t& free_b) { free_b = (uint64_t)s.device_free; return true; };
    PhaseClock clk(false);
    Plan2D plan;
    const int rc = plan_2d_strands(b.reg, b.host_reads, b.reads_have_n, b.rd, b.flags, cl, ki, clk, b.cd, b.pd, plan);
    if (rc) return rc;
    if (plan.keep == 1) b.held = plan.keep_bytes;
    plan_2d_cells(b.host_reads, b.rd, cl, b.n_q2bit_words, warm_cells, b.cd, plan);
    b.cd.set_current(cl.grid, b.n_reads());
    digest_2d_cells(d, plan, b.pd, cell_arena_bytes(b.n_q2bit_words, cl.n_cells, plan.pool.size(), b.n_reads()));
    // ... as if the run had been enqueued and waited for
    b.forms = Forms2D{plan.keep, plan.brute, plan.joint_v2, plan.joint_chain, plan.all_strands_given};
    b.buckets = plan.buckets;
    b.warm_pending = false;
    commit_2d(b.cd, b.pd);
    b.run_open = true; b.refined = false;
    return NRA_OK;
}

int play_step(Played& b, const nra_plan2d_step_t& s, Digest& d)
{
    const int32_t n_reads = b.n_reads();
    if (s.kind != NRA_PLAN2D_REFINE) b.run_open = false;
    switch (s.kind) {
    case NRA_PLAN2D_CELLS: {
        if (s.n_cells < 0) return fail(NRA_E_ARG, "bad cell count");
        if (s.n_cells > 0 && (!s.cell_read || !s.cell_k1 || !s.cell_k2)) return fail(NRA_E_ARG, "NULL cell array");
        Cells2D cl;
        cl.read_strand = s.read_strand; cl.n_cells = s.n_cells;
        cl.cell_read = s.cell_read; cl.cell_k1 = s.cell_k1; cl.cell_k2 = s.cell_k2;
        return play_cells(b, s, cl, d);
    }
    case NRA_PLAN2D_GRID: {
        std::vector<GridRow> rows, keep;
        int64_t n = 0;
        const int rc = route_grid(n_reads, s.start1, s.step1, s.count1, s.lo1, s.hi1, s.start2, s.step2, s.count2, s.lo2, s.hi2,
                                  rows, n, &keep);
        if (rc) return rc;
        d.num("n_cells", n);
        const JointGrid grid{s.step1, s.step2, rows.data(), keep.data()};
        Cells2D cl;
        cl.read_strand = s.read_strand; cl.n_cells = n; cl.grid = &grid;
        return play_cells(b, s, cl, d);
    }
    case NRA_PLAN2D_SWEEP_FLANKS: {
        if (n_reads > 0 && !s.read_strand) return fail(NRA_E_ARG, "NULL strand array");
        const int32_t left_len = (int32_t)b.reg.left.size(), right_len = (int32_t)b.reg.right.size();
        FlankPlan fp;
        if (sweeps_flanks_ahead(b.rd, b.flags, left_len, right_len, n_reads))
            plan_2d_flanks(b.rd, b.cd, s.read_strand, left_len, right_len, fp);
        digest_2d_flanks(d, fp);
        if (fp.parts.empty()) return NRA_OK;
        b.warm_pending = true;
        b.warm_cells = fp.cells;
        commit_2d_flanks(b.cd, fp);
        return NRA_OK;
    }
    case NRA_PLAN2D_REFINE: {
        if (s.buf1 <= 0 || s.buf2 <= 0 || s.buf1 > 4096 || s.buf2 > 4096) return fail(NRA_E_ARG, "bad refinement buffers");
        if (n_reads > 0 && (!s.lo1 || !s.hi1 || !s.lo2 || !s.hi2)) return fail(NRA_E_ARG, "NULL bound array");
        int rc = check_2d_refine(b.run_open && !b.refined, b.forms, b.cd, b.buckets, n_reads, s.buf1, s.buf2, s.lo1, s.hi1, s.lo2,
                                 s.hi2);
        if (rc) return rc;
        const int64_t cap = (int64_t)(2 * s.buf1) * (2 * s.buf2);
        if (!cells_2d_countable(cap * n_reads)) return fail(NRA_E_RANGE, "too many cells");
        RefinePlan rp;
        rc = plan_2d_refine(b.host_reads, b.rd, b.cd, b.buckets, s.buf1, s.buf2, rp);
        if (rc) return rc;
        digest_2d_refine(d, rp, refine_arena_bytes(rp.fs_total, cap, n_reads), cap * n_reads);
        b.refined = true;
        return NRA_OK;
    }
    case NRA_PLAN2D_INVALIDATE:
        b.cd.invalidate();
        return NRA_OK;
    }
    return fail(NRA_E_ARG, "unknown step kind");
}

}  // namespace

std::string plan_2d_digest(const nra_joint_region_t* reg, const std::vector<NraDevRead>& host_reads, bool reads_have_n,
                           size_t n_q2bit_words, const nra_scoring_t* sc, int32_t flags, const nra_plan2d_step_t* steps,
                           int32_t n_steps)
{
    Played b{Region2D{std::string(reg->left ? reg->left : "", (size_t)reg->left_len), std::string(reg->unit1, (size_t)reg->unit1_len),
                      std::string(reg->mid ? reg->mid : "", (size_t)reg->mid_len), std::string(reg->unit2, (size_t)reg->unit2_len),
                      std::string(reg->right ? reg->right : "", (size_t)reg->right_len)},
             host_reads, reads_have_n, n_q2bit_words, flags};
    plan_2d_reads(host_reads, reg->left_len, reg->right_len, sc, flags, b.rd);
    b.cd.init(b.n_reads());
    Digest d;
    digest_2d_reads(d, b.rd);
    for (int32_t i = 0; i < n_steps; ++i) {
        d.line("step", std::to_string(i) + " kind " + std::to_string(steps[i].kind));
        const int rc = play_step(b, steps[i], d);
        if (rc) d.line("error", std::to_string(rc) + " " + nra_last_error());
        digest_2d_carried(d, b.cd);
    }
    return d.s;
}
