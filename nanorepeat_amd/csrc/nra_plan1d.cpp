// nra_plan1d.cpp -- the plan of a 1D batch (nra_plan1d.h), step by step in the order plan_1d runs them, and its digest.
// Host arithmetic only: no environment, no device.
#include "nra_plan1d.h"

#include <cmath>
#include <cstring>

namespace {

int fail(int code, const std::string& msg) { return nra_set_error(code, msg.c_str()); }

// the arguments of plan_1d, as the steps share them
struct PlanIn {
    const nra_region_t* regions;
    int32_t n_regions;
    const std::vector<NraDevRead>& reads;
    int32_t n_reads;
    const int32_t *kmin, *kmax;
    const nra_scoring_t* sc;
    int32_t flags;
    const Plan1DKnobs& knobs;
    int simds;
    bool all_ext() const { return (flags & NRA_F_ALL_EXTENTS) != 0; }
    bool test_chain() const { return (flags & NRA_F_TEST_CHAIN) != 0; }
    int64_t tlen(int32_t r) const       // the longest template of read r
    {
        const nra_region_t& rg = regions[reads[r].region];
        return (int64_t)rg.left_len + (int64_t)rg.unit_len * kmax[r] + rg.right_len;
    }
};

// reads by raw bucket index while they are routed and folded (route_reads); chain_cols: the widest chained template
struct Routing {
    std::vector<std::vector<int32_t>> by_bucket;
    int chain_cols = 0;
};

// ---- candidates and templates -----------------------------------------------------------------
int plan_candidates(const PlanIn& in, Plan1D& p)
{
    // per-region largest k, candidate offsets
    p.region_kmax.assign((size_t)in.n_regions, 0);
    p.coff.assign((size_t)in.n_reads + 1, 0);
    p.read_bucket.assign((size_t)in.n_reads, -1);
    int64_t total = 0;
    for (int32_t r = 0; r < in.n_reads; ++r) {
        p.coff[r] = (uint32_t)total;
        if (in.kmin[r] > in.kmax[r]) continue;
        if (in.kmin[r] < 0) return fail(NRA_E_ARG, "kmin < 0");
        const int g = in.reads[r].region;
        const int64_t tl = in.tlen(r);
        if (tl > NRA_MAX_TLEN_WIDE) return fail(NRA_E_RANGE, "template longer than " + std::to_string(NRA_MAX_TLEN_WIDE));
        p.region_kmax[g] = std::max(p.region_kmax[g], in.kmax[r]);
        total += (int64_t)in.kmax[r] - in.kmin[r] + 1;
        if (total > 0x7ff00000ll) return fail(NRA_E_RANGE, "more than 2^31 candidates in one batch");
    }
    p.coff[in.n_reads] = (uint32_t)total;
    p.n_cands = total;
    return NRA_OK;
}

int plan_templates(const PlanIn& in, Plan1D& p)
{
    // code pool + region table
    std::vector<uint8_t>& pool = p.pool;
    p.dregs.resize((size_t)in.n_regions);
    bool& has_n = p.has_n;                       // templates; the reads' share is known when the packing is over
    for (int32_t g = 0; g < in.n_regions; ++g) {
        const nra_region_t& rg = in.regions[g];
        NraDevRegion d{};
        d.p1_off = pool_append(pool, rg.left, rg.left_len, rg.unit, rg.unit_len, p.region_kmax[g], has_n);
        d.p2_off = (uint32_t)pool.size();
        d.p3_off = pool_append(pool, rg.right, rg.right_len, nullptr, 0, 0, has_n);
        {   // rev(R) + rev(unit)^kmax for the reverse sweep
            std::string rr(rg.right, rg.right + rg.right_len), ru(rg.unit, rg.unit + rg.unit_len);
            std::reverse(rr.begin(), rr.end());
            std::reverse(ru.begin(), ru.end());
            d.pr_off = pool_append(pool, rr.data(), rg.right_len, ru.data(), rg.unit_len, p.region_kmax[g], has_n);
        }
        d.l1 = rg.left_len; d.m1 = rg.unit_len; d.l2 = 0; d.m2 = 0; d.l3 = rg.right_len;
        p.dregs[g] = d;
        if (pool.size() > 0xfff00000ull) return fail(NRA_E_RANGE, "template pool exceeds 4 GB");
    }
    pool.push_back(0);
    return NRA_OK;
}

// brute force or the sweeps, and the margin of the taint scheme: what the regions, the scoring and the flags allow
void plan_schemes(const PlanIn& in, Plan1D& p)
{
    const nra_scoring_t* sc = in.sc;
    bool brute = in.all_ext() || (in.flags & NRA_F_BRUTE_FORCE) != 0;
    for (int32_t g = 0; g < in.n_regions; ++g)       // the junction needs a base on either side
        if (in.regions[g].left_len < 1 || in.regions[g].right_len < 1) brute = true;
    {   // the sweep kernels keep (substitution score + gap-open cost) in unsigned table bytes
        // (doubled: the low bit of every state is the origin bit)
        const int o1 = sc->gap_open1 + sc->gap_ext1;
        if (o1 < sc->mismatch || o1 < sc->sc_ambi || 2 * (sc->match + o1) > 127) brute = true;
        // and every state in [0x0400, 0x7bff] (nra_sweep.hip: bias 2048, "minus infinity" 1280)
        const int o2 = sc->gap_open2 + sc->gap_ext2;
        if (2 * sc->gap_ext1 > 256 || 2 * sc->gap_ext2 > 256 || 2 * (o2 + sc->mismatch + sc->sc_ambi) > 700) brute = true;
        // The taint scheme quadruples the scores: the same bounds at 4x, and the relaxed cell opens its one
        // gap state at o1 (= min(o1, o2): it shares the exact cell's substitution table).  Other schemes keep the doubled
        // cells of every sweep.  NRA_RELAX_C (tests, measurements): the margin, in bases; 0 turns the scheme off.
        p.relax_c = NRA_RELAX_C_DEFAULT;
        if (in.knobs.has_relax_c) p.relax_c = std::max(0, in.knobs.relax_c);
        if (p.relax_c > 0) p.relax_c = std::max(p.relax_c, 64);
        if ((in.flags & NRA_F_FULL_ANCHORS) || o1 > o2 || 4 * (sc->match + o1) > 127 || 4 * sc->gap_ext1 > 256 ||
            4 * sc->gap_ext2 > 256 || 4 * (o2 + sc->mismatch + sc->sc_ambi) > 700)
            p.relax_c = 0;
    }
    p.brute = brute;
}

// ---- the fitted model ---------------------------------------------------------------------------
// reads of more rows than this leave the one-block kernels for the chained ones (NRA_CHAIN_FROM: experiments)
int choose_chain_from(const PlanIn& in, bool brute)
{
    const nra_scoring_t* sc = in.sc;
    int chain_from = NRA_RING_MT_FROM;
    if (in.knobs.has_chain_from) chain_from = std::max(64, std::min(in.knobs.chain_from, NRA_MAX_QLEN_1BLOCK));
    const bool ring_units = [&] { for (int32_t g = 0; g < in.n_regions; ++g) if (in.regions[g].unit_len > NRA_SWEEP_RING_MAX_M) return false; return true; }();
    if (!ring_units || brute || (in.flags & (NRA_F_DPP_SWEEP | NRA_F_SERIAL_CHAIN))) chain_from = NRA_MAX_QLEN_1BLOCK;
    if (chain_from == NRA_RING_MT_FROM && !in.knobs.has_chain_from) {
        // The reads of (NRA_RING_MT_FROM, 3072] rows can go either way: one register block of 28 - 48 rows per lane -- one
        // wave per SIMD, padding in steps of 256 / 512 rows, 4.3 T cells/s x the fill of the launch's last round of the
        // SIMDs -- or row blocks of 12 .. 15 rows per lane, three waves per SIMD: 3.7 - 4.0 T cells/s (4.1 - 4.4 with two
        // blocks per read) once there are two rounds of them, 1.9 + 1.2 x rounds - 0.25 x (blocks per read - 2) below that
        // (the blocks of a read lag one another).  The model is fitted to tools/gpu_block_rows.py: on 1000 - 10 000 reads
        // of 1.6 - 3 kb it picks the faster form, or one within 3 %, in 54 of 54 cases
        // (profiles/r03_row_blocks_or_one_block_54_cases.txt); such reads run up to 37 % faster as blocks, config 5
        // 20.4 -> 17.3 ms.
        int64_t n_class = 0, rows_single = 0, rows_blocks[NRA_RING_MT_R + 1] = {0}, rows_class[NRA_RING_MT_R + 1] = {0};
        for (int32_t r = 0; r < in.n_reads; ++r) {
            const int q = in.reads[r].qlen;
            if (in.kmin[r] > in.kmax[r] || q <= NRA_RING_MT_FROM || max_score(sc, q) > kScoreCapBit) continue;
            for (int R = NRA_RING_MT_R_MIN; R <= NRA_RING_MT_R; ++R) {
                const int64_t rows = ((int64_t)q + 64 * R - 1) / (64 * R) * (64 * R);
                rows_blocks[R] += rows;
                if (q <= NRA_MAX_QLEN_1BLOCK) rows_class[R] += rows;
            }
            if (q <= NRA_MAX_QLEN_1BLOCK) { ++n_class; rows_single += 64 * (int64_t)kRList[rows_for_qlen(q)]; }
        }
        if (n_class > 0) {
            int R = NRA_RING_MT_R;
            for (int r2 = NRA_RING_MT_R - 1; r2 >= NRA_RING_MT_R_MIN; --r2) if (rows_blocks[r2] < rows_blocks[R]) R = r2;
            const double simds = (double)in.simds;
            const double waves = (double)((n_class + 1) / 2), nblk = (double)rows_class[R] / (64.0 * R) / (double)n_class;
            const double r1 = waves / simds, e1 = r1 / std::ceil(r1);
            const double r2 = waves * nblk / (3.0 * simds);
            const double t_single = (double)rows_single / (4.3 * e1);
            const double cap = 3.7 + 0.1 * (R - NRA_RING_MT_R_MIN) + (nblk < 2.5 ? 0.4 : 0.0);
            const double t_blocks = (double)rows_class[R] / std::min(cap, 1.9 + 1.2 * r2 - 0.25 * (nblk - 2.0));
            if (t_single <= t_blocks) chain_from = NRA_MAX_QLEN_1BLOCK;
        }
    }
    return chain_from;
}

// ---- chained flags ------------------------------------------------------------------------------
// Which reads leave the packed int16 sweeps for the chained int32 ones (one read per wave, any length):
// more rows than one register block, scores beyond the doubled int16 range, or a template whose
// extents do not fit the 16-bit payload of the int32 extents kernel.
int plan_chained(const PlanIn& in, int chain_from, Plan1D& p)
{
    const bool test_chain = in.test_chain();
    p.chained.assign((size_t)in.n_reads, 0);
    for (int32_t r = 0; r < in.n_reads; ++r) {
        if (in.kmin[r] > in.kmax[r]) continue;
        const int64_t ms = max_score(in.sc, in.reads[r].qlen);
        const int64_t tl = in.tlen(r);
        p.chained[r] = test_chain || in.reads[r].qlen > chain_from || ms > kScoreCapBit || tl > NRA_MAX_TLEN;
        if (p.brute && p.chained[r] && !test_chain) {
            // without the sweeps (flank-less region, unusual scoring, brute force on request) only what the
            // packed brute-force kernel holds can be scored
            if (in.reads[r].qlen > NRA_MAX_QLEN_1BLOCK || ms > kScoreCapPk16 || tl > NRA_MAX_TLEN)
                return fail(NRA_E_RANGE, "read " + std::to_string(r) + " (" + std::to_string(in.reads[r].qlen) +
                                             " bases) needs the junction decomposition: no brute force / ALL_EXTENTS, "
                                             "flanks >= 1, default-like scoring");
            p.chained[r] = 0;
        }
    }
    return NRA_OK;
}

// ---- reads to buckets ---------------------------------------------------------------------------
int route_reads(const PlanIn& in, Plan1D& p, Routing& rt)
{
    // the chained reads (every read with NRA_F_TEST_CHAIN): bucket kNumR = int32 cells, one read per wave;
    // bucket kNumR + 1 = packed int16, two reads per wave -- doubled scores up to 27000 (reads of up to 6750
    // bases with the default scoring) in the LDS-ring kernels, which hold units of up to NRA_SWEEP_RING_MAX_M
    // buckets kNumR + 2 + i: half-wave sweeps (k_sweep_ring32), i = index of the half's rows per lane in kRList
    std::vector<std::vector<int32_t>>& by_bucket = rt.by_bucket;
    by_bucket.assign((size_t)2 * kNumR + 2, std::vector<int32_t>());
    const bool ring_ok = (in.flags & NRA_F_DPP_SWEEP) == 0 && !p.brute;
    for (int32_t r = 0; r < in.n_reads; ++r) {
        if (in.kmin[r] > in.kmax[r] || in.reads[r].qlen == 0) continue;
        int bi = rows_for_qlen(in.reads[r].qlen);
        if (ring_ok && !p.chained[r] && in.reads[r].qlen <= 32 * NRA_RING32_MAX_R &&
            in.regions[in.reads[r].region].unit_len <= NRA_SWEEP_RING_MAX_M && (in.flags & NRA_F_NO_HALF_WAVE) == 0)
            bi = kNumR + 2 + rows_for_qlen(2 * in.reads[r].qlen);        // 32 * R >= qlen
        if (p.chained[r]) {
            const nra_region_t& rg = in.regions[in.reads[r].region];
            const bool packed = max_score(in.sc, in.reads[r].qlen) <= kScoreCapBit && rg.unit_len <= NRA_SWEEP_RING_MAX_M &&
                                (in.flags & NRA_F_DPP_SWEEP) == 0;
            bi = packed ? kNumR + 1 : kNumR;
            rt.chain_cols = std::max(rt.chain_cols, rg.left_len + rg.unit_len * in.kmax[r] + rg.right_len);
        }
        p.read_bucket[r] = bi;
        by_bucket[bi].push_back(r);
    }
    if ((!by_bucket[kNumR].empty() || !by_bucket[kNumR + 1].empty()) && p.brute)
        return fail(NRA_E_RANGE, "NRA_F_TEST_CHAIN needs the junction decomposition (no brute force / ALL_EXTENTS, flanks >= 1)");
    return NRA_OK;
}

// ---- folding and the straggler rule -------------------------------------------------------------
void fold_buckets(const PlanIn& in, int chain_from, Plan1D& p, Routing& rt)
{
    std::vector<std::vector<int32_t>>& by_bucket = rt.by_bucket;
    {   // small buckets fold into the next instantiation of their own kind
        std::vector<std::vector<int32_t>> full(by_bucket.begin(), by_bucket.begin() + kNumR);
        std::vector<std::vector<int32_t>> halfb(by_bucket.begin() + kNumR + 2, by_bucket.end());
        fold_small_buckets(full, 1024, 2);    // wider folding (up to 16384 reads / 4 rows) changes nothing in 1D
        fold_small_buckets(halfb, 2048, 2);
        for (int i = 0; i < kNumR; ++i) { by_bucket[i] = std::move(full[i]); by_bucket[kNumR + 2 + i] = std::move(halfb[i]); }
    }
    if (chain_from < NRA_MAX_QLEN_1BLOCK && !in.test_chain() && !by_bucket[kNumR + 1].empty()) {
        // ... and a handful of reads left in a one-block bucket above one row block (961 - 3072 bases, fewer than 256 of a
        // kind: 128 waves) joins the row blocks, where there are any: a length distribution that straddles
        // NRA_RING_MT_FROM would otherwise leave them a launch of their own (1000 reads of 1528 - 1582 bases, 24 of them
        // below the line: 4.2 ms against 2.7).  Larger buckets stay: two blocks pad a 1000-base read by half.
        for (int bi = 0; bi < kNumR; ++bi) {
            if (kRList[bi] <= NRA_RING_MT_R || by_bucket[bi].empty() || by_bucket[bi].size() >= 256) continue;
            for (int32_t r : by_bucket[bi]) {
                const nra_region_t& rg = in.regions[in.reads[r].region];
                rt.chain_cols = std::max(rt.chain_cols, rg.left_len + rg.unit_len * in.kmax[r] + rg.right_len);
                p.chained[r] = 1;
                p.read_bucket[r] = kNumR + 1;
                by_bucket[kNumR + 1].push_back(r);
            }
            by_bucket[bi].clear();
        }
    }
    p.chain_cap = (rt.chain_cols + 127) / 64 * 64 + 64;
}

// ---- per-bucket tasks ---------------------------------------------------------------------------
// kind of a bucket and its rows per lane, from its raw index bi and its reads
Bucket bucket_shape(const PlanIn& in, const Plan1D& p, int bi, const std::vector<int32_t>& members)
{
    const bool test_chain = in.test_chain();
    const std::vector<NraDevRead>& reads = in.reads;
    Bucket bk;
    bk.chain = bi == kNumR || bi == kNumR + 1;
    bk.wide = bi == kNumR;
    bk.half = bi >= kNumR + 2;
    if (bk.chain) {
        // LDS-ring chain unless a unit is too long for the ring (then the DPP chain, int32 only)
        bk.ring = (in.flags & NRA_F_DPP_SWEEP) == 0;
        for (int32_t r : members)
            if (in.regions[reads[r].region].unit_len > NRA_SWEEP_RING_MAX_M) bk.ring = false;
        bk.payload_R = test_chain ? NRA_CHAIN_R_TEST : NRA_CHAIN_R;
        // the row blocks of a read as concurrent waves (k_sweep_ringmt), unless one read alone would need more
        // strips than the scratch budget holds (then: one wave per read, block after block, two strips)
        bk.mt = bk.ring && (in.flags & NRA_F_SERIAL_CHAIN) == 0;
        if (bk.mt) {
            const int rows = 64 * (test_chain ? NRA_CHAIN_R_TEST : NRA_RING_MT_R_MIN);      // (the shortest block there is)
            int qmax = 0;
            for (int32_t r : members) qmax = std::max(qmax, reads[r].qlen);
            const size_t fit = (size_t)(NRA_CHAIN_SCRATCH_BUDGET / 2) / ((size_t)5 * 8 * (size_t)p.chain_cap);
            if ((size_t)((qmax + rows - 1) / rows) > fit + 1) bk.mt = false;
        }
        bk.R = test_chain ? NRA_CHAIN_R_TEST : (bk.mt ? NRA_RING_MT_R : bk.ring ? NRA_RING_CHAIN_R : NRA_CHAIN_R);
        if (bk.mt && !test_chain && !bk.wide) {
            // the block height that pads the bucket's reads least (ties: the taller block, fewer hand-offs; the int32
            // blocks of the longest reads stay at 15: 7.7 kb cores 96 ms against 102 ms at 14 with 0.5 % fewer cells)
            int64_t best = -1;
            for (int R = NRA_RING_MT_R; R >= NRA_RING_MT_R_MIN; --R) {
                int64_t rows = 0;
                for (int32_t r : members) rows += ((int64_t)reads[r].qlen + 64 * R - 1) / (64 * R) * (64 * R);
                if (best < 0 || rows < best) { best = rows; bk.R = R; }
            }
        }
    } else {
        bk.R = kRList[bk.half ? bi - kNumR - 2 : bi];
    }
    return bk;
}

// the reads of a bucket: their final bucket index, algorithmic cells, queue capacity, and the brute-force tasks
void bucket_candidates(const PlanIn& in, Plan1D& p, Bucket& bk, const std::vector<int32_t>& members)
{
    const int32_t *kmin = in.kmin, *kmax = in.kmax;
    const bool all_ext = in.all_ext();
    for (int32_t r : members) {
        p.read_bucket[r] = (int32_t)p.buckets.size();
        const NraDevRegion& d = p.dregs[in.reads[r].region];
        {   // algorithmic cells: q x sum over k of (|L| + m k + |R|)
            const int64_t K = (int64_t)kmax[r] - kmin[r] + 1;
            const int64_t sum_k = ((int64_t)kmin[r] + kmax[r]) * K / 2;
            p.alg_cells += (int64_t)in.reads[r].qlen * (K * ((int64_t)d.l1 + d.l3) + (int64_t)d.m1 * sum_k);
        }
        if (all_ext) {
            for (int32_t k = kmin[r]; k <= kmax[r]; ++k) {
                p.queue_tasks.push_back(NraTask{r, k, 0, (int32_t)(p.coff[r] + (uint32_t)(k - kmin[r]))});
                bk.cells_queue += sweep_cells(bk.R, d.l1 + d.m1 * k + d.l3);
            }
        }
        if (!all_ext && p.brute) {
            for (int32_t k = kmin[r]; k <= kmax[r]; k += 2) {
                NraPairTask t{};
                t.read = r; t.k1a = k; t.k2a = 0; t.out_a = (int32_t)(p.coff[r] + (uint32_t)(k - kmin[r]));
                if (k + 1 <= kmax[r]) { t.k1b = k + 1; t.k2b = 0; t.out_b = t.out_a + 1; }
                else { t.k1b = k; t.k2b = 0; t.out_b = -1; }
                t.flags = 0;
                p.pair_tasks.push_back(t);
                const int tl = d.l1 + d.m1 * (t.out_b >= 0 ? k + 1 : k) + d.l3;
                bk.cells_pair += 2 * sweep_cells(bk.R, tl);
            }
        }
        bk.queue_cap += (size_t)(kmax[r] - kmin[r] + 1);
    }
}

// the sweep tasks of a bucket: its reads paired (or, half-wave, grouped by four) by region and length
void bucket_sweep_tasks(const PlanIn& in, Plan1D& p, Bucket& bk, const std::vector<int32_t>& members)
{
    const std::vector<NraDevRead>& reads = in.reads;
    const int32_t *kmin = in.kmin, *kmax = in.kmax;
    std::vector<NraSweepTask>& sweep_tasks = p.sweep_tasks;
    // pair reads of one region by length: two reads share a wave (int16 halves)
    std::vector<int32_t> order(members);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        if (reads[x].region != reads[y].region) return reads[x].region < reads[y].region;
        return reads[x].qlen > reads[y].qlen;
    });
    bk.sweep_off = sweep_tasks.size();
    // the LDS-ring sweeps hold unit lengths up to NRA_SWEEP_RING_MAX_M; a bucket with a longer unit
    // keeps the DPP sweeps
    if (!bk.chain) {
        bk.ring = (in.flags & NRA_F_DPP_SWEEP) == 0;
        for (int32_t r : order)
            if (p.dregs[reads[r].region].m1 > NRA_SWEEP_RING_MAX_M) bk.ring = false;
        // the taint scheme: quadrupled scores <= 27000 in the packed cells (nra_pk16.h)
        bk.taint = bk.ring && p.relax_c > 0;
        for (int32_t r : order)
            if (4 * max_score(in.sc, reads[r].qlen) > 27000) bk.taint = false;
    }
    if (bk.half) {
        // four reads of a region per wave: two pairs, one per half, the union of their windows
        for (size_t i = 0; i < order.size();) {
            NraSweepTask t{};
            const int32_t g = reads[order[i]].region;
            int32_t quad[4] = {-1, -1, -1, -1};
            int nq = 0;
            while (nq < 4 && i < order.size() && reads[order[i]].region == g) quad[nq++] = order[i++];
            t.read_a = quad[0]; t.read_b = quad[1]; t.read_c = quad[2]; t.read_d = quad[3];
            t.kmin = kmin[quad[0]]; t.kmax = kmax[quad[0]];
            for (int j = 1; j < nq; ++j) { t.kmin = std::min(t.kmin, kmin[quad[j]]); t.kmax = std::max(t.kmax, kmax[quad[j]]); }
            const NraDevRegion& d = p.dregs[g];
            bk.cells_sweep += (int64_t)2 * 64 * bk.R * ((d.l1 + d.m1 * t.kmax + 31 * d.m1) + (d.l3 + 31));
            t.snap_off = p.snap_total;
            p.snap_total += (uint64_t)NRA_SNAP_LANE_STRIDE(bk.R) * 64;       // lane-major in the half-wave kernel
            sweep_tasks.push_back(t);
        }
    } else
    for (size_t i = 0; i < order.size();) {
        NraSweepTask t{};
        t.read_a = order[i]; t.read_b = -1; t.read_c = -1; t.read_d = -1;
        t.kmin = kmin[t.read_a]; t.kmax = kmax[t.read_a];
        // (the int32 chained sweeps take one read per wave)
        if (!bk.wide && i + 1 < order.size() && reads[order[i + 1]].region == reads[order[i]].region) {
            t.read_b = order[i + 1];
            t.kmin = std::min(t.kmin, kmin[t.read_b]);
            t.kmax = std::max(t.kmax, kmax[t.read_b]);
            i += 2;
        } else {
            i += 1;
        }
        const NraDevRegion& d = p.dregs[reads[t.read_a].region];
        int qmax = reads[t.read_a].qlen;
        if (t.read_b >= 0) qmax = std::max(qmax, reads[t.read_b].qlen);
        const int nblk = bk.chain ? (qmax + 64 * bk.R - 1) / (64 * bk.R) : 1;
        if (bk.ring)    // pipelines 64*m (forward) and 64 (reverse) columns deep, per row block
            bk.cells_sweep += (int64_t)nblk * (bk.wide ? 1 : 2) * 64 * bk.R *
                              ((d.l1 + d.m1 * t.kmax + 63 * d.m1) + (d.l3 + 63));
        else
            bk.cells_sweep += (int64_t)nblk * (bk.wide ? 1 : 2) * (sweep128_cells(bk.R, d.l1 + d.m1 * t.kmax) +
                                                                   sweep128_cells(bk.R, d.l3));
        t.snap_off = p.snap_total;
        p.snap_total += (uint64_t)nblk * 3 * bk.R * 64;
        sweep_tasks.push_back(t);
    }
    bk.n_sweep = (int)(sweep_tasks.size() - bk.sweep_off);
}

// ---- ringmt launch groups -----------------------------------------------------------------------
void ringmt_groups(const PlanIn& in, Plan1D& p, Bucket& bk)
{
    const std::vector<NraDevRead>& reads = in.reads;
    const std::vector<NraSweepTask>& sweep_tasks = p.sweep_tasks;
    std::vector<NraChainBlock>& chain_blocks = p.chain_blocks;
    // launch groups: as many tasks as the strip budget holds (one strip between consecutive blocks of a
    // task), each group's (task, block) list block-major: all blocks 0, then all blocks 1, ...
    const size_t fit = std::max<size_t>(1, (size_t)(NRA_CHAIN_SCRATCH_BUDGET / 2) / ((size_t)5 * 8 * (size_t)p.chain_cap));
    const int rows = 64 * bk.R;
    auto nblk_of = [&](const NraSweepTask& t) {
        int qmax = reads[t.read_a].qlen;
        if (t.read_b >= 0) qmax = std::max(qmax, reads[t.read_b].qlen);
        return std::max(1, (qmax + rows - 1) / rows);
    };
    size_t most_strips = 0;
    for (int t0 = 0; t0 < bk.n_sweep;) {
        size_t used = 0;
        int t1 = t0, max_blk = 0;
        std::vector<size_t> base;
        while (t1 < bk.n_sweep) {
            const int nb2 = nblk_of(sweep_tasks[bk.sweep_off + (size_t)t1]);
            if (t1 > t0 && used + (size_t)(nb2 - 1) > fit) break;
            base.push_back(used);
            used += (size_t)(nb2 - 1);
            max_blk = std::max(max_blk, nb2);
            ++t1;
        }
        const size_t first_block = chain_blocks.size();
        for (int blk = 0; blk < max_blk; ++blk)
            for (int t = t0; t < t1; ++t) {
                const int nb2 = nblk_of(sweep_tasks[bk.sweep_off + (size_t)t]);
                if (blk >= nb2) continue;
                const int32_t sb = (int32_t)base[(size_t)(t - t0)];
                chain_blocks.push_back(NraChainBlock{t, blk, nb2, blk > 0 ? sb + blk - 1 : -1,
                                                     blk < nb2 - 1 ? sb + blk : -1});
            }
        bk.mt_groups.push_back({first_block, (int)(chain_blocks.size() - first_block)});
        most_strips = std::max(most_strips, used);
        t0 = t1;
    }
    bk.n_strips = (int)most_strips;
    bk.strip_off = p.mt_strip_total;                     // (in strips of 5 * chain_cap granules)
    p.mt_strip_total += most_strips;
    p.chain_queue_cap = std::max(p.chain_queue_cap, bk.queue_cap);
}

void plan_buckets(const PlanIn& in, Plan1D& p, const Routing& rt)
{
    const std::vector<std::vector<int32_t>>& by_bucket = rt.by_bucket;
    // longest reads first: int32 chain, packed chain, full-wave R = 48 ... 1, then the half-wave buckets 16 ... 1
    std::vector<int> bucket_order{kNumR, kNumR + 1};
    for (int i = kNumR - 1; i >= 0; --i) bucket_order.push_back(i);
    for (int i = kNumR - 1; i >= 0; --i) bucket_order.push_back(kNumR + 2 + i);
    for (const int bi : bucket_order) {
        if (by_bucket[bi].empty()) continue;
        Bucket bk = bucket_shape(in, p, bi, by_bucket[bi]);
        bk.pair_off = p.pair_tasks.size();
        bk.queue_off = p.queue_total;
        bucket_candidates(in, p, bk, by_bucket[bi]);
        if (!p.brute) {
            bucket_sweep_tasks(in, p, bk, by_bucket[bi]);
            if (bk.chain && bk.mt) {
                ringmt_groups(in, p, bk);
            } else if (bk.chain) {
                // (two chained buckets at most -- packed and int32 -- share the budget)
                bk.n_strips = chain_strips((size_t)bk.n_sweep, bk.ring ? NRA_RING_CHAIN_STRIPS : NRA_CHAIN_STRIPS,
                                           (size_t)10 * 4 * (size_t)p.chain_cap, NRA_CHAIN_SCRATCH_BUDGET / 2);
                bk.strip_off = p.strip_total;
                p.strip_total += (size_t)bk.n_strips * 10 * (size_t)p.chain_cap;
                p.chain_queue_cap = std::max(p.chain_queue_cap, bk.queue_cap);
            }
        }
        bk.n_pair = (int)(p.pair_tasks.size() - bk.pair_off);
        bk.n_queue = in.all_ext() ? (int)bk.queue_cap : 0;
        p.queue_total += bk.queue_cap;
        p.queue_count.push_back(bk.n_queue);
        p.task_base.push_back((uint32_t)bk.queue_off);
        p.buckets.push_back(bk);
    }
    bool any_taint = false;
    for (const Bucket& bk : p.buckets) any_taint = any_taint || bk.taint;
    if (any_taint) {
        p.task_reads.resize(p.sweep_tasks.size());
        for (size_t t = 0; t < p.sweep_tasks.size(); ++t) {
            const NraSweepTask& x = p.sweep_tasks[t];
            p.task_reads[t] = (uint8_t)((x.read_a >= 0) + (x.read_b >= 0) + (x.read_c >= 0) + (x.read_d >= 0));
        }
    }
}

// ---- quanta ticket lists ------------------------------------------------------------------------
void plan_quanta(const PlanIn& in, Plan1D& p)
{
    const std::vector<NraDevRead>& reads = in.reads;
    // Quanta (k_sweep_ringq): for the unchained LDS-ring buckets of a batch whose tasks are few against the wave slots --
    // kernel-length tasks then end a launch with SIMDs holding 3 or 4 of them while others hold 2 or 3; with tens of
    // tasks per slot (BASELINE config 4) two launches already run at 0.98 of the issue ceiling and the states at the
    // cut (NRA_QSTATE_INTS(R) x 256 B a task) would only be traffic.
    std::vector<uint32_t>& qlist = p.qlist;
    size_t &q_tasks = p.q_tasks, &q_state = p.q_state, n_q_tasks_all = 0;
    for (const Bucket& bk : p.buckets) if (bk.ring && !bk.chain && !bk.mt) n_q_tasks_all += (size_t)bk.n_sweep;
    // Parts of NRA_Q_STEPS = 384 steps.  Measured on one box, ms per step (config 2 | 5000 reads | 20 000 reads of it):
    // no quanta 5.76 | 4.21 | 10.74; parts of 2048 (whole sweeps) 6.03; 1024 5.72; 768 5.32 | 3.39 | 9.93; 512 5.35 | 3.35 |
    // 9.95; 448 5.25; 384 5.22 | 3.20 | 9.93; 320 5.33; 256 5.46 | 3.58 | 10.43; 192 5.55; 128 5.54.  With more than
    // 8 tasks per SIMD the parts lose to two launches (40 000 reads 19.9 -> 20.2 ms, config 4 279 -> 285): the rule above.
    // (NRA_TEST_QSTEPS overrides the part size for such measurements and for the tests.)
    // Fewer tasks than SIMDs: a call's time is one task's chain of parts, every cut ~20 us of it (1000 reads: 1.99 -> 2.19 ms
    // per step with parts of 384): a reverse sweep, a forward sweep to its first cut and the rest then, as in this round's
    // first form.
    int q_steps_wanted = n_q_tasks_all < (size_t)in.simds ? NRA_Q_WHOLE : NRA_Q_STEPS;
    if (in.knobs.has_qsteps) q_steps_wanted = std::max(64, in.knobs.qsteps / 64 * 64);
    const bool want_quanta = (in.flags & (NRA_F_NO_QUANTA | NRA_F_DPP_SWEEP)) == 0 && n_q_tasks_all > 0 &&
                             n_q_tasks_all <= (size_t)8 * (size_t)in.simds;
    for (Bucket& bk : p.buckets) {
        if (!want_quanta || !bk.ring || bk.chain || bk.mt || bk.n_sweep <= 0) continue;
        bk.quanta = true;
        bk.q_off = qlist.size(); bk.q_task_off = q_tasks; bk.q_state_off = q_state;
        // Parts of `q_steps` steps (a multiple of 64; longer for sweeps that would make more than NRA_Q_MAX_PARTS of them).
        // Ticket order: every reverse sweep's part 0, task by task, then every part 1, ..., then the forward sweeps' parts
        // the same way -- a part's producers (the part before it; for a forward part at or behind the first boundary step
        // the task's whole reverse sweep) always hold smaller tickets.
        const NraSweepTask* bt = p.sweep_tasks.data() + bk.sweep_off;
        int max_steps = 0;
        std::vector<int> steps_rev((size_t)bk.n_sweep), steps_fwd((size_t)bk.n_sweep), cut_fwd((size_t)bk.n_sweep);
        for (int t = 0; t < bk.n_sweep; ++t) {
            const NraDevRegion& d = p.dregs[reads[bt[t].read_a].region];
            steps_rev[(size_t)t] = NRA_Q_STEPS_REV(d.l3, bk.half);
            steps_fwd[(size_t)t] = NRA_Q_STEPS_FWD(d.l1, d.m1, bt[t].kmax, bk.half);
            cut_fwd[(size_t)t] = NRA_Q_CUT(d.l1 + d.m1 * bt[t].kmin - 1);
            max_steps = std::max(max_steps, std::max(steps_rev[(size_t)t], steps_fwd[(size_t)t]));
            bk.q_fwd_steps += steps_fwd[(size_t)t];
        }
        bk.q_steps = std::max(q_steps_wanted, ((max_steps + NRA_Q_MAX_PARTS - 2) / (NRA_Q_MAX_PARTS - 1) + 63) / 64 * 64);
        for (int dir = 0; dir < 2; ++dir)
            for (int part = 0; part < NRA_Q_MAX_PARTS; ++part) {
                bool any = false;
                for (int t = 0; t < bk.n_sweep; ++t) {
                    // parts of this sweep: before the first cut (forward only), and from it on
                    const int cut = dir ? cut_fwd[(size_t)t] : 0, steps = dir ? steps_fwd[(size_t)t] : steps_rev[(size_t)t];
                    const int n_parts = (cut + bk.q_steps - 1) / bk.q_steps + std::max(1, (steps - cut + bk.q_steps - 1) / bk.q_steps);
                    if (part < n_parts) {
                        qlist.push_back(((uint32_t)dir << 31) | ((uint32_t)part << NRA_Q_PART_SHIFT) | (uint32_t)t);
                        any = true;
                    }
                }
                if (!any) break;
            }
        bk.n_quanta = (int)(qlist.size() - bk.q_off);
        q_tasks += 2 * (size_t)bk.n_sweep;
        int max_rev = 0;
        for (int v : steps_rev) max_rev = std::max(max_rev, v);
        q_state += (max_rev > bk.q_steps ? 2 : 1) * (size_t)bk.n_sweep * NRA_QSTATE_INTS(bk.R) * 64;
    }
    // (NRA_TEST_SAT=0 and NRA_TEST_SAT_STEPS in the environment, tests and measurements only: no saturation exit, and
    // the steps between its checkpoints)
    p.sat_steps = NRA_SAT_EXIT ? NRA_SAT_STEPS : -1;
    if (in.knobs.has_sat_steps) if (NRA_SAT_EXIT) p.sat_steps = std::max(0, in.knobs.sat_steps);
    if (in.knobs.has_sat) if (in.knobs.sat == 0) p.sat_steps = -1;
}

// ---- the clears rule ----------------------------------------------------------------------------
void plan_clears(const PlanIn& in, Plan1D& p)
{
    // Does a run have to clear cand_score and cand_flag first (run_1d)?  Not where the forward sweeps write both for
    // every candidate.  Per kernel family, from its `flush` (nra_sweep.hip): a task's sweep puts out one value per
    // repeat count of [task kmin, task kmax], the union of its reads' windows (the boundary of kcur leaves lane W - 1
    // while kcur <= kmax; the last, partial group of W is flushed behind the loop), and `flush` stores score (-1 below
    // min_score) and verdict for every read of the task whose window holds that count, under no other condition.
    // A half-wave task's empty upper half (`half_on`) has no reads.  The re-sweep only rewrites.
    // The table records that reading, family by family: a new family, or one whose `flush` changes, goes in with
    // `false` (its batches keep the clears) until its `flush` has been read again.
    enum Family { F_RING, F_RING32, F_RINGQ, F_RINGMT, F_RINGCHAIN, F_PK16, F_COUNT };
    static const bool kFlushWritesAll[F_COUNT] = {
        true,       // k_sweep_ring      (sweep_ring_body)
        true,       // k_sweep_ring32    (sweep_ring_body, HALF)
        true,       // k_sweep_ringq     (sweep_ring_body, QUANTA: the part that ends the forward sweep flushes the rest;
                    //                    the saturation exit flushes and writes every count from kcur to the task's kmax)
        true,       // k_sweep_ringmt    (the last row block's wave)
        true,       // k_sweep_ringchain (the last row block)
        true,       // k_sweep_pk16      (sweep_body; CHAIN: the last row block)
    };
    // not with brute force, NRA_F_ALL_EXTENTS or NRA_F_TIE_EXTENTS (no sweeps; the cleared flag 2 is what sends a
    // candidate to the extents kernel there), and every read with candidates has to be in a bucket (an empty read is
    // in none: its candidates keep the cleared -1)
    bool all = !p.brute && !in.all_ext() && (in.flags & NRA_F_TIE_EXTENTS) == 0;
    for (int32_t r = 0; r < in.n_reads && all; ++r) all = in.kmin[r] > in.kmax[r] || in.reads[r].qlen > 0;
    for (const Bucket& bk : p.buckets) {
        const Family f = bk.quanta ? F_RINGQ : bk.mt ? F_RINGMT : (bk.ring && bk.chain) ? F_RINGCHAIN
                       : (bk.ring && bk.half) ? F_RING32 : bk.ring ? F_RING : F_PK16;
        all = all && kFlushWritesAll[f];
    }
    p.sweeps_write_all = all;
}

// ---- statistics ---------------------------------------------------------------------------------
void plan_statistics(Plan1D& p)
{
    for (const Bucket& bk : p.buckets) {
        p.cells_pair += bk.cells_pair;
        p.cells_queue += bk.cells_queue;
        p.cells_sweep += bk.cells_sweep;
    }
}

}  // namespace

int plan_1d(const nra_region_t* regions, int32_t n_regions, const std::vector<NraDevRead>& reads, const int32_t* kmin,
            const int32_t* kmax, const nra_scoring_t* sc, int32_t flags, const Plan1DKnobs& knobs, int simds,
            PhaseClock& clk, Plan1D& p)
{
    const PlanIn in{regions, n_regions, reads, (int32_t)reads.size(), kmin, kmax, sc, flags, knobs, simds};
    int rc = plan_candidates(in, p);
    if (rc) return rc;
    rc = plan_templates(in, p);
    if (rc) return rc;
    // buckets by rows-per-lane; tasks
    plan_schemes(in, p);
    const int chain_from = choose_chain_from(in, p.brute);
    rc = plan_chained(in, chain_from, p);
    if (rc) return rc;
    clk.mark("  candidate offsets, templates, chained flags");
    Routing rt;
    rc = route_reads(in, p, rt);
    if (rc) return rc;
    clk.mark("  reads to buckets");
    fold_buckets(in, chain_from, p, rt);
    clk.mark("  small buckets folded");
    plan_buckets(in, p, rt);
    if (!p.brute) plan_quanta(in, p);
    plan_clears(in, p);
    plan_statistics(p);
    clk.mark("templates, buckets, tasks");
    return NRA_OK;
}

// ---- digest -------------------------------------------------------------------------------------
std::string plan_1d_digest(const Plan1D& p)
{
    Digest d;
    d.num("n_cands", p.n_cands);
    d.num("has_n", p.has_n);
    d.num("brute", p.brute);
    d.num("relax_c", p.relax_c);
    d.num("chain_cap", p.chain_cap);
    d.num("sat_steps", p.sat_steps);
    d.num("sweeps_write_all", p.sweeps_write_all);
    d.num("snap_total", (int64_t)p.snap_total);
    d.num("strip_total", (int64_t)p.strip_total);
    d.num("mt_strip_total", (int64_t)p.mt_strip_total);
    d.num("chain_queue_cap", (int64_t)p.chain_queue_cap);
    d.num("queue_total", (int64_t)p.queue_total);
    d.num("q_tasks", (int64_t)p.q_tasks);
    d.num("q_state", (int64_t)p.q_state);
    d.num("alg_cells", p.alg_cells);
    d.num("cells_pair", p.cells_pair);
    d.num("cells_queue", p.cells_queue);
    d.num("cells_sweep", p.cells_sweep);
    d.num("n_buckets", (int64_t)p.buckets.size());
    for (size_t i = 0; i < p.buckets.size(); ++i) {
        const Bucket& b = p.buckets[i];
        std::string v;
        auto add = [&](const char* k, int64_t x) { if (!v.empty()) v += ' '; v += k; v += '='; v += std::to_string(x); };
        add("R", b.R); add("chain", b.chain); add("wide", b.wide); add("half", b.half); add("payload_R", b.payload_R);
        add("strip_off", (int64_t)b.strip_off); add("n_strips", b.n_strips); add("mt", b.mt);
        add("n_pair", b.n_pair); add("pair_off", (int64_t)b.pair_off);
        add("n_queue", b.n_queue); add("queue_off", (int64_t)b.queue_off); add("queue_cap", (int64_t)b.queue_cap);
        add("n_sweep", b.n_sweep); add("sweep_off", (int64_t)b.sweep_off);
        add("ring", b.ring); add("quanta", b.quanta); add("taint", b.taint); add("q_fwd_steps", b.q_fwd_steps);
        add("q_off", (int64_t)b.q_off); add("q_task_off", (int64_t)b.q_task_off); add("q_state_off", (int64_t)b.q_state_off);
        add("n_quanta", b.n_quanta); add("q_steps", b.q_steps);
        add("cells_pair", b.cells_pair); add("cells_queue", b.cells_queue); add("cells_sweep", b.cells_sweep);
        v += " mt_groups=";
        for (size_t g = 0; g < b.mt_groups.size(); ++g)
            v += (g ? "," : "") + std::to_string(b.mt_groups[g].first) + ":" + std::to_string(b.mt_groups[g].second);
        if (b.mt_groups.empty()) v += "-";
        d.line(("bucket" + std::to_string(i)).c_str(), v);
    }
    d.array("region_kmax", p.region_kmax);
    d.array("coff", p.coff);
    d.array("read_bucket", p.read_bucket);
    d.array("chained", p.chained);
    d.array("pool", p.pool);
    d.array("dregs", p.dregs, [](Fnv& f, const NraDevRegion& x) {
        f.put(x.p1_off); f.put(x.p2_off); f.put(x.p3_off); f.put(x.pr_off);
        f.put(x.l1); f.put(x.m1); f.put(x.l2); f.put(x.m2); f.put(x.l3);
    });
    d.array("sweep_tasks", p.sweep_tasks, [](Fnv& f, const NraSweepTask& x) {
        f.put(x.read_a); f.put(x.read_b); f.put(x.kmin); f.put(x.kmax); f.put(x.snap_off); f.put(x.read_c); f.put(x.read_d);
    });
    d.array("pair_tasks", p.pair_tasks, [](Fnv& f, const NraPairTask& x) {
        f.put(x.read); f.put(x.k1a); f.put(x.k2a); f.put(x.k1b); f.put(x.k2b); f.put(x.out_a); f.put(x.out_b); f.put(x.flags);
    });
    d.array("queue_tasks", p.queue_tasks, [](Fnv& f, const NraTask& x) { f.put(x.read); f.put(x.k1); f.put(x.k2); f.put(x.out); });
    d.array("queue_count", p.queue_count);
    d.array("task_base", p.task_base);
    d.array("chain_blocks", p.chain_blocks, [](Fnv& f, const NraChainBlock& x) {
        f.put(x.task); f.put(x.blk); f.put(x.nblk); f.put(x.strip_in); f.put(x.strip_out);
    });
    d.array("qlist", p.qlist);
    d.array("task_reads", p.task_reads);
    return d.s;
}
