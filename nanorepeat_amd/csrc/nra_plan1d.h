// nra_plan1d.h -- the plan of a 1D batch: everything nra_batch1d_create decides before it touches the device (candidate
// offsets, template pool, buckets, sweep tasks, launch groups, ticket lists, the clears rule, the statistics), and the
// helpers that planning shares with the rest of nra_host.cpp.  plan_1d calls neither getenv nor any hip* function: the
// environment knobs and the SIMD count come in as arguments, so a plan can be made -- and tested -- without a device.
#ifndef NRA_PLAN1D_H
#define NRA_PLAN1D_H
#include "nanorepeat_amd.h"
#include "nra_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

// NRA_DEBUG: wall time of the host phases of a create call
struct PhaseClock {
    bool on;                   // NRA_DEBUG / NRA_DEBUG_PHASES, as the caller read it
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit PhaseClock(bool on_) : on(on_) {}
    void mark(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[nra]   %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

const int kRList[] = {
#define X(r) r,
    NRA_R_LIST(X)
#undef X
};
const int kNumR = (int)(sizeof(kRList) / sizeof(kRList[0]));

inline int rows_for_qlen(int qlen)   // index into kRList, -1 if too long
{
    for (int i = 0; i < kNumR; ++i)
        if (64 * kRList[i] >= qlen) return i;
    return -1;
}

inline uint8_t encode_base(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return NRA_CODE_N;
    }
}

struct Bucket {
    int R = 0;
    bool chain = false;        // reads longer than one register block: chained row blocks
    bool wide = false;         // chained: int32 cells, one read per wave (else packed int16, two reads per wave)
    bool half = false;         // k_sweep_ring32: two read pairs per wave, 32 lanes each (R = rows per lane of a half; a ring bucket)
    int payload_R = 0;         // chained: row block of the extents kernel (NRA_CHAIN_R / NRA_CHAIN_R_TEST)
    size_t strip_off = 0;      // chained: this bucket's scratch strips in chain_sweep (int32 index)
    int n_strips = 0;
    bool mt = false;           // chained LDS-ring sweeps with the row blocks of a read as concurrent waves (k_sweep_ringmt)
    std::vector<std::pair<size_t, int>> mt_groups;   // launches: (first entry of chain_blocks, number of blocks)
    int n_pair = 0;            // pk16 tasks (1D score / 2D strand probe)
    size_t pair_off = 0;       // offset into pair_tasks
    int n_queue = 0;           // payload tasks prebuilt on the host (ALL_EXTENTS / 2D cells)
    size_t queue_off = 0;      // offset into queue_tasks (also the base of the tie queue)
    size_t queue_cap = 0;      // capacity of this bucket's queue region
    int n_sweep = 0;           // junction-decomposition tasks (pairs of reads)
    size_t sweep_off = 0;
    bool ring = false;         // k_sweep_ring (LDS hand-off) instead of k_sweep_pk16 (DPP hand-off)
    bool quanta = false;       // ... and its reverse and forward sweeps as ONE launch of quanta taken by ticket (k_sweep_ringq)
    bool taint = false;        // ... with the relaxed cell over the anchor columns far from the junction, and the exact re-sweep
                               // of the tasks it flags
    int64_t q_fwd_steps = 0;   // ... the steps of its forward sweeps (nra_batch1d_saturation)
    size_t q_off = 0, q_task_off = 0, q_state_off = 0;      // into q_list, q_words' arrivals (2 a task), q_state (int32, 2 slots a task)
    int n_quanta = 0, q_steps = 0;                            // entries of q_list; steps of a part
    int n_jbwd = 0;            // 2D decomposition: reverse sweeps (one per read)
    size_t jbwd_off = 0;
    int n_jlpk = 0, n_jrpk = 0;    // ... packed sweeps of the payload-free columns of L / rev(R) (one per pair of reads)
    size_t jlpk_off = 0, jrpk_off = 0;
    int n_comb = 0;            // 2D, junction at the end of mid: combine tasks (one per read)
    size_t comb_off = 0;
    int n_probe = 0;           // 2D, chained reads: strand-probe payload tasks (two per read)
    size_t probe_off = 0;
    int64_t cells_pair = 0;    // executed cells per run, pk16
    int64_t cells_queue = 0;   // executed cells per run, prebuilt payload queue
    int64_t cells_sweep = 0;   // executed cells per run, both sweeps
};

// Largest alignment score a read of qlen bases can reach, against what a cell format holds:
// int32 cells keep the score in their upper 16 bits; the packed int16 kernels keep value + 8192
// (brute force), two biased values added (chained sweep: 2 x 8192 + score), or the same with
// doubled scores (origin-bit sweep).
const int64_t kScoreCapI32 = 32000, kScoreCapPk16 = 24000, kScoreCapBit = 13500;
inline int64_t max_score(const nra_scoring_t* sc, int64_t qlen) { return (int64_t)sc->match * qlen; }

// A rows-per-lane bucket with few reads would run as its own under-filled launches: fold it into the
// next non-empty instantiation within `span` more rows per lane (the extra rows are padding).
inline void fold_small_buckets(std::vector<std::vector<int32_t>>& by_bucket, size_t min_reads, int span)
{
    for (int bi = 0; bi + 1 < kNumR; ++bi) {
        if (by_bucket[bi].empty() || by_bucket[bi].size() >= min_reads) continue;
        int up = -1;
        for (int bj = bi + 1; bj < kNumR && kRList[bj] <= kRList[bi] + span; ++bj)
            if (!by_bucket[bj].empty()) { up = bj; break; }
        if (up < 0) continue;
        by_bucket[up].insert(by_bucket[up].end(), by_bucket[bi].begin(), by_bucket[bi].end());
        by_bucket[bi].clear();
    }
}

// Scratch strips of a chained launch: one per wave, `bytes_per_strip` each (a few values per template column).  As
// many as there are tasks, at most `most`, and no more than fit the budget: a very wide template (up to
// NRA_MAX_TLEN_WIDE columns: 160 - 190 MB per strip) gets fewer waves, never none.
inline int chain_strips(size_t n_tasks, int most, size_t bytes_per_strip, size_t budget = NRA_CHAIN_SCRATCH_BUDGET)
{
    const size_t fit = std::max<size_t>(1, budget / std::max<size_t>(bytes_per_strip, 1));
    return (int)std::max<size_t>(1, std::min(std::min<size_t>(n_tasks, (size_t)most), fit));
}

// executed cells of one wave sweep with 64 cells in flight (k_score_pk16, payload, joint kernels):
// 64*R rows x (ceil((tlen+63)/64)*64) columns
inline int64_t sweep_cells(int R, int tlen) { return (int64_t)64 * R * (((int64_t)tlen + 126) / 64 * 64); }
// k_sweep_pk16: two virtual cells per lane, 128 in flight, the step loop stops with the last column
inline int64_t sweep128_cells(int R, int ncols) { return (int64_t)64 * R * ((int64_t)ncols + 127); }

inline uint32_t pool_append(std::vector<uint8_t>& pool, const char* s, int32_t len, const char* unit,
                            int32_t ulen, int32_t reps, bool& has_n)
{
    uint32_t off = (uint32_t)pool.size();
    for (int32_t i = 0; i < len; ++i) { uint8_t c = encode_base(s[i]); has_n |= c >= 4; pool.push_back(c); }
    for (int32_t k = 0; k < reps; ++k)
        for (int32_t i = 0; i < ulen; ++i) { uint8_t c = encode_base(unit[i]); has_n |= c >= 4; pool.push_back(c); }
    return off;
}

// The environment knobs of a 1D plan (tests, measurements), read once by the caller; `has_*`: the variable is set.
struct Plan1DKnobs {
    bool has_relax_c = false, has_chain_from = false, has_qsteps = false, has_sat = false, has_sat_steps = false;
    int relax_c = 0;           // NRA_RELAX_C
    int chain_from = 0;        // NRA_CHAIN_FROM (its presence alone switches the fitted model off)
    int qsteps = 0;            // NRA_TEST_QSTEPS
    int sat = 0;               // NRA_TEST_SAT
    int sat_steps = 0;         // NRA_TEST_SAT_STEPS
};

// What nra_batch1d_create decides before its first allocation and needs after it.
struct Plan1D {
    // candidates and templates
    std::vector<int32_t> region_kmax;          // per region: largest k of its reads
    std::vector<uint32_t> coff;                // per read (+ 1): its first candidate
    int64_t n_cands = 0;
    std::vector<uint8_t> pool;                 // template codes
    std::vector<NraDevRegion> dregs;
    bool has_n = false;                        // templates; the reads' share is known when the packing is over
    bool brute = false;                        // K independent alignments instead of the sweeps
    int relax_c = 0;                           // the taint scheme's margin; 0: off
    // reads to buckets
    std::vector<uint8_t> chained;
    std::vector<int32_t> read_bucket;          // index into `buckets`, -1: in none
    int chain_cap = 0;
    std::vector<Bucket> buckets;
    // tasks
    std::vector<NraSweepTask> sweep_tasks;
    std::vector<NraPairTask> pair_tasks;
    std::vector<NraTask> queue_tasks;          // ALL_EXTENTS only; otherwise just capacity
    std::vector<int32_t> queue_count;
    std::vector<uint32_t> task_base;
    std::vector<NraChainBlock> chain_blocks;
    std::vector<uint8_t> task_reads;           // per sweep task: its reads (where a bucket runs the taint scheme)
    uint64_t snap_total = 0;
    size_t strip_total = 0, mt_strip_total = 0, chain_queue_cap = 0, queue_total = 0;
    // quanta
    std::vector<uint32_t> qlist;
    size_t q_tasks = 0, q_state = 0;           // arrival counters; int32 of wave states at the cut
    int sat_steps = -1;
    // the clears rule
    bool sweeps_write_all = false;
    // statistics
    int64_t alg_cells = 0, cells_pair = 0, cells_queue = 0, cells_sweep = 0;
};

// `reads`: the layout alone (qlen and region of PackedReads::reads); the packed words may still be in the making.
// Returns NRA_OK, or an NRA_E_* with the error text set (nra_last_error).
int plan_1d(const nra_region_t* regions, int32_t n_regions, const std::vector<NraDevRead>& reads, const int32_t* kmin,
            const int32_t* kmax, const nra_scoring_t* sc, int32_t flags, const Plan1DKnobs& knobs, int simds,
            PhaseClock& clk, Plan1D& plan);

// ---- the writer of a plan's digest (shared with nra_plan2d.cpp)
// 64-bit FNV-1a over values fed field by field (struct padding never enters)
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n)
    {
        const unsigned char* s = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) { h ^= s[i]; h *= 1099511628211ull; }
    }
    template <class T> void put(T v) { bytes(&v, sizeof v); }
};

struct Digest {
    std::string s;
    void line(const char* key, const std::string& value) { s += key; s += ' '; s += value; s += '\n'; }
    void num(const char* key, int64_t v) { line(key, std::to_string(v)); }
    template <class T, class F> void array(const char* key, const std::vector<T>& v, F feed)
    {
        Fnv f;
        for (const T& x : v) feed(f, x);
        char buf[64];
        snprintf(buf, sizeof buf, "%zu %016llx", v.size(), (unsigned long long)f.h);
        line(key, buf);
    }
    template <class T> void array(const char* key, const std::vector<T>& v)
    {
        array(key, v, [](Fnv& f, const T& x) { f.put(x); });
    }
};

// The plan as text, one `key value` per line: scalars, one line per bucket, length and 64-bit FNV-1a hash per array.
std::string plan_1d_digest(const Plan1D& plan);

#endif  // NRA_PLAN1D_H
