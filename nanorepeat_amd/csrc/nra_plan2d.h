// nra_plan2d.h -- the plan of a joint (2D) cell list: what is fixed when the reads are packed (Reads2D), what a batch
// carries from one cell list to the next (Carried2D, Pending2D), and the plan of one list in the two stages
// set_cells_common runs them in (plan_2d_strands before the strand-only kernels are enqueued, plan_2d_cells after), plus
// the plans of the two neighbours, nra_batch2d_sweep_flanks and nra_batch2d_refine.  Nothing here calls getenv or a hip*
// function: the keep budget, what the keep arena holds and the device's free memory come in as arguments (KeepInputs), so
// a plan can be made -- and tested -- without a device.
#ifndef NRA_PLAN2D_H
#define NRA_PLAN2D_H
#include "nra_plan1d.h"

#include <functional>

// 2D decomposition: reads of one bucket whose wave states fit the state buffer together; the
// prefix sweeps of a group run, then its tail sweeps, then the next group reuses the buffer.
struct JointGroup {
    int R = 0;
    int bucket = 0;
    int n_pre = 0, n_tail = 0;
    size_t pre_off = 0, tail_off = 0;
};

// k_joint_sweep (reverse and tail sweeps): the step loop stops when the lane of the read's last row has taken the last column
inline int64_t joint_cells(int R, int ncols, int qlen) { return (int64_t)64 * R * ((int64_t)ncols + std::min(63, std::max(qlen - 1, 0) / R)); }

// k1 values per MID-scan task (push_midscan; the static tasks of a refinement)
const int kMidscanChunk = 3;            // config 3, device ms per step: whole reads 6.23, 1: 6.23, 2: 6.18, 3: 6.15, 4: 6.16, 6: 6.40

using GridRow = NraGridRow;
// rows: the cells of every read.  keep: the repeat counts of every read the sweeps leave column states at, when these
// are kept for a later, finer grid (same layout: k1lo, n1 / k2lo, n2 at step 1; a superset of the read's cells).
struct JointGrid { int32_t step1, step2; const GridRow* rows; const GridRow* keep; };

// The reference's routing of reads to the cells of one grid round (nanoRepeat_joint.py:397-409 round 2, :315-330
// round 3): read r takes the grid values g of axis a with lo_a[r] <= g < hi_a[r]; none on one axis = no cells.
int route_grid(int32_t n_reads, int32_t start1, int32_t step1, int32_t count1, const double* lo1, const double* hi1,
               int32_t start2, int32_t step2, int32_t count2, const double* lo2, const double* hi2,
               std::vector<GridRow>& rows, int64_t& n_cells, std::vector<GridRow>* keep = nullptr);

// The joint region as a batch holds it.
struct Region2D {
    std::string left, unit1, mid, unit2, right;
};

// What is fixed when the reads are packed.
struct Reads2D {
    std::vector<uint8_t> chained_reads;
    // rows-per-lane bucket and partner of every read: the packed sweeps (k_joint_pk16) take two reads per wave, and the
    // state they leave at the end of L depends on the read and its strand only, so it is kept like the reverse sweeps
    // (lst_strand / lst_pending)
    std::vector<int32_t> jbucket, jpair_of;
    std::vector<NraJointPairTask> jpairs;
    bool jpack_l = false, jpack_r = false;
    uint64_t jpack_ints = 0;                   // int32 of one side's packed wave states
};
void plan_2d_reads(const std::vector<NraDevRead>& reads, int32_t left_len, int32_t right_len, const nra_scoring_t* sc,
                   int32_t flags, Reads2D& out);

// What a batch carries from one cell list to the next.
struct Carried2D {
    // the reverse sweep of a read (the R side of the junction, A) depends on the read, R and the strand only: a later
    // cell list of the same batch reuses it (rev_strand: strand it was made for, 0 = not made); lst_strand / rpk_strand:
    // the same for the packed sweeps of L / of rev(R) up to the window
    std::vector<int8_t> rev_strand, lst_strand, rpk_strand;
    // routed grids: the column states the prefix sweep (at every k1 of keep_rows) and the extended reverse sweep (at
    // every k2) left, kept for a later grid whose cells lie inside (nra_batch2d_invalidate / other strands drop them)
    bool keep_valid = false;
    std::vector<NraGridRow> keep_rows;
    std::vector<int8_t> keep_strand;
    std::vector<uint64_t> keep_state_off, keep_rs_off;
    std::vector<int32_t> keep_ra_off;
    bool joint_v2_prev = false;
    std::vector<NraGridRow> cur_rows;           // the current routed grid's rows (nra_batch2d_refine checks what a refinement can ask for)
    int32_t cur_step1 = 0, cur_step2 = 0;

    // the rows of the list whose buffers are on the device now (none: per-cell arrays)
    void set_current(const JointGrid* grid, int32_t n_reads)
    {
        cur_rows.clear();
        if (grid) { cur_rows.assign(grid->rows, grid->rows + n_reads); cur_step1 = grid->step1; cur_step2 = grid->step2; }
    }
    void init(int32_t n_reads)
    {
        rev_strand.assign((size_t)n_reads, 0); lst_strand.assign((size_t)n_reads, 0); rpk_strand.assign((size_t)n_reads, 0);
    }
    // Forget what earlier cell lists left for later ones (the reverse sweeps): the next list starts like the first.
    void invalidate()
    {
        std::fill(rev_strand.begin(), rev_strand.end(), (int8_t)0);
        std::fill(lst_strand.begin(), lst_strand.end(), (int8_t)0);
        std::fill(rpk_strand.begin(), rpk_strand.end(), (int8_t)0);
        keep_valid = false;
    }
};

// What the next run makes valid (given strands only: a probed strand is not known on the host).
struct Pending2D {
    std::vector<std::pair<int32_t, int8_t>> rev, lst, rpk;
    bool keep = false;
    void clear() { rev.clear(); lst.clear(); rpk.clear(); }
};
// the reverse sweeps enqueued by a run stay valid for later cell lists of this batch ... and so do the column states
void commit_2d(Carried2D& cd, Pending2D& pd);

// The inputs of the keep decision that the plan does not read itself.
struct KeepInputs {
    uint64_t budget = 0;                       // bytes (NRA_JOINT_KEEP_BUDGET_GB in the environment, or the built-in budget)
    bool keep_off = false;                     // this cell list keeps nothing (the retry after the kept states did not fit)
    uint64_t held = 0;                         // bytes the keep arena holds
    // what the device has free; asked only when the kept states pass the budget and need more than the arena holds.
    // false: the device did not say
    std::function<bool(uint64_t&)> device_free;
};

// One cell list: per-cell arrays (grid == NULL) or a routed grid.
struct Cells2D {
    const int8_t* read_strand = nullptr;
    int64_t n_cells = 0;
    const int32_t *cell_read = nullptr, *cell_k1 = nullptr, *cell_k2 = nullptr;
    const JointGrid* grid = nullptr;
};

struct Plan2D {
    // cells per read
    std::vector<uint32_t> first, cnt;
    int32_t k1max = 0, k2max = 0;              // of the cells
    int32_t k1max_pool = 0, k2max_pool = 0;    // of the template pool (kept column states reach further)
    int64_t tlmax = 0;
    // the forms of the list
    int keep = 0;                              // 0 = nothing kept, 1 = this list sweeps and keeps, 2 = no sweeps
    uint64_t keep_bytes = 0;
    bool device_asked = false;                 // the keep decision asked what the device has free
    bool brute = false, joint_v2 = false, joint_chain = false, cells_need_clear = true, all_strands_given = false;
    // templates and reads
    std::vector<uint8_t> pool;
    bool has_n = false;
    std::vector<NraDevRegion> dregs;
    std::vector<NraDevRead> reads;             // the batch's reads + the shadows of chained reads
    // buckets
    std::vector<std::vector<int32_t>> by_bucket;
    std::vector<int> bucket_ids;               // by_bucket index of every entry of `buckets`
    std::vector<Bucket> buckets;
    uint64_t state_cap = 0;
    // part 1: what depends on the reads and their strands only
    std::vector<NraPairTask> pair_tasks;
    std::vector<NraTask> probe_tasks;
    std::vector<int32_t> probe_count;
    std::vector<NraJointTask> jbwd;
    std::vector<NraJointPairTask> jlpk, jrpk;
    std::vector<uint8_t> pair_l, pair_r;
    std::vector<uint64_t> rs_off;
    std::vector<int32_t> ra_off;
    uint64_t rs_total = 0;
    int64_t ra_total = 0;
    int chain_cap = 0, payload_strips = 0;
    // part 2: the sweeps that depend on the cell list
    std::vector<NraTask> queue_tasks;
    std::vector<int32_t> queue_count;
    std::vector<NraJointTask> jpre, jtail;
    std::vector<int32_t> k1list;
    std::vector<NraJointCombineTask> jcomb;
    std::vector<JointGroup> jgroups;
    uint64_t fs_total = 0, state_base = 0;
    int64_t fb_total = 0;
    int64_t alg_cells = 0;
    nra_stats_t stats{};                       // the five a cell list sets
};

inline bool cells_2d_countable(int64_t n_cells) { return n_cells <= 0x7ff00000ll; }
// bytes of a cell list's arena: one chunk for everything but the wave states, which get their own
inline size_t cell_arena_bytes(size_t n_q2bit_words, int64_t n_cells, size_t pool_bytes, int32_t n_reads)
{
    return n_q2bit_words * 16 * 13 + (size_t)n_cells * 72 + pool_bytes + (size_t)n_reads * 256 + (8u << 20);
}

// Stage 1: cells per read, the limits, the keep decision, the template pool, the buckets, the part-1 tasks, the pending
// lists.  Returns NRA_OK, or an NRA_E_* with the error text set (nra_last_error).
int plan_2d_strands(const Region2D& reg, const std::vector<NraDevRead>& host_reads, bool reads_have_n, const Reads2D& rd,
                    int32_t flags, const Cells2D& cl, const KeepInputs& ki, PhaseClock& clk, Carried2D& cd,
                    Pending2D& pd, Plan2D& plan);
// Stage 2: the part-2 tasks, the groups, the totals, the statistics (warm_cells: of flank sweeps enqueued ahead of this
// list, 0 without).
void plan_2d_cells(const std::vector<NraDevRead>& host_reads, const Reads2D& rd, const Cells2D& cl, size_t n_q2bit_words,
                   int64_t warm_cells, Carried2D& cd, Plan2D& plan);

// nra_batch2d_sweep_flanks: per rows-per-lane bucket (pairs are listed bucket by bucket) the pairs whose reads all come
// with a strand and whose state is not valid for it.
struct FlankPart { int R; size_t off, n_l, n_r; };
struct FlankPlan {
    std::vector<FlankPart> parts;                  // the longest reads first, like the cell lists' buckets
    std::vector<NraJointPairTask> tasks;           // L- and R-side tasks of a pair next to each other; L marked in bit 63 of `state`
    std::vector<std::pair<int32_t, int8_t>> l_done, r_done;
    int64_t cells = 0;                             // cells these sweeps execute
};
// does this batch sweep flanks ahead of time at all?
inline bool sweeps_flanks_ahead(const Reads2D& rd, int32_t flags, int32_t left_len, int32_t right_len, int32_t n_reads)
{
    return !((flags & NRA_F_BRUTE_FORCE) != 0 || left_len < 1 || right_len < 2 || (!rd.jpack_l && !rd.jpack_r) || n_reads == 0);
}
void plan_2d_flanks(const Reads2D& rd, const Carried2D& cd, const int8_t* read_strand, int32_t left_len, int32_t right_len,
                    FlankPlan& out);
void commit_2d_flanks(Carried2D& cd, const FlankPlan& fp);      // once the sweeps are enqueued

// The forms of the current cell list, as nra_batch2d_refine reads them.
struct Forms2D { int keep; bool brute, joint_v2, joint_chain, all_strands_given; };
// nra_batch2d_refine: is the batch in the state for a refinement (run_open: a run is enqueued, nothing has waited for it,
// it carries no refinement yet), and does every count a read's refinement can ask for lie among the counts column states
// were kept at?  NRA_OK or NRA_E_STATE with the error text set.
int check_2d_refine(bool run_open, const Forms2D& f, const Carried2D& cd, const std::vector<Bucket>& buckets, int32_t n_reads,
                    int32_t buf1, int32_t buf2, const double* lo1, const double* hi1, const double* lo2, const double* hi2);
// ... and its static tasks: what a read's refinement needs whatever its round-2 size turns out to be
struct RefinePlan {
    std::vector<NraJointTask> mid;                 // bucket after bucket
    std::vector<NraJointCombineTask> comb;
    std::vector<size_t> mid_off, comb_off;         // per bucket (+ 1)
    std::vector<uint32_t> first;
    std::vector<int32_t> rowspad;
    uint64_t fs_total = 0;
    int64_t fb_total = 0;
};
int plan_2d_refine(const std::vector<NraDevRead>& host_reads, const Reads2D& rd, const Carried2D& cd,
                   const std::vector<Bucket>& buckets, int32_t buf1, int32_t buf2, RefinePlan& out);

// bytes a refinement adds to the cell list's arena
inline size_t refine_arena_bytes(uint64_t fs_total, int64_t cap, int32_t n_reads)
{
    return (size_t)fs_total * 4 + (size_t)cap * n_reads * 8 + (size_t)n_reads * 128 + (4u << 20);
}

// The parts of the digest: scalars, one line per bucket / group / part, length and 64-bit FNV-1a hash per array.
void digest_2d_reads(Digest& d, const Reads2D& rd);
void digest_2d_carried(Digest& d, const Carried2D& cd);
void digest_2d_cells(Digest& d, const Plan2D& plan, const Pending2D& pd, size_t expect);
void digest_2d_flanks(Digest& d, const FlankPlan& fp);
void digest_2d_refine(Digest& d, const RefinePlan& rp, size_t expect, int64_t n_cands);
// The steps of nra_plan2d_digest (nanorepeat_amd.h), played on one Reads2D + Carried2D without a device.
std::string plan_2d_digest(const nra_joint_region_t* reg, const std::vector<NraDevRead>& host_reads, bool reads_have_n,
                           size_t n_q2bit_words, const nra_scoring_t* sc, int32_t flags, const nra_plan2d_step_t* steps,
                           int32_t n_steps);

#endif  // NRA_PLAN2D_H
