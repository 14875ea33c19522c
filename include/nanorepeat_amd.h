/*
 * nanorepeat_amd.h -- C ABI of the MI355X-native NanoRepeat repeat-size scorer.
 *
 * This is the drop-in boundary for NanoRepeat's per-read repeat-size estimation
 * hot path.  The reference (WGLab/NanoRepeat 1.8.3) has no FFI: its boundary is
 * the string call `pyminimap2.main(cmd) -> (stdout, stderr)` with FASTA files on
 * disk, issued once per read (1D) or once per grid cell (2D).  Each entry point
 * below replaces one reference function together with the aligner calls it
 * makes; the file:line it replaces is cited on the declaration.
 *
 * Conventions: extern "C", plain pointers and sizes, caller-owned buffers,
 * returns 0 on success and a negative NRA_E_* code on failure (message via
 * nra_last_error(), thread-local).  Nothing throws across the boundary.  The
 * library must not be initialised before fork(); use one process per GPU.
 *
 * The scoring model is minimap2's documented `-x map-ont` objective
 * (match +2, mismatch -4, two-piece affine gap min(4+2l, 24+l), N = -1),
 * solved as an *optimal* local alignment.  See DESIGN.md for the exact
 * recurrences and tie-break rules; oracle/nr_oracle.c is the CPU restatement
 * the HIP kernels must match bit for bit.
 */
#ifndef NANOREPEAT_AMD_H
#define NANOREPEAT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRA_ABI_VERSION 4

/* error codes */
#define NRA_OK            0
#define NRA_E_ARG        -1   /* bad argument (null pointer, negative size, window too large ...) */
#define NRA_E_DEVICE     -2   /* HIP runtime error / no device */
#define NRA_E_RANGE      -3   /* a sequence exceeds what the entry point holds (limits on each declaration) */
#define NRA_E_NOMEM      -4
#define NRA_E_STATE      -5   /* the batch is not in the state the call needs (nra_batch2d_refine: the caller takes the two-call path) */

/* per-read status (1D and 2D) */
#define NRA_READ_OK        0  /* at least one best-scoring record passed the selector */
#define NRA_READ_FALLBACK  1  /* 1D only: records exist but no top-score record passes the flank
                                 test -> caller keeps round2_repeat_size (nanoRepeat_bam.py:433) */
#define NRA_READ_NO_RECORD 2  /* no candidate reached min_dp_score: the reference gets an empty PAF
                                 and leaves the read's size unset (nanoRepeat_bam.py:421) */
#define NRA_READ_SKIPPED   3  /* kmin > kmax on input: read has no round-2 estimate
                                 (nanoRepeat_bam.py:460) */

/* flags */
#define NRA_F_ALL_EXTENTS  1  /* explicit extents DP (tstart/tend) for EVERY candidate; implies brute force */
#define NRA_F_TIE_EXTENTS  2  /* explicit extents DP for every top-score tie, so cand_tstart/cand_tend are
                                 filled for them (the one-shot call sets it when those arrays are given);
                                 without it only ties whose flank verdict is ambiguous are re-run */
#define NRA_F_TEST_CHAIN   8  /* testing only: sweep every read in chained 128-row blocks (the mechanism reads
                                 longer than 3072 bases use with 1536-row blocks) */
#define NRA_F_DPP_SWEEP    16 /* testing / comparison: sweep unchained reads with k_sweep_pk16 (DPP hand-off, combine on
                                 every step) instead of k_sweep_ring (LDS hand-off, combine on every m-th step) */
#define NRA_F_NO_HALF_WAVE 32 /* testing / comparison: reads of up to 768 bases take one pair per wave (k_sweep_ring) instead of
                                 two pairs per wave, 32 lanes each (k_sweep_ring32) */
#define NRA_F_NO_JOINT_PACK 64 /* testing / comparison, 2D: sweep the columns outside the scoring window in the int32 payload
                                 cells too, instead of packed int16 cells with two reads per wave (k_joint_pk16) */
#define NRA_F_SERIAL_CHAIN 128 /* testing / comparison, 1D: sweep the row blocks of a long read one after the other in one wave
                                 (k_sweep_ringchain) instead of as concurrent waves (k_sweep_ringmt) */
#define NRA_F_JOINT_TAILS 256  /* testing / comparison, 2D routed grids: junction at R[0] and one tail sweep over mid + unit2^k2 per
                                 (read, k1) -- what explicit cell lists use -- instead of the junction at the end of mid (extended
                                 reverse sweeps, MID sweeps, k_joint_combine) */
#define NRA_F_JOINT_NO_CHAIN 512 /* testing / comparison, 2D routed grids: the MID part (last prefix column + mid) as one systolic sweep per
                                 (read, k1) resuming from the prefix sweep's wave state, instead of column-parallel scans
                                 (k_joint_midscan) on the column states the prefix sweep leaves */
#define NRA_F_JOINT_NO_KEEP 1024 /* testing / comparison, 2D routed grids: every grid of a batch sweeps its reads again, instead of keeping
                                 the column states a coarse grid's sweeps leave at EVERY repeat count of a read's range, from which a
                                 finer grid inside those ranges (the reference's round 3 after round 2) needs no sweep at all */
#define NRA_F_NO_QUANTA 2048  /* testing / comparison, 1D: a bucket's reverse sweeps and forward sweeps as two launches (k_sweep_ring /
                                 k_sweep_ring32) instead of one launch of quanta taken by ticket -- the sweeps cut into parts of a few
                                 hundred steps (k_sweep_ringq) */
#define NRA_F_QUANTA_2L 4096  /* accepted and ignored since the sweeps' quanta became parts of a few hundred steps (it ran the three
                                 quanta of round 4's first form as two launches without tickets: measured no better than no quanta) */
#define NRA_F_FULL_ANCHORS 8192 /* testing / comparison, 1D: the LDS-ring sweeps run the exact cell over every anchor column, instead of
                                 a relaxed upper-bound cell over the anchor columns far from the junction and an exact re-sweep of the
                                 read pairs where that bound may have reached a result (same results either way) */
#define NRA_F_BRUTE_FORCE  4  /* score the K candidates of a read as K independent alignments
                                 (k_score_pk16) instead of the junction decomposition (k_sweep_pk16) */

/* Scoring parameters: minimap2 `-x map-ont` defaults.
 * A gap of length l costs min(gap_open1 + l*gap_ext1, gap_open2 + l*gap_ext2). */
typedef struct nra_scoring {
    int32_t match;        /* +2  */
    int32_t mismatch;     /*  4  (penalty, positive) */
    int32_t gap_open1;    /*  4  */
    int32_t gap_ext1;     /*  2  */
    int32_t gap_open2;    /* 24  */
    int32_t gap_ext2;     /*  1  */
    int32_t sc_ambi;      /*  1  (penalty for N against anything) */
    int32_t min_dp_score; /* 80  records with a lower score are absent (minimap2 -s) */
} nra_scoring_t;

/* One 1D repeat region.  Candidate k is the sequence left + unit*k + right
 * (nanoRepeat_bam.py:478-481).  Sequences are ASCII (ACGTN, either case). */
typedef struct nra_region {
    const char* left;
    const char* unit;
    const char* right;
    int32_t left_len;
    int32_t unit_len;
    int32_t right_len;
} nra_region_t;

/* One joint (two adjacent motifs) region.  Candidate (k1,k2) is
 * left + unit1*k1 + mid + unit2*k2 + right (nanoRepeat_joint.py:499-505). */
typedef struct nra_joint_region {
    const char* left;
    const char* unit1;
    const char* mid;
    const char* unit2;
    const char* right;
    int32_t left_len;
    int32_t unit1_len;
    int32_t mid_len;
    int32_t unit2_len;
    int32_t right_len;
} nra_joint_region_t;

/* Work and timing counters of a batch (timings: HIP events on the streams the kernels run on). */
typedef struct nra_stats {
    int64_t n_alignments;     /* (read, candidate) pairs scored */
    int64_t algorithmic_cells;/* sum of qlen * tlen over those pairs */
    int64_t executed_cells;   /* DP cells the scoring kernels update as planned when the batch is created (padding
                                 included); far below algorithmic_cells when the junction decomposition shares work
                                 across k.  An upper bound: a 1D forward sweep that leaves through the saturation exit
                                 updates fewer (nra_batch1d_saturation reports the skipped steps of a run) */
    int64_t algorithmic_bytes;/* HBM bytes the algorithm must move (packed reads + flanks + results) */
    int64_t n_extent_tasks;   /* alignments re-run by the extents kernel (top-score ties) */
    double  score_kernel_ms;  /* dominant kernel: sum of its launches, HIP events on the batch stream */
    double  extent_kernel_ms; /* second-pass kernel (1D extents) */
    double  total_ms;         /* first launch -> last launch of the run, HIP events */
    int32_t n_score_launches;
    int32_t n_runs;           /* completed runs (nra_batch_run + nra_batch_sync) the sums below cover */
    double  score_phase_ms;   /* wall time of the scoring phase on the device (first scoring launch ->
                                 last one done); < score_kernel_ms when launches of different read-length
                                 buckets overlap on their own streams */
    /* the four timings above belong to the LAST run; these are summed over all n_runs runs */
    double  sum_score_kernel_ms, sum_extent_kernel_ms, sum_total_ms, sum_score_phase_ms;
    int64_t intermediate_bytes; /* HBM bytes the decomposition itself moves per run between its kernels: the R side
                                   of the junction (1D) / the wave states and the R side (2D), written once, read once */
} nra_stats_t;

typedef struct nra_batch nra_batch_t;   /* device-resident inputs + outputs of one call */

/* ---- library ------------------------------------------------------------------ */
int         nra_abi_version(void);
const char* nra_version(void);
const char* nra_last_error(void);
int         nra_device_count(void);              /* < 0 on error */
void        nra_default_scoring(nra_scoring_t* sc);
/* The library keeps a few device chunks (<= 2 GiB per device), pinned staging buffers, streams and events of
 * destroyed batches for the next call (hipMalloc / hipStreamCreate dominate a small one-shot call otherwise), and
 * gives the chunks back by itself when a device allocation fails.  This call gives them back now (device < 0: on
 * every device); batches that are alive are not touched. */
int         nra_release_cached_memory(int device);

/* ---- 1D: replaces round3_estimation(data_type, fast_mode, repeat_region, num_cpu)
 *      nanoRepeat_bam.py:446-450 (= round3_align :452-500, one pymm2.main call per
 *      read at :497, + round3_estimation_from_alignment :436-444) ---------------------
 *
 * Inputs: n_regions regions; n_reads oriented core sequences concatenated in `seqs`
 * with offsets seq_off[n_reads+1]; read_region[i] = region index of read i (NULL when
 * n_regions == 1); candidate window kmin[i]..kmax[i] inclusive (kmin > kmax = skipped).
 * A read holds at most 200 000 bases and a candidate template 4 000 000 columns (NRA_E_RANGE beyond).
 * Reads of up to 3072 bases run two to a wave in packed int16 cells; longer ones (any round-2 size
 * the reference's window rule covers, nanoRepeat_bam.py:463-472) run one to a wave as chained row
 * blocks in int32 cells and need the junction decomposition: no NRA_F_BRUTE_FORCE / ALL_EXTENTS.
 *
 * Per-read outputs (all caller-allocated, n_reads entries):
 *   best_score  max AS over the read's candidates (0 when no record)
 *   sum_k,n_ties  sum and count of k over the records tied at best_score that pass
 *               tstart < left_len && tlen - tend < right_len  (nanoRepeat_bam.py:426-428);
 *               the repeat size is sum_k / n_ties in float64 (= np.mean at :431)
 *   status      NRA_READ_*
 * Optional per-candidate outputs (NULL to skip), sum_i max(0, kmax-kmin+1) entries in
 * read order then k order: cand_score (AS, or -1 when below min_dp_score), cand_tstart,
 * cand_tend (-1 unless the candidate ties the best score -- NRA_F_TIE_EXTENTS, implied when
 * these arrays are given -- or NRA_F_ALL_EXTENTS is set). */
int nra_round3_1d(int device,
                  const nra_region_t* regions, int32_t n_regions,
                  int32_t n_reads, const char* seqs, const int64_t* seq_off,
                  const int32_t* read_region,
                  const int32_t* kmin, const int32_t* kmax,
                  const nra_scoring_t* sc, int32_t flags,
                  int32_t* best_score, int64_t* sum_k, int32_t* n_ties, uint8_t* status,
                  int32_t* cand_score, int32_t* cand_tstart, int32_t* cand_tend);

/* ---- 2D: replaces the aligner loop + selector of
 *      round2_estimation_of_repeat_size nanoRepeat_joint.py:397-421 and
 *      round3_estimation_of_repeat_size nanoRepeat_joint.py:315-347 (one pymm2.main
 *      call per grid cell at :417 / :341), followed by
 *      estimate_two_repeats_from_paf :427-478 and the CIGAR window rescoring
 *      tk.target_region_alignment_stats_from_cigar tk.py:435-500 ----------------------
 *
 * Inputs: one joint region; n_reads full reads (either strand, at most 200 000 bases; reads beyond
 * 3072 bases are scored uncut, cell by cell, in chained row blocks); a list of n_cells
 * (read, k1, k2) grid cells, grouped by read (cell_read non-decreasing).
 * read_strand (n_reads, in/out, may be NULL): 0 = choose the strand with the higher DP
 * score against the read's first listed cell (ties -> '+'), +1 / -1 = forced; on return
 * holds the strand used.
 *
 * Per-cell outputs (optional): cell_score = AS (-1 when below min_dp_score),
 * cell_wscore = window score over [max(0,L-10), min(tlen, L+m1*k1+mid+m2*k2+10))
 * (nanoRepeat_joint.py:445-449).  Per-read outputs: best_wscore, sum_k1, sum_k2, n_ties
 * over the cells tied at the maximum window score (:458-476), status OK / NO_RECORD. */
int nra_joint_2d(int device,
                 const nra_joint_region_t* region,
                 int32_t n_reads, const char* seqs, const int64_t* seq_off,
                 int8_t* read_strand,
                 int64_t n_cells, const int32_t* cell_read,
                 const int32_t* cell_k1, const int32_t* cell_k2,
                 const nra_scoring_t* sc, int32_t flags,
                 int32_t* cell_score, int32_t* cell_wscore,
                 int32_t* best_wscore, int64_t* sum_k1, int64_t* sum_k2,
                 int32_t* n_ties, uint8_t* status);

/* ---- generic batched local alignment: the DP engine of the path, exposed for the rows
 *      around it: anchor finding nanoRepeat_bam.py:260-286 (anchors vs
 *      reads, pymm2.main at :281) and the round-2 estimate :334-393 (cores vs left + unit*T,
 *      pymm2.main at :362), each of which is one aligner call over many reads in the reference.
 *
 * n_seqs sequences concatenated in `seqs` (offsets seq_off[n_seqs+1]); n_pairs pairs
 * (pair_query[i], pair_target[i]) of sequence indices.  A sequence used as a query holds at
 * most 200 000 bases (above 3072: chained row blocks), as a target at most 4 000 000 (a whole
 * long read as the target of an anchor); pairs whose score or extents outgrow the int32 cells
 * (score > 32000, target > 65000) run in int64 cells.  nra_align_pairs_cigar: query <= 3072,
 * target <= 65000.  Outputs per pair: score (AS; -1 when below
 * min_dp_score), tstart, tend (target coordinates, 0-based half-open; oracle tie-breaks:
 * largest tstart, then smallest tend; -1 when no record). */
int nra_align_pairs(int device,
                    int32_t n_seqs, const char* seqs, const int64_t* seq_off,
                    int64_t n_pairs, const int32_t* pair_query, const int32_t* pair_target,
                    const nra_scoring_t* sc, int32_t flags,
                    int32_t* score, int32_t* tstart, int32_t* tend);

/* ---- alignment paths in the reference's wire format: the same pairs as
 *      nra_align_pairs, plus the query extents and a minimap2-style --eqx CIGAR ("12=1X3I4D")
 *      of the co-optimal path the oracle's traceback picks (paf.py:32-79 carries it as cg:Z).
 * cigar: caller buffer of cigar_cap bytes; pair i's NUL-terminated string starts at
 * cigar + cigar_off[i] (cigar_off has n_pairs + 1 entries; empty string when no record).
 * The trace needs qlen * tlen bytes of device memory per pair (8 GiB per call at most). */
int nra_align_pairs_cigar(int device,
                          int32_t n_seqs, const char* seqs, const int64_t* seq_off,
                          int64_t n_pairs, const int32_t* pair_query, const int32_t* pair_target,
                          const nra_scoring_t* sc, int32_t flags,
                          int32_t* score, int32_t* tstart, int32_t* tend,
                          int32_t* qstart, int32_t* qend,
                          char* cigar, int64_t cigar_cap, int64_t* cigar_off);

/* The same call for queries of any length: arguments and outputs as nra_align_pairs_cigar, query <= 200 000 bases,
 * target <= 65 000, qlen * tlen bytes of trace per pair and 8 GiB per call at most (NRA_E_RANGE beyond any of these,
 * before the device is touched).  A query beyond 3072 bases is filled in row blocks of 1536 rows, each a wave of its
 * own, chained like the sweeps of nra_round3_1d; a pair whose score may pass 32 000 runs in 64-bit cells.  Every
 * output equals the oracle's traceback bit for bit.  DESIGN.md section 21. */
int nra_align_paths(int device,
                    int32_t n_seqs, const char* seqs, const int64_t* seq_off,
                    int64_t n_pairs, const int32_t* pair_query, const int32_t* pair_target,
                    const nra_scoring_t* sc, int32_t flags,
                    int32_t* score, int32_t* tstart, int32_t* tend,
                    int32_t* qstart, int32_t* qend,
                    char* cigar, int64_t cigar_cap, int64_t* cigar_off);

/* ---- device-resident batches (what bench.py times): create = encode + H2D,
 *      run = kernels only (asynchronous on the batch's own stream), fetch = D2H ------- */
int  nra_batch1d_create(int device,
                        const nra_region_t* regions, int32_t n_regions,
                        int32_t n_reads, const char* seqs, const int64_t* seq_off,
                        const int32_t* read_region,
                        const int32_t* kmin, const int32_t* kmax,
                        const nra_scoring_t* sc, int32_t flags,
                        nra_batch_t** out);
int  nra_batch2d_create(int device,
                        const nra_joint_region_t* region,
                        int32_t n_reads, const char* seqs, const int64_t* seq_off,
                        const int8_t* read_strand,
                        int64_t n_cells, const int32_t* cell_read,
                        const int32_t* cell_k1, const int32_t* cell_k2,
                        const nra_scoring_t* sc, int32_t flags,
                        nra_batch_t** out);
/* The joint mode scores the same reads in two grid rounds (nanoRepeat_joint.py:266-269): the reads can be
 * packed and uploaded once (create_reads) and each round's cell list set on the resident batch
 * (set_cells; may be called again after a run -- device buffers are reused).  nra_batch2d_create is the two
 * calls in one. */
int  nra_batch2d_create_reads(int device,
                              const nra_joint_region_t* region,
                              int32_t n_reads, const char* seqs, const int64_t* seq_off,
                              const nra_scoring_t* sc, int32_t flags,
                              nra_batch_t** out);
int  nra_batch2d_set_cells(nra_batch_t* b, const int8_t* read_strand,
                           int64_t n_cells, const int32_t* cell_read,
                           const int32_t* cell_k1, const int32_t* cell_k2);
/* A whole grid round in one call -- the reference's routing of reads to grid cells, done by the library
 * (round 2: nanoRepeat_joint.py:397-409, round 3: :315-330).  Axis a (1, 2) has the grid values
 * g = start_a + i * step_a, i in [0, count_a) (round 2: range(round1_min, round1_max + 1, step), :397-398;
 * round 3: range(max(0, int(min size - s)), int(max size + s + 2)), :298-303); read r takes the values with
 * lo_a[r] <= g < hi_a[r] (round 2: its round-1 range [min, max), :407; round 3: [max(size - s, range min),
 * min(size + s, range max)), :325-330 -- doubles, because the round-2 sizes are means), and no cells when either
 * axis gives it none.  A read's cells are listed k1-major, k2 ascending, reads in input order: the order
 * nra_batch2d_set_cells wants and the per-cell arrays of nra_batch2d_fetch follow.
 * nra_joint_grid_cells is the routing alone, on the host (no device needed): returns the number of cells and, when
 * the three arrays are given (cap entries each), the list itself.  nra_batch2d_set_grid = the routing + set_cells,
 * without per-cell arrays crossing the boundary; *n_cells (optional) receives the number of cells. */
int64_t nra_joint_grid_cells(int32_t n_reads,
                             int32_t start1, int32_t step1, int32_t count1, const double* lo1, const double* hi1,
                             int32_t start2, int32_t step2, int32_t count2, const double* lo2, const double* hi2,
                             int64_t cap, int32_t* cell_read, int32_t* cell_k1, int32_t* cell_k2);
int  nra_batch2d_set_grid(nra_batch_t* b, const int8_t* read_strand,
                          int32_t start1, int32_t step1, int32_t count1, const double* lo1, const double* hi1,
                          int32_t start2, int32_t step2, int32_t count2, const double* lo2, const double* hi2,
                          int64_t* n_cells);
/* A later cell list reuses what an earlier one left on the device for the same read and strand: the packed sweeps of
 * the two flanks, and -- routed grids with every strand given -- the column states on either side of the junction, which
 * a grid's sweeps leave at EVERY repeat count k with lo_a[r] <= k < hi_a[r] (no further than one step beyond the read's
 * first / last grid value), not only at the grid's own values: a later grid whose cells all lie inside (round 3 after
 * round 2) runs no sweep at all (results identical; NRA_F_JOINT_NO_KEEP switches this off).  nra_batch2d_invalidate
 * drops all of it: the next list starts like the first (a benchmark repeating the two rounds on one resident batch
 * calls it at the top of every repetition). */
int  nra_batch2d_invalidate(nra_batch_t* b);
/* The flank sweeps ahead of the cell list.  What a joint run sweeps first -- L and rev(R) up to the scoring window, a third
 * of a round's device time -- depends on the reads and their strands only.  A caller that knows every strand (round 1 of
 * the reference does, nanoRepeat_joint.py:509-649) calls this right after nra_batch2d_create_reads / _invalidate, BEFORE it
 * derives step sizes, bounds and grids on the host (:239-259, :351-374): the kernels are enqueued and the call returns;
 * the cell lists that follow find the flank states valid for those strands and sweep no flank (a read with strand 0
 * here, or another strand later, is swept by its cell list as before).  Results are identical with and without the
 * call; a batch that sweeps no packed flanks (brute force, short flanks) does nothing. */
int  nra_batch2d_sweep_flanks(nra_batch_t* b, const int8_t* read_strand);
/* The reference's round 3 (round3_estimation_of_repeat_size, nanoRepeat_joint.py:275-349) as a REFINEMENT of the routed
 * grid whose run has just been enqueued (set_grid -> nra_batch_run -> this call, before anything waits for the run):
 * routed on the device from that grid's per-read results, without the host seeing them.  Read r with a result (status
 * OK, n_ties > 0) has the sizes size_a = sum_ka / n_ties (float64, the mean of its tied cells, :473-474) and takes the
 * unit-step cells k_a with  max(size_a - buf_a, lo_a[r]) <= k_a < min(size_a + buf_a, hi_a[r])  on both axes (:320-330:
 * buf_a = the grid's step on axis a, [lo, hi) = the read's round-1 range, the bounds the grid was routed with; lo >= 0);
 * a read without a result takes none.  The cells are scored from the column states the grid's sweeps kept (no sweep
 * runs), and the per-read outputs of nra_batch2d_fetch are then the refinement's (status NO_RECORD for a read without
 * cells); its per-cell arrays hold (2 buf1)(2 buf2) entries a read, the read's n1 x n2 cells first (k1-major),
 * and nra_stats_t.n_alignments counts the cells of both grids.  What the host saves: a fetch, a second routing and task
 * list, and the idle device between the two rounds.  NRA_E_STATE when the batch kept no column states for its current
 * grid (strands not all given, explicit cell list, NRA_F_JOINT_NO_KEEP / _TAILS / _NO_CHAIN, reads beyond 3072 bases,
 * kept states over budget), when some read's refinement could reach a count no column state was kept at (other buffers or
 * bounds than the grid's; a grid that itself ran from the states an earlier grid kept), or when the run was already waited
 * for: the caller then fetches and calls nra_batch2d_set_grid for the finer grid itself -- same results. */
int  nra_batch2d_refine(nra_batch_t* b, int32_t buf1, int32_t buf2,
                        const double* lo1, const double* hi1, const double* lo2, const double* hi2);
int  nra_batch_run(nra_batch_t* b);      /* enqueue every kernel of the path; returns at once */
int  nra_batch_sync(nra_batch_t* b);     /* wait for the batch stream */
int  nra_batch_stats(nra_batch_t* b, nra_stats_t* st);   /* after sync */
int  nra_batch1d_fetch(nra_batch_t* b,
                       int32_t* best_score, int64_t* sum_k, int32_t* n_ties, uint8_t* status,
                       int32_t* cand_score, int32_t* cand_tstart, int32_t* cand_tend);
/* 1D, after sync: how many sweep tasks (read pairs, or two pairs of the half-wave sweeps) and reads the relaxed anchor
 * columns sent to the exact re-sweep in the last run, and how many there were in all (0 / 0 with NRA_F_FULL_ANCHORS) */
int  nra_batch1d_resweeps(nra_batch_t* b, int64_t* tasks, int64_t* reads, int64_t* tasks_total, int64_t* reads_total);
/* 1D, after sync: the saturation exit of the forward sweeps in quanta in the last run (additive, ABI 4).  A sweep whose wave
 * state repeats from one unit boundary to the next ends there and writes its last value for every repeat count left.
 * *sweeps: sweep tasks that left that way, *steps: the sweep steps they skipped; *sweeps_total, *steps_total: the forward
 * sweeps in quanta of the batch and their steps as planned (0 / 0 where no bucket runs in quanta) */
int  nra_batch1d_saturation(nra_batch_t* b, int64_t* sweeps, int64_t* steps, int64_t* sweeps_total, int64_t* steps_total);
/* 1D: which per-candidate arrays a run of this batch clears before its kernels start (additive, ABI 4; for tests and
 * measurements).  *scores: cand_score and the flank verdicts -- 0 where every bucket's forward sweeps write them for every
 * candidate; *extents: cand_tstart / cand_tend -- 0 where the selection kernel sets them to -1 on its way */
int  nra_batch1d_clears(nra_batch_t* b, int32_t* scores, int32_t* extents);
/* 1D: the plan nra_batch1d_create would make for these inputs on a device of `simds` SIMDs (1024 on MI355X), as text, on
 * the host (no device needed; additive, ABI 4; for tests and measurements).  One `key value` per line: the plan's scalars,
 * one line per bucket, and for every array its length and a 64-bit FNV-1a hash over its values.  Writes at most cap bytes
 * (0-terminated) to buf and returns the bytes the whole text needs, or a negative NRA_E_* like the create call. */
int64_t nra_plan1d_digest(const nra_region_t* regions, int32_t n_regions,
                          int32_t n_reads, const char* seqs, const int64_t* seq_off,
                          const int32_t* read_region, const int32_t* kmin, const int32_t* kmax,
                          const nra_scoring_t* sc, int32_t flags, int32_t simds, char* buf, int64_t cap);
/* 2D: the plans a joint batch of these reads would make for a sequence of steps, as text, on the host (no device needed;
 * additive, ABI 4; for tests and measurements).  The steps are played in order on what a batch carries from one cell list
 * to the next; after each the batch counts as run and waited for.  A step carries its own inputs: its strands (or NULL),
 * its cells / grid / bounds and buffers, the keep budget in bytes and a stand-in for the device's free bytes; what the
 * keep arena holds is what the last keeping step asked for.  Per step: the plan's scalars, one line per bucket and per
 * group of sweeps, for every array of the plan and of the carried state its length and a 64-bit FNV-1a hash over its
 * values -- or the step's error code and text.  Buffer and return value as nra_plan1d_digest. */
#define NRA_PLAN2D_CELLS 0        /* nra_batch2d_set_cells */
#define NRA_PLAN2D_GRID 1         /* nra_batch2d_set_grid */
#define NRA_PLAN2D_SWEEP_FLANKS 2 /* nra_batch2d_sweep_flanks */
#define NRA_PLAN2D_REFINE 3       /* nra_batch2d_refine (behind the step before it, as if that one was not waited for) */
#define NRA_PLAN2D_INVALIDATE 4   /* nra_batch2d_invalidate */
typedef struct {
    int32_t kind;
    const int8_t* read_strand;
    int64_t n_cells;                                        /* cell list */
    const int32_t *cell_read, *cell_k1, *cell_k2;
    int32_t start1, step1, count1, start2, step2, count2;   /* grid */
    const double *lo1, *hi1, *lo2, *hi2;                    /* grid, refinement */
    int32_t buf1, buf2;                                     /* refinement */
    int64_t keep_budget, device_free;                       /* bytes */
} nra_plan2d_step_t;
int64_t nra_plan2d_digest(const nra_joint_region_t* region, int32_t n_reads, const char* seqs, const int64_t* seq_off,
                          const nra_scoring_t* sc, int32_t flags, const nra_plan2d_step_t* steps, int32_t n_steps,
                          char* buf, int64_t cap);
int  nra_batch2d_fetch(nra_batch_t* b, int8_t* read_strand,
                       int32_t* cell_score, int32_t* cell_wscore,
                       int32_t* best_wscore, int64_t* sum_k1, int64_t* sum_k2,
                       int32_t* n_ties, uint8_t* status);
void nra_batch_destroy(nra_batch_t* b);

/* ---- anchor screen: which regions' anchors a read carries (FASTQ / FASTA input) ------------
 *      replaces the genome-wide mapping of preprocess_fastq (nanoRepeat.py:41-76) and the BAM
 *      window fetch of extract_fastq_from_bam (nanoRepeat_bam.py:577-600) as the choice of the
 *      reads each region sees; the anchor check (find_anchor_locations_in_reads) still decides.
 *
 * A k-window counts when all its bases are ACGT (either case); canon(w) = min(code(w), code(revcomp(w))),
 * 2 bits per base (A=0 C=1 G=2 T=3), first base most significant.  K(g, s) = the distinct canonical k-mers of
 * side s (0 left, 1 right) of region g, without periodic k-mers (w[i] == w[i+p] for all i, some p in 1..6) and
 * without k-mers found in more than max_occ of the 2 * n_regions sets.  c(r, g, s) = the window positions of read
 * r whose canonical k-mer is in K(g, s).  Pair (r, g) passes when c(r,g,s) >= min(min_hits, |K(g,s)|) on both
 * sides: a region whose two sets are empty takes every read.  DESIGN.md section 13. */
typedef struct nra_screen nra_screen_t;

typedef struct nra_screen_stats {
    int64_t n_keys;            /* distinct canonical k-mers in the index */
    int64_t n_postings;        /* (k-mer, region side) entries of the index */
    int64_t n_masked_periodic; /* distinct periodic k-mers of the anchors, left out */
    int64_t n_masked_max_occ;  /* distinct k-mers in more than max_occ sets, left out */
    int64_t n_empty_regions;   /* regions both of whose sets are empty: every read passes them */
    int64_t index_bytes;       /* device bytes of the table and the postings */
    int64_t bases_screened;    /* read bases over every nra_screen_reads / _partial call */
    int64_t n_calls;           /* nra_screen_reads / _partial calls that succeeded */
    double  build_ms;          /* host time of the index build in nra_screen_create */
    double  kernel_ms;         /* screen kernels of the last call (HIP events) */
    double  sum_kernel_ms;     /* ... summed over n_calls */
    int64_t n_classes;         /* motif classes of the last nra_screen_set_motifs (0 without one) */
    double  motif_kernel_ms;   /* k_screen_motifs of the last nra_screen_reads_partial call (HIP events) */
    double  sum_motif_kernel_ms; /* ... summed over the nra_screen_reads_partial calls */
} nra_screen_stats_t;

/* anchors 2g / 2g+1 = left / right anchor of region g: bytes [anchor_off[i], anchor_off[i+1]) of `anchors`
 * (2 * n_regions + 1 offsets).  k odd in 11..15, max_occ in 1..255.  Builds the index on the host, keeps it on
 * the device; the handle serves any number of nra_screen_reads calls (one at a time). */
int nra_screen_create(int device, int32_t n_regions, const char* anchors, const int64_t* anchor_off,
                      int32_t k, int32_t max_occ, nra_screen_t** out);
/* n_reads reads, bytes [seq_off[i], seq_off[i+1]) of `seqs`; min_hits >= 1.  Writes the passing pairs sorted by
 * read, then region, with c(r, g, left) and c(r, g, right).  *n_pairs is the capacity of the four arrays on entry
 * and the number of pairs on return; when the pairs exceed the capacity the call writes none, leaves the number
 * needed in *n_pairs and returns NRA_E_RANGE. */
int nra_screen_reads(nra_screen_t* s, int32_t n_reads, const char* seqs, const int64_t* seq_off, int32_t min_hits,
                     int64_t* n_pairs, int32_t* pair_read, int32_t* pair_region,
                     int32_t* hits_left, int32_t* hits_right);
int nra_screen_stats(const nra_screen_t* s, nra_screen_stats_t* st);
int nra_screen_destroy(nra_screen_t* s);

/* ---- motif screen: one-anchor and in-repeat reads (additive, ABI 4) ----
 *
 * Windows, code, canon, K(g, s) and c(r, g, s) are those above.
 * Motif classes.  The root of a motif (upper-cased ACGT) is its shortest word w with motif = w^j.  Two roots are in
 * one class when one is a rotation of the other or of its reverse complement.  A region whose root is longer than 6
 * bases has no class: class_of[g] = -1, which is not an error.
 * Periodic windows.  A valid k-window w has period q when w[i] == w[i+q] for all i < k - q.  Its smallest period p in
 * 1..6, if any, makes it a window of the class of w[0:p] (w[0:p] is then primitive).  m(r, C) = the window positions
 * of read r that are windows of class C.  W(r) = max(0, len(r) - k + 1) counts every position, valid or not.
 * Pairs.  pass(s): |K(g,s)| > 0 and c(r,g,s) >= min(min_hits, |K(g,s)|).  nra_screen_reads_partial returns, sorted by
 * read then region, every pair (r, g) of one of four kinds:
 *   0  both anchors  exactly the pairs nra_screen_reads returns for the same arguments (regions with empty sets
 *                    included)
 *   1  left only     pass(left), the right set is not empty, and not pass(right)
 *   2  right only    pass(right), the left set is not empty, and not pass(left)
 *   3  in repeat     none of the above, class_of[g] >= 0, W(r) >= 1 and
 *                    m(r, class_of[g]) >= max(min_hits, ceil(motif_share_pct * W(r) / 100))
 * Every pair carries hits_left = c(r,g,left), hits_right = c(r,g,right) and motif_windows = m(r, class_of[g]), 0
 * without a class. */

/* The motif of region g = bytes [motif_off[g], motif_off[g+1]) of `motifs`; n_regions must equal the handle's.  An
 * empty motif or a byte other than ACGT (either case) is NRA_E_ARG, a motif over 64 bases NRA_E_RANGE.  Builds the
 * class table on the host and keeps it on the device: 5460 uint16 entries (class + 1, or 0) at off[p] + code(p-mer),
 * off[p] = 4 + ... + 4^(p-1), every rotation of every class root and of its reverse complement filled in.  A second
 * call replaces the first. */
int nra_screen_set_motifs(nra_screen_t* s, int32_t n_regions, const char* motifs, const int64_t* motif_off);
/* nra_screen_reads with the four kinds above; min_hits >= 1, motif_share_pct in 1..100 (else NRA_E_ARG).  The capacity
 * protocol is nra_screen_reads': *n_pairs is the capacity of the six arrays on entry and the number of pairs on return;
 * too small a capacity writes nothing, leaves the number needed in *n_pairs and returns NRA_E_RANGE.  Without motifs
 * set no pair is of kind 3.  One upload of the reads serves the anchor and the motif kernel. */
int nra_screen_reads_partial(nra_screen_t* s, int32_t n_reads, const char* seqs, const int64_t* seq_off,
                             int32_t min_hits, int32_t motif_share_pct, int64_t* n_pairs,
                             int32_t* pair_read, int32_t* pair_region, int32_t* hits_left, int32_t* hits_right,
                             int32_t* motif_windows, uint8_t* kind);

/* ---- repeat structure: what a read's tract is made of (no counterpart in the reference) ---------------------------
 *
 * Each read's tract s (n bases, upper-cased first; a byte other than ACGT mismatches every motif base) is aligned
 * globally in s against its motif u (p bases, 1 <= p <= 64, uppercase ACGT) repeated without end, starting and ending
 * at any phase (phase j = motif bases consumed mod p).  Unit costs:
 *   D[0][j] = 0;  for i >= 1, c = s[i-1]:
 *   T[j]    = min(D[i-1][(j-1) mod p] + (c != u[(j-1) mod p])   diagonal, consumes u[(j-1) mod p]
 *                 D[i-1][j] + 1)                                insertion; a tie takes the diagonal
 *   D[i][j] = min(T[j], D[i][(j-1) mod p] + 1)                  deletion, cyclic until stable; a tie keeps T
 *   edits = min_j D[n][j]; the end phase is the smallest j that attains it.
 * Traceback from (n, end phase): a deletion stays in row i and moves to phase j-1, an insertion to (i-1, j), a diagonal
 * step to (i-1, j-1); start_phase = the phase where it reaches row 0.  One path byte per tract base: bits 0-1 the
 * base's op (0 match, 1 mismatch, 2 insertion), bits 2-7 the motif bases deleted right after it (0..p-1).
 * DESIGN.md section 14. */

/* motif m = bytes [motif_off[m], motif_off[m+1]) of `motifs` (n_motifs >= 1); read r = bytes [seq_off[r],
 * seq_off[r+1]) of `seqs` (at most 200 000, NRA_E_RANGE beyond), aligned against motif read_motif[r].  Writes
 * edits[r], start_phase[r] and the path bytes of read r at path[seq_off[r] ...] (path: seq_off[n_reads] bytes).
 * A motif of 0 bases or with a byte other than A, C, G, T is NRA_E_ARG, one of more than 64 bases NRA_E_RANGE;
 * arguments are checked before the device is touched. */
int nra_read_structure(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off,
                       int32_t n_reads, const char* seqs, const int64_t* seq_off, const int32_t* read_motif,
                       int32_t* edits, int32_t* start_phase, uint8_t* path);

/* ---- tandem motifs: which motifs a read's tract is made of (no counterpart in the reference) ----------------------
 *
 * For each tract s (n bases, upper-cased first) and each period p = 1..max_period, position i (i + 2p <= n) is a
 * tandem position when s[i, i+p) == s[i+p, i+2p), all 2p bases are A, C, G or T (any other byte breaks the window)
 * and the word w = s[i, i+p) is primitive (not x^m for a shorter x: AA never counts at p = 2, ATAT never at p = 4).
 * The class of w is its smallest rotation in the order A < C < G < T; its code is that rotation in base 4, first base
 * most significant.  There are 964 classes of 1..6 bases.  DESIGN.md section 15. */

/* tract t = bytes [seq_off[t], seq_off[t+1]) of `seqs` (at most 200 000 bases, NRA_E_RANGE beyond).  Writes
 * n_tandem[t * max_period + p - 1] = the tandem positions of period p, and the top_n classes by count as
 * (top_p, top_code, top_count)[t * top_n + q], ordered by count descending, then p ascending, then code ascending;
 * (0, -1, 0) in unused slots.  1 <= max_period <= 6 and 1 <= top_n <= 8, else NRA_E_ARG; arguments are checked
 * before the device is touched. */
int nra_tract_motifs(int device, int32_t n_tracts, const char* seqs, const int64_t* seq_off, int32_t max_period,
                     int32_t top_n, int32_t* n_tandem, int8_t* top_p, int32_t* top_code, int32_t* top_count);

/* ---- tandem periods: the lag-match spectrum of a tract for lags up to 64 (no counterpart in the reference) ---------
 *
 * For each tract s (n bases, upper-cased first) and each lag p = 1..max_period:
 *   valid[p] = #{ i : 0 <= i, i + p < n, s[i] and s[i+p] both A, C, G or T }
 *   match[p] = #{ those i with s[i] == s[i+p] }
 * Where n <= p both are 0.  match[p] / valid[p] is the share of the tract that repeats at distance p: near 1 at the
 * period of a tandem repeat and at its multiples, near 1/4 for sequence without a period.  The outputs are integers:
 * the result of a tract does not depend on the other tracts of the call or on their order.  DESIGN.md section 22. */

/* tract t = bytes [seq_off[t], seq_off[t+1]) of `seqs` (at most 200 000 bases, NRA_E_RANGE beyond; empty tracts and
 * n_tracts = 0 are fine).  Writes match[t * max_period + p - 1] and valid[t * max_period + p - 1] for p = 1..max_period.
 * 1 <= max_period <= 64, else NRA_E_ARG; arguments are checked before the device is touched. */
int nra_tract_periods(int device, int32_t n_tracts, const char* seqs, const int64_t* seq_off, int32_t max_period,
                      int32_t* match, int32_t* valid);

/* ---- anchored extension: how many repeat units a tract shows from one anchored end (no counterpart in the reference)
 *
 * For a read with one anchor only: the sequence s that follows the anchor (n bases, upper-cased first; a byte other
 * than ACGT mismatches every motif base) is extended along its motif u (p bases, 1 <= p <= 64, uppercase ACGT) repeated
 * without end, anchored at its first base, free at its far end.  Scores match = a, mismatch = b, gap = g
 * (1 <= a <= 127, 0 <= b <= 127, 1 <= g <= 127).  Each cell holds a score H and a count M of motif bases consumed;
 * phase j = motif bases consumed mod p.
 *   H[0][j] = 0, M[0][j] = 0                        anchored at row 0, any start phase; no zero floor later
 *   for i >= 1, c = s[i-1], k = (j-1) mod p:
 *     diagonal  H[i-1][k] + (c == u[k] ? a : -b),   count M[i-1][k] + 1
 *     insertion H[i-1][j] - g,                      count M[i-1][j]
 *     T[j] = the larger; a tie takes the diagonal
 *     H[i][j] = max over d = 0..p-1 of T[(j-d) mod p] - g*d, count + d    (d motif bases deleted);
 *               among equal values the smallest d wins
 *   best = the largest H[i][j] over i >= 0; among equals the smallest i, then the smallest j.
 * Outputs per sequence: score = best H (0 with end = 0 when nothing is positive), end = that i, end_phase = that j,
 * motif_bases = that M.  motif_bases / p is the number of repeat units the sequence shows next to its anchor: a lower
 * bound from one read, not an allele size.  DESIGN.md section 16. */

/* Motifs and reads as for nra_read_structure (read r: at most 200 000 bases, NRA_E_RANGE beyond; a motif of 0 bases
 * or with a byte other than A, C, G, T is NRA_E_ARG, one of more than 64 bases NRA_E_RANGE); a score outside its range
 * is NRA_E_ARG.  Writes score[r], end[r], end_phase[r], motif_bases[r].  Arguments are checked before the device is
 * touched. */
int nra_extend_tracts(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off,
                      int32_t n_reads, const char* seqs, const int64_t* seq_off, const int32_t* read_motif,
                      int32_t match, int32_t mismatch, int32_t gap,
                      int32_t* score, int32_t* end, int32_t* end_phase, int32_t* motif_bases);

/* ---- mixture fits: the diagonal Gaussian mixtures of the phasing step, many fits in one call
 *
 * One fit of n components to the N x d sample X (float64, d = 1 or 2) from n start rows, everything in float64:
 *   1. means = the start rows.  labels = nearest mean (squared distance summed over the axes; a tie goes to the lowest
 *      component).  Up to 10 Lloyd steps: the mean of a component with points becomes the mean of its points, one
 *      without keeps its mean, relabel; stop early when no label changes.
 *   2. responsibilities r = one-hot labels, then the M-step of a diagonal mixture:
 *      nk = sum r + 10 eps (eps = 2^-52), mu = sum r x / nk, var = sum r x^2 / nk - mu^2 + 1e-6, w = nk / N.
 *   3. E-step: log p(x, c) = log w_c - (d log 2 pi + sum log var_c) / 2 - sum (x - mu_c)^2 / var_c / 2 (sums over the
 *      axes), log p(x) by log-sum-exp over c, r = exp(log p(x, c) - log p(x)), lb = mean of log p(x) over the points;
 *      then the M-step on r.  Stop after the M-step of the first E-step whose |lb - lb of the E-step before| < 1e-3
 *      (converged = 1), or after 100 E-steps (converged = 0).
 * Outputs per fit: lb of its last E-step, n_iter = E-steps, converged, and w, mu, var of its last M-step.  A fit is
 * a function of its sample and its start rows alone: not of the other fits of the call, their order, or the run.
 * DESIGN.md section 17. */

/* flags of nra_mixture_fit, for tests and comparisons: the results do not depend on them */
#define NRA_MIX_STREAM     1   /* every problem streams its points from memory, also one that fits in registers */
#define NRA_MIX_ONE_CLASS  2   /* no separate kernel for problems of up to 1024 points */

/* Problem p = prob_n[p] rows of prob_d[p] doubles from samples[prob_off[p]] (of n_samples doubles in all; problems may
 * share rows).  Fit f = fit_n[f] components on problem fit_problem[f]; its start rows are the next fit_n[f] entries of
 * `starts`, fits in order.  Writes lb[f], n_iter[f], converged[f], and with o = fit_n[0] + ... + fit_n[f-1]:
 * w[o + c], mu[2 (o + c) + axis], var[2 (o + c) + axis] (axis 1 is 0 where d = 1).  d other than 1 or 2, a problem
 * without points or outside the samples, a value that is not finite, n < 1, n > N or a start row >= N is NRA_E_ARG;
 * n > 32 or N > 4 194 304 is NRA_E_RANGE.  Arguments are checked before the device is touched. */
int nra_mixture_fit(int device, int64_t n_samples, const double* samples, int32_t n_problems, const int64_t* prob_off,
                    const int32_t* prob_n, const int32_t* prob_d, int32_t n_fits, const int32_t* fit_problem,
                    const int32_t* fit_n, const int32_t* starts, int32_t flags,
                    double* lb, double* w, double* mu, double* var, int32_t* n_iter, int32_t* converged);

/* ---- bootstrap of the mixture fits: the order search of every replicate of every problem in one call
 *
 * A problem is what the phasing step fits: m kept reads of d axes (x, row-major), an error rate e, the noise z of its
 * simulated sample (100 m d doubles) and the start rows of its fits.  Replicate b of it resamples the reads by
 * idx[b][0..m) and keeps the noise in place.  Row j (0 <= j < N = 100 m), axis a of its sample:
 *   X_b[j][a] = x[idx[b][j mod m]][a] + (z[j d + a] e) (10 + x[idx[b][j mod m]][a])
 * evaluated in this order in float64 with nothing contracted (idx[b] = 0, 1, ..., m - 1 gives the problem's own sample).
 * Order search of a replicate, every fit as specified for nra_mixture_fit:
 *   for n = first_n, first_n + 1, ...:
 *     n > max_n: decided, order max_n with the model made for it.
 *     n > n_cap: NRA_BOOT_NEEDS_MORE (the caller runs the problem again with a larger n_cap).
 *     n = 1: nothing to fit and no pair to overlap; go on.
 *     fit n components from each of the ten starts of order n; the best is the largest lb, a tie to the lowest start.
 *     if two components i < j of the best have intervals mu +- z_o max(1, sqrt(var)) that overlap on every axis
 *     (max of the lower ends - min of the upper ends <= 0: touching counts): decided, order n - 1 with the best model
 *     of order n - 1.
 * Order 1 has no parameters: every read belongs to its one component.
 * Outputs per replicate: status, and when decided the order, the best start of that order (-1 for order 1), its lb
 * (0 for order 1) and w, mu, var of its components.  A replicate is a function of its problem and its indices alone:
 * not of the other replicates or problems of the call, their order, the flags or the run.  DESIGN.md section 24. */
#define NRA_BOOT_DECIDED     0
#define NRA_BOOT_NEEDS_MORE  1

/* Problem p: prob_m[p] reads of prob_d[p] axes from x[prob_x_off[p]] (of n_x doubles), noise from z[prob_z_off[p]]
 * (of n_z), error rate prob_e[p], interval factor prob_zo[p], orders prob_first_n[p] .. prob_n_cap[p] <= prob_max_n[p];
 * its start rows from starts[prob_start_off[p]] (of n_starts): for every order n from max(first_n, 2) to n_cap, ten
 * starts of n rows each, order-major.  idx: n_rep * m indices per problem, problems in order, replicate-major.
 * Replicate b of problem p is r = p * n_rep + b; with o = n_rep * (n_cap[0] + ... + n_cap[p-1]) + b * n_cap[p] it writes
 * status[r], order[r], best_start[r], lb[r], w[o + c], mu[2 (o + c) + axis], var[2 (o + c) + axis] for c < order[r]
 * (axis 1 is 0 where d = 1; entries not written are 0).  flags: NRA_MIX_STREAM, NRA_MIX_ONE_CLASS, as for
 * nra_mixture_fit; the results do not depend on them.
 * n_rep < 1, an index or a start row out of range, a value that is not finite, d other than 1 or 2, m < 1, or orders
 * that are not first_n = 1 or 2, 1 <= n_cap <= max_n are NRA_E_ARG; n_rep > 1000, n_cap > 32 or N > 4 194 304 is NRA_E_RANGE.
 * Arguments are checked before the device is touched. */
int nra_mixture_bootstrap(int device, int64_t n_x, const double* x, int64_t n_z, const double* z, int32_t n_problems,
                          const int32_t* prob_m, const int32_t* prob_d, const int64_t* prob_x_off,
                          const int64_t* prob_z_off, const double* prob_e, const double* prob_zo,
                          const int32_t* prob_first_n, const int32_t* prob_n_cap, const int32_t* prob_max_n,
                          const int64_t* prob_start_off, int64_t n_starts, const int32_t* starts, int32_t n_rep,
                          const int32_t* idx, int32_t flags, int32_t* status, int32_t* order, int32_t* best_start,
                          double* lb, double* w, double* mu, double* var);

/* ---- censored allele fit: spanning reads and lower bounds in one mixture likelihood (no counterpart in the reference)
 *
 * A problem is N values in the log domain y = ln(10 + size), the first n_exact of them exact observations, the other
 * N - n_exact lower bounds (right-censored observations), and a known standard deviation tau.  A model (n, open) has n
 * closed components N(nu_k, tau^2) with weights w_k and, when open = 1, one open component with weight w_o: density 0
 * at every exact value and survival 1 at every bound (an allele no read spans).  Everything in float64, nothing
 * contracted into an fma.  With u = z sqrt(1/2):
 *   logS(z)   = log(0.5 erfc(u))             lambda(z) = sqrt(2/pi) exp(-u u) / erfc(u)      for u <= 0
 *   logS(z)   = log(0.5 erfcx(u)) - u u      lambda(z) = sqrt(2/pi) / erfcx(u)               for u >  0
 *   exact y:  log p(y, k) = (log w_k - log(2 pi tau^2) / 2) - (y - nu_k)^2 (1 / (2 tau^2)); the open component: none
 *   bound c:  log p(c, k) = log w_k + logS((c - nu_k) (1 / tau));  the open component: log w_o
 * One fit from the start means nu^0, with w = 1 / (n + open):
 *   E-step: log p(y) by log-sum-exp over the components (maximum, sum of exp in component order, the open one last),
 *   r = exp(log p(y, k) - log p(y)), lb = (sum of log p(y)) / N.
 *   M-step: nk = sum r + 10 eps (eps = 2^-52), w = nk / N for every component; for a closed one with sum r > 1e-12,
 *   nu_k = (sum over exact of r y + sum over bounds of r (nu_k + tau lambda(z))) / nk, else nu_k stays.
 *   Stop after the M-step of the first E-step with |lb - lb of the E-step before| < tol (converged = 1), or after
 *   max_iter E-steps (converged = 0).
 * Outputs per fit: ll = lb N of its last E-step, n_iter = E-steps, converged, and w, nu of its last M-step.  A fit is a
 * function of its problem and its start means alone: not of the other fits of the call, their order, the flags or the
 * run.  The posteriors of a model are the r of one E-step from its w and nu.  DESIGN.md section 26. */

#define NRA_CENS_F_STREAM        1   /* testing / comparison: every problem streams its values from memory */
#define NRA_CENS_MAX_COMPONENTS  8   /* closed components of a model */
#define NRA_CENS_MAX_N     1048576   /* values of a problem */
#define NRA_CENS_MAX_ITER      500   /* largest max_iter */

/* Problem p = prob_n[p] values from values[prob_off[p]] (of n_values in all), the first prob_n_exact[p] exact, with
 * tau = prob_tau[p].  Fit f = (fit_n[f] closed components, fit_open[f] in {0, 1}) on problem fit_problem[f]; its start
 * means are the next fit_n[f] entries of `starts`, fits in order.  Writes ll[f], n_iter[f], converged[f], nu[s + k] with
 * s = fit_n[0] + ... + fit_n[f-1], and w[s + f' + k] with f' = fit_open[0] + ... + fit_open[f-1] (the open weight last).
 * n outside 1..8, N > 1 048 576 or max_iter > 500 is NRA_E_RANGE; n_exact outside 1..N, a value, start or tau that is
 * not finite, tau <= 0, open other than 0 or 1, open = 1 on a problem without a bound, max_iter < 1, tol negative or
 * not finite, or an unknown flag is NRA_E_ARG.  Arguments are checked before the device is touched. */
int nra_censored_fit(int device, int64_t n_values, const double* values, int32_t n_problems, const int64_t* prob_off,
                     const int32_t* prob_n, const int32_t* prob_n_exact, const double* prob_tau, int32_t n_fits,
                     const int32_t* fit_problem, const int32_t* fit_n, const int32_t* fit_open, const double* starts,
                     int32_t max_iter, double tol, int32_t flags, double* ll, double* w, double* nu, int32_t* n_iter,
                     int32_t* converged);

/* Problems as above, one model each: (model_n[p], model_open[p]) with nu[s + k] and w[s + p' + k] laid out as the
 * outputs of nra_censored_fit with problem p in the place of fit f (weights > 0 and finite, else NRA_E_ARG).  Writes
 * the posteriors of value i of problem p at resp[R_p + i (n + open) + k], R_p = the entries of the problems before;
 * resp holds n_resp entries (fewer than needed: NRA_E_RANGE).  The other errors as for nra_censored_fit. */
int nra_censored_posteriors(int device, int64_t n_values, const double* values, int32_t n_problems,
                            const int64_t* prob_off, const int32_t* prob_n, const int32_t* prob_n_exact,
                            const double* prob_tau, const int32_t* model_n, const int32_t* model_open, const double* w,
                            const double* nu, int64_t n_resp, double* resp);

/* ---- bootstrap of the censored allele fit: the model search of every replicate of every problem in one call
 *
 * A bootstrap problem is a problem as above in sorted layout: its m = n_exact exact values ascending, then its
 * q = N - m bounds ascending.  Replicate b of it is the row idx[b][0..N) of indices into the problem's values,
 * ascending, so that its first m_b = #(idx[b][j] < m) positions are exact values in order and the others bounds in
 * order; position j holds value idx[b][j] of the problem (the row 0, 1, ..., N - 1 is the problem itself).
 * Model search of a replicate with m_b >= 1, every fit as specified for nra_censored_fit on the replicate's values:
 *   d_b = the number of distinct values among the exact positions; q_b = N - m_b.
 *   for n = 1 .. min(max_alleles, d_b), open = 0 and, when q_b > 0, open = 1:
 *     three starts, each n means taken from the replicate by position, with pos(k, n, L) = min(L - 1, floor((k + 0.5) /
 *     n * L)) evaluated in float64, the division and the product each rounded once:
 *       start 0: exact position pos(k, n, m_b) for k < n;
 *       start 1: value pos(k, n, N) of the merge of the two sorted runs for k < n;
 *       start 2: exact position pos(k, n - 1, m_b) for k < n - 1, then the larger of the runs' last values.
 *     the best start is the largest ll, a tie to the lowest start.
 *     BIC = -2 ll + (2 n + open - 1) lnN, the product taken first, nothing contracted; lnN is the caller's ln N.
 *   the model is the lowest BIC; within 1e-9 of it the fewest parameters 2 n + open win, then open = 0.
 * A replicate with m_b = 0 is not fitted: NRA_CENS_BOOT_NO_EXACT, n = 0, open = (q_b > 0).
 * A replicate is a function of its problem's values, its row, tau, lnN, max_alleles, max_iter and tol alone: not of
 * the other replicates or problems of the call, their order, the flags or the run.  DESIGN.md section 27. */
#define NRA_CENS_BOOT_FITTED    0
#define NRA_CENS_BOOT_NO_EXACT  1
#define NRA_CENS_BOOT_MAX_B  1000   /* largest n_rep */

/* Problems as for nra_censored_fit, each in sorted layout, with prob_ln_n[p] = ln N.  idx: n_rep * N indices per
 * problem, problems in order, replicate-major; rep_m[p * n_rep + b] = m_b.  Replicate b of problem p is r = p * n_rep + b
 * and writes status[r], model_n[r], model_open[r], best_start[r], n_iter[r], ll[r], bic[r], nu[8 r + k] for k < n and
 * w[9 r + k] for k < n + open (the open weight at k = n); entries not written are 0.  flags: NRA_CENS_F_STREAM; the
 * results do not depend on it.
 * n_rep < 1, an index outside 0 .. N - 1, a row that is not ascending, rep_m that disagrees with its row, a value, tau
 * or lnN that is not finite, tau <= 0, n_exact outside 1..N, values that are not ascending within a part, max_iter < 1,
 * tol negative or not finite, or an unknown flag is NRA_E_ARG; n_rep > 1000, max_alleles outside 1..8, N > 1 048 576,
 * max_iter > 500 or more than 2^31 - 1 replicates in all is NRA_E_RANGE.  Arguments are checked before the device is
 * touched. */
int nra_censored_bootstrap(int device, int64_t n_values, const double* values, int32_t n_problems,
                           const int64_t* prob_off, const int32_t* prob_n, const int32_t* prob_n_exact,
                           const double* prob_tau, const double* prob_ln_n, int32_t n_rep, const int32_t* idx,
                           const int32_t* rep_m, int32_t max_alleles, int32_t max_iter, double tol, int32_t flags,
                           int32_t* status, int32_t* model_n, int32_t* model_open, int32_t* best_start,
                           int32_t* n_iter, double* ll, double* bic, double* nu, double* w);

/* ---- allele consensus: one sequence per group of tracts (no counterpart in the reference) ----------------------------
 *
 * Integer arithmetic throughout: the outputs are a function of the group alone, bit for bit.
 * A group is a list of tracts (upper-cased; A C G T -> codes 0..3, any other byte -> code 4); empty tracts are dropped,
 * m tracts remain, in the order given.
 *   Backbone of round 0: sort the tracts by (length, position in the group), take element (m - 1) / 2 (integer
 *   division), remove its code-4 bases.
 *   Alignment of a tract s (n bases) to the backbone b (t bases), global, unit cost:
 *     D[0][j] = j, D[i][0] = i,
 *     D[i][j] = min(D[i-1][j-1] + (s[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)   (code 4 mismatches every base).
 *   Traceback from (n, t) to (0, 0): at each cell the diagonal if it attains D[i][j], else the insertion (i-1, j), else
 *   the deletion (i, j-1).  The path gives per backbone column j the tract base aligned to it or "deleted", and per
 *   slot j in [0, t] (before column j; slot t is after the last column) the run of inserted tract bases.
 *   Left out: a tract with D[n][t] > max_dist takes no part in that round's vote (it may vote in a later round).
 *   Vote of the m_v tracts that take part: col[j][c], c in {A, C, G, T, deleted} (a code-4 base aligned to the column
 *   abstains); ins[j][c], c in {A, C, G, T}: the first base, in tract order, of the tract's insertion run in slot j,
 *   if the run is not empty and that base is A, C, G or T.
 *   New backbone, slots and columns interleaved from the left: slot j emits argmax_c ins[j][c] (a tie: the smallest
 *   code) when 2 * sum_c ins[j][c] > m_v; column j emits the symbol with the most votes -- on a tie the backbone's own
 *   base if it is among the tied, else the smallest code, "deleted" last -- unless that symbol is "deleted".
 *   Rounds: repeat with the new backbone until a round returns the backbone unchanged (converged = 1) or max_rounds
 *   rounds have run.  A round with m_v = 0 ends the group with the backbone it has, converged = 0 (the round counts).
 * Outputs per group: the consensus; n_rounds; converged; the tracts that voted in the last round and those left out
 * of it; per consensus base its support: the votes for the emitted symbol in the round that emitted it (the ins votes
 * for a base that entered through a slot; 0 everywhere when no round voted).  A group without tracts returns an empty
 * consensus and four zeros.
 * The device aligns inside a band of 64 c diagonals, c in {1, 2, 4, 8, 16}: with delta = t - n and
 * h = (64 c - 1 - |delta|) / 2 >= 0 the band holds the diagonals j - i in [min(0, delta) - h, max(0, delta) + h].  A
 * path from (0, 0) to (n, t) that leaves that range by x diagonals costs at least |delta| + 2 x, so every path of cost
 * <= w = |delta| + 2 h lies in the band: a banded distance <= w is the distance, and every traceback decision is the
 * full matrix's (a co-optimal predecessor lies on an optimal path, so in the band with its exact value; another one has
 * a banded value >= its true value and still fails the equality); a banded distance > w means the distance is > w.
 * A tract is aligned in a wider band until its banded distance is <= min(w, max_dist), or w >= max_dist says it is
 * left out.  max_dist <= 1000 (the widest band proves 1022).  DESIGN.md section 18. */

#define NRA_CONS_MAX_DIST     1000   /* largest (and default) max_dist */
#define NRA_CONS_MAX_ROUNDS   64
#define NRA_CONS_N_STATS      16     /* int64 counters: [c] alignments run and [5 + c] tract rows swept in band class c
                                        (c = 0..4: 64, 128, 256, 512, 1024 diagonals), [10] rounds launched, [11]
                                        alignment launches, [12] alignments repeated in a wider band, [13] tract-rounds
                                        left out by |t - n| > max_dist alone, [14] pointer bytes of the largest launch */

/* Group g = tracts [group_off[g], group_off[g+1]) (group_off[0] = 0, group_off[n_groups] = n_tracts); tract r = bytes
 * [seq_off[r], seq_off[r+1]) of `seqs` (at most 200 000 bases, NRA_E_RANGE beyond).  0 <= max_dist <= 1000 and
 * 1 <= max_rounds <= 64 (negative or zero: NRA_E_ARG, larger: NRA_E_RANGE).  Writes the consensus of group g as
 * letters at consensus[cons_off[g] .. cons_off[g+1]) and its supports at the same indices of `support` (both hold
 * cons_cap entries; NRA_E_RANGE when the consensuses need more), group_res[4 g ..] = n_rounds, converged, voted, left out, and stats[] if not
 * NULL.  Arguments are checked before the device is touched. */
int nra_tract_consensus(int device, int32_t n_groups, const int64_t* group_off, int32_t n_tracts, const char* seqs,
                        const int64_t* seq_off, int32_t max_dist, int32_t max_rounds, int64_t cons_cap,
                        char* consensus, int32_t* support, int64_t* cons_off, int32_t* group_res, int64_t* stats);

/* ---- allele split: two haplotypes of one size allele, told apart by tract sequence (no counterpart in the reference)
 *
 * Integer arithmetic throughout: the outputs are a function of the group and its backbone, bit for bit.  Every rule
 * counts and none looks at the order of the tracts: permuting the tracts of a group permutes the labels.
 * A group is a list of m tracts, coded as for the consensus (A C G T -> 0..3, any other byte -> 4; empty tracts stay),
 * and one backbone of t bases, all A, C, G or T (in practice the group's consensus).
 *   Step 1, pileup.  Each tract is aligned to the backbone by exactly the consensus alignment and traceback above (same
 *   band classes, same widening rule and proof).  A tract with D[n][t] <= max_dist gets a row: sym[j], per backbone
 *   column j, is the code 0..4 of the base aligned to it (4 abstains from every count) or 5, deleted.  Any other tract is
 *   left out: no row, label -1, distance -1.  m_v tracts have a row.  Insertion slots are not used by this version: in
 *   a tandem tract left-shifted insertion runs pile up at the run starts, and a column of them says little.
 *   Step 2, variant sites.  Per column, n[c] = the rows that show base c (c in A, C, G, T); a = the most voted base,
 *   b = the second (ties: the smaller code).  Column j is a site iff n[b] >= min_count and
 *   100 n[b] >= min_share_pct (n[a] + n[b]) and 2 (n[a] + n[b]) >= m_v.  Only substitution sites are called, deletion
 *   columns are not.  Sites are listed by ascending column; of more than max_sites those with the largest n[b] stay
 *   (ties: the smaller column), still listed by column.
 *   Step 3, two haplotypes.  The anchor is the site with the largest n[b] (ties: the smaller column).  Start labels: 0
 *   where the row shows a at the anchor, 1 where it shows b, else 2, undecided.  Up to max_iter times: per haplotype
 *   and site, its symbol is the most voted base among the rows with its label (ties: the smaller code; when none of them
 *   shows a base there, a of the site for haplotype 0 and b for 1); per row, its mismatches against either haplotype
 *   over the sites where it shows a base; fewer wins, a tie keeps the label (undecided included); all rows change
 *   together; stop after an iteration that changed no label.  Without a site every row has label 0 and no iteration runs.
 *   Step 4, verdict, on the symbols and counts of the final labels.  A site is supported when the two haplotype symbols
 *   differ and, in each haplotype, at least one row shows its symbol and 100 * (rows showing it) >= min_purity_pct *
 *   (rows showing a base there).  split = 1 iff both haplotypes have at least min_count rows and at least min_sites
 *   sites are supported.  Haplotype 0 is the one with more rows (a tie: the one that started as 0); labels, symbols and
 *   counts are swapped to make it so.
 * An empty backbone or a group without tracts has no sites and no split.  DESIGN.md section 19. */

#define NRA_SPLIT_MAX_SITES   4096
#define NRA_SPLIT_MAX_ITER    64
#define NRA_SPLIT_N_STATS     16     /* int64 counters as NRA_CONS_N_STATS, but [10] sites called and [15] groups split */

/* Groups and tracts as for nra_tract_consensus; backbone g = bytes [bb_off[g], bb_off[g+1]) of `backbones` (at most
 * 200 000 bases, NRA_E_RANGE beyond; a byte other than A, C, G, T in either case is NRA_E_ARG).  0 <= max_dist <= 1000;
 * min_count, min_sites >= 1; min_share_pct, min_purity_pct in 1..100; max_sites in 1..4096; max_iter in 1..64 (below:
 * NRA_E_ARG, above: NRA_E_RANGE).  Writes label[r] (-1, 0, 1, 2 undecided) and dist[r] per tract;
 * group_res[8 g ..] = split, rows in haplotype 0, in 1, undecided, tracts left out, n_sites, n_supported, iterations;
 * the sites of group g as records [site_off[g], site_off[g+1]) of `sites`, 12 ints each: column, symbol of haplotype 0,
 * of 1, the A C G T counts of haplotype 0, of 1, supported; and at site_sym[sym_off[g] + q m + i] what tract i of the
 * group shows at its site q (0..5, 6 without a row).  `sites` holds site_cap records and site_sym sym_cap bytes
 * (NRA_E_RANGE when they do not suffice: min(max_sites, t) sites per group always do); stats[] if not NULL.  Arguments
 * are checked before the device is touched. */
int nra_allele_split(int device, int32_t n_groups, const int64_t* group_off, int32_t n_tracts, const char* seqs,
                     const int64_t* seq_off, const char* backbones, const int64_t* bb_off, int32_t max_dist,
                     int32_t min_count, int32_t min_share_pct, int32_t min_purity_pct, int32_t min_sites,
                     int32_t max_sites, int32_t max_iter, int32_t* label, int32_t* dist, int32_t* group_res,
                     int64_t site_cap, int32_t* sites, int64_t* site_off, int64_t sym_cap, uint8_t* site_sym,
                     int64_t* sym_off, int64_t* stats);

/* ---- flank haplotypes: reads phased by the variants of the repeat's flanks (no counterpart in the reference)
 *
 * Integer arithmetic only: the outputs are a function of the group, bit for bit, and permuting the rows of a group
 * permutes the per-row outputs and changes nothing else.
 * Group: one per region.  Two backbone sides, bL (tL bases) and bR (tR bases), A C G T only, either may be empty, both
 * written from the repeat outward.  The group has tL + tR columns: column o of the left side is column o, column o of
 * the right side is column tL + o; o is the offset from the repeat.
 * Row: one per read, up to two segments sL and sR, coded as consensus tracts (A C G T -> 0..3, any other byte -> 4), also
 * written from the repeat outward.  An absent segment and an empty one are the same thing.
 *   Alignment of a segment s (n >= 1 bases) to its side b (t columns): the start is pinned, the end is free.  Unit cost,
 *   D[0][j] = j, D[i][0] = i and the recurrence of the consensus contract (code 4 mismatches every base).
 *   e = min over 0 <= j <= t of D[n][j], j* = the smallest j that attains it.  Traceback from (n, j*) to (0, 0) with the
 *   consensus priority: diagonal, insertion, deletion.  A column j < j* gets the code of the base aligned to it (0..4) or
 *   5, deleted; a column j >= j* gets 6, not covered; insertions leave no mark.  If e > max_dist the side is left out:
 *   every column 6, dist = -1, end = 0.  An absent side has dist = -2, end = 0 and every column 6.
 *   Band: classes c in {1, 2, 4, 8, 16}, h = 32 c - 1, the band holds the diagonals j - i in [-h, h] (the device adds
 *   h + 1, which changes nothing below).  A path from (0, 0) that leaves the band costs more than h, so every cell of row
 *   n with a true value <= h has that value in the band and every other cell a value > h: a banded e <= min(h, max_dist)
 *   is the true e with the true j*, and every traceback decision is the full matrix's (the argument of the consensus
 *   contract).  A side starts in the smallest class with h >= min(max_dist, n / 32 + 8) and is
 *   aligned in the next wider band until that holds or h >= max_dist says it is left out.  0 <= max_dist <= 500 (the
 *   widest band proves 511).
 *   Sites.  Per column, n[c] = the rows that show base c, cov = the rows whose code there is <= 5; a = the most voted
 *   base, b = the second (ties: the smaller code).  A column at side offset o is a site iff o >= skip and
 *   n[b] >= min_count and 100 n[b] >= min_share_pct (n[a] + n[b]) and 2 (n[a] + n[b]) >= cov.  Substitution sites only,
 *   listed by column; of more than max_sites those with the largest n[b] stay (ties: the smaller column).
 *   Haplotypes and verdict: steps 3 and 4 of the allele split above, word for word, over the rows with at least one
 *   aligned side ("shows a base" treats the codes 4, 5 and 6 alike).  A row without an aligned side has label -1 and
 *   takes part in nothing.  phased = 1 iff both haplotypes have min_count rows and min_sites sites are supported;
 *   haplotype 0 is the larger one.  DESIGN.md section 25. */

#define NRA_FLANK_MAX_DIST    500    /* largest max_dist of nra_flank_phase */

/* Group g = rows [group_off[g], group_off[g+1]); segment `side` (0 left, 1 right) of row r = bytes [seg_off[2 r + side],
 * seg_off[2 r + side + 1]) of `segs`; side `side` of group g = bytes [bb_off[2 g + side], bb_off[2 g + side + 1]) of
 * `backbones` (a side or a segment of more than 200 000 bases: NRA_E_RANGE; a backbone byte other than A, C, G, T in
 * either case: NRA_E_ARG).  0 <= max_dist <= 500, skip >= 0 (negative: NRA_E_ARG), the other thresholds as for
 * nra_allele_split (below range NRA_E_ARG, above NRA_E_RANGE).  Writes label[r] (-1, 0, 1, 2 undecided),
 * dist[2 r + side] and end[2 r + side] = j*; group_res[8 g ..] = phased, rows in haplotype 0, in 1, undecided, rows with
 * label -1, n_sites, n_supported, iterations; site records, site_sym ([site][row]), their offsets and capacities as for
 * nra_allele_split, the column of a record being the group column (tL and above: the right side); stats[] (16 counters
 * in the layout of NRA_SPLIT_N_STATS, per aligned side) if not NULL.  Arguments are checked before the device is
 * touched. */
int nra_flank_phase(int device, int32_t n_groups, const int64_t* group_off, int32_t n_rows, const char* segs,
                    const int64_t* seg_off, const char* backbones, const int64_t* bb_off, int32_t max_dist, int32_t skip,
                    int32_t min_count, int32_t min_share_pct, int32_t min_purity_pct, int32_t min_sites,
                    int32_t max_sites, int32_t max_iter, int32_t* label, int32_t* dist, int32_t* end,
                    int32_t* group_res, int64_t site_cap, int32_t* sites, int64_t* site_off, int64_t sym_cap,
                    uint8_t* site_sym, int64_t* sym_off, int64_t* stats);

/* ---- motif runs: which motifs a tract is made of, how many units of each, and where (no counterpart in the reference)
 *
 * A motif set is M motifs u_0 .. u_{M-1}, 1 <= M <= 8, each uppercase ACGT of p_m = 1..32 bases, with S = sum of p_m <=
 * 32 states.  State (m, j) means "in motif m, j = motif bases consumed mod p_m"; the states are ordered by (m, j).  A
 * tract s (n <= 200 000 bases, upper-cased first; a byte other than ACGT mismatches every motif base) is aligned
 * globally in s against the set, every motif repeated without end, starting and ending at any state; W is the price of
 * changing motif, 1 <= W <= 1000.  Unit costs otherwise:
 *   D[0][m,j] = 0 for every state;  for i >= 1, c = s[i-1]:
 *   T[m,j] = min(D[i-1][m,(j-1) mod p_m] + (c != u_m[(j-1) mod p_m])   diagonal, consumes u_m[(j-1) mod p_m]
 *                D[i-1][m,j] + 1)                                      insertion; a tie takes the diagonal
 *   A[m,j] = min(T[m,j], A[m,(j-1) mod p_m] + 1)                       deletion, cyclic inside motif m until stable; a
 *                                                                      tie keeps T
 *   b1 = the smallest A over all states, at the smallest state that attains it; b2 = the same over the states of every
 *        motif other than b1's (absent when M = 1)
 *   D[i][m,j] = min(A[m,j], (m is not b1's motif ? b1 : b2) + W)       switch; a tie keeps A
 *   edits = min D[n][.]; the end state is the smallest one that attains it.
 * No second deletion pass follows the switch: every state of a motif is offered the same b + W, so a cell that takes
 * the switch has a predecessor at b + W or less and gains nothing from a deletion, and a cell that keeps A has
 * A <= b + W already and A is closed under deletions.  D[i] is closed as it stands.
 * Traceback from (n, end state), in the priority diagonal, insertion, deletion, switch: a cell of row i that took the
 * switch continues at the A-layer of its source state (b1's or b2's) in the same row, so at most one switch happens
 * between two tract bases; a deletion stays in row i and moves to (m, j-1); an insertion goes to D[i-1][m,j], a
 * diagonal step to D[i-1][m,j-1].  start_motif and start_phase are the state in which the path reaches row 0 (0, 0 for
 * an empty tract).  Per tract base one path byte exactly as nra_read_structure writes it (bits 0-1 the op: 0 match, 1
 * mismatch, 2 insertion; bits 2-7 the motif bases deleted right after it), and one byte with the index, within the
 * set, of the motif that consumed or inserted the base.  With M = 1 the contract is that of nra_read_structure:
 * edits, start_phase and the path bytes are the same.  DESIGN.md section 20. */

/* set q = motifs [set_motif_off[q], set_motif_off[q+1]) of the motif list (n_sets >= 1); motif m = bytes [motif_off[m],
 * motif_off[m+1]) of `motifs`; tract t = bytes [seq_off[t], seq_off[t+1]) of `seqs`, aligned against set tract_set[t].
 * Writes edits[t], start_phase[t], start_motif[t], and the path bytes and motif bytes of tract t at path[seq_off[t] ...]
 * and motif_of[seq_off[t] ...] (seq_off[n_tracts] bytes each).  switch_cost <= 0, a set without motifs, a motif of 0
 * bases or with a byte other than A, C, G, T is NRA_E_ARG; a set of more than 8 motifs or more than 32 motif bases in
 * all, a tract of more than 200 000 bases or switch_cost > 1000 is NRA_E_RANGE.  Arguments are checked before the
 * device is touched. */
int nra_tract_segments(int device, int32_t n_sets, const int32_t* set_motif_off, const char* motifs,
                       const int64_t* motif_off, int32_t n_tracts, const char* seqs, const int64_t* seq_off,
                       const int32_t* tract_set, int32_t switch_cost, int32_t* edits, int32_t* start_phase,
                       int32_t* start_motif, uint8_t* path, uint8_t* motif_of);

/* ---- CpG methylation per read: the MM/ML calls of a read, counted over its tract and flanks (no counterpart in the
 * reference)
 *
 * All of it is integer arithmetic; the result of a read does not depend on the other reads of the call or their order.
 *
 * The sequenced strand.  A read has the stored bytes S[0..n) and the flag bits 0 (stored reversed: the record holds the
 * reverse complement of what was sequenced) and 1 (implicit: a C the list skips is unmodified).  The sequenced strand
 * is O: O[i] = S[i] without bit 0, O[i] = comp(S[n-1-i]) with it.  Case is ignored; every byte other than A, C, G, T
 * is "other" and is its own complement.
 *
 * Ranks.  n_c = the number of C in O.  The read's list is m deltas d_0 .. d_{m-1} (>= 0) and m call bytes; the listed
 * ranks are L_j = j + d_0 + ... + d_j, 0-based among the C of O (summed in 64 bits: they do not wrap).  If m > 0 and
 * L_{m-1} >= n_c, the read's status is NRA_METH_BAD_TAG and all its counters are 0; a read with m > n has that status
 * without being decoded.  Otherwise the status is NRA_METH_OK.
 *
 * Sites and calls.  A site is a stored index s, 0 <= s < n - 1, with S[s] = C and S[s+1] = G: the same set whichever
 * strand was sequenced.  Its C on the sequenced strand is O[s] without bit 0 and O[n-2-s] with it; r is that C's rank.
 * The site's call is probs[j] if r = L_j; byte 0 if r is not listed and bit 1 is set; none otherwise.
 *
 * Segments.  nb = ceil(flank / bin); a read has 2 nb + 1 segments, in this order: before[0..nb), tract, after[0..nb).
 * A site is in the tract when tract_lo <= s and s + 2 <= tract_hi; in before[(tract_lo - s - 2) / bin] when
 * s + 2 <= tract_lo and tract_lo - s - 2 < flank; in after[(s - tract_hi) / bin] when s >= tract_hi and
 * s - tract_hi < flank.  A site with one base on either side of a tract edge, or farther out than `flank`, is in no
 * segment.  Bin 0 is the one next to the repeat.  "Before" and "after" are in stored coordinates: which of them is the
 * reference's left side is the caller's business.
 *
 * Counters per segment, five int32 in this order: sites, called (sites with a call), meth (call >= hi_byte), unmeth
 * (call <= lo_byte), sum (of the call bytes).  DESIGN.md section 28. */
#define NRA_METH_OK        0
#define NRA_METH_BAD_TAG   1
#define NRA_METH_MAX_N     4000000   /* bases of a read: whole reads go in, not cores (the target limit of nra_align_pairs) */
#define NRA_METH_MAX_FLANK 100000
#define NRA_METH_MAX_BINS  64
#define NRA_METH_COUNTERS  5

/* read r = bytes [seq_off[r], seq_off[r+1]) of `seqs` (any case); its list = entries [mod_off[r], mod_off[r+1]) of
 * `deltas` and `probs`; flags[r] bits 0 and 1 as above (other bits: NRA_E_ARG); its tract = stored [tract_lo[r],
 * tract_hi[r]), 0 <= lo <= hi <= n.  Writes counts[(r * (2 nb + 1) + segment) * 5 + counter], n_c[r] and status[r].
 * A read of more than 4 000 000 bases, flank > 100 000 or more than 64 bins is NRA_E_RANGE; a negative delta, offsets
 * that decrease, a tract outside 0 <= lo <= hi <= n, a NULL array with n_reads > 0, flank or bin below 1, bin > flank,
 * or bytes outside 0 <= lo_byte < hi_byte <= 255 are NRA_E_ARG.  Arguments are checked before the device is touched;
 * n_reads = 0 writes nothing. */
int nra_read_methylation(int device, int32_t n_reads, const char* seqs, const int64_t* seq_off,
                         const int32_t* deltas, const uint8_t* probs, const int64_t* mod_off,
                         const uint8_t* flags, const int32_t* tract_lo, const int32_t* tract_hi,
                         int32_t flank, int32_t bin, int32_t lo_byte, int32_t hi_byte,
                         int32_t* counts, int32_t* n_c, int32_t* status);

/* ---- Repeat scan: the tandem runs of every read, with no region, anchor or motif given (no counterpart in the
 * reference)
 *
 * All of it is integer arithmetic; the result of a read does not depend on the other reads of the call or their order.
 *
 * Windows.  As for the screen: read r has len - k + 1 window positions (none when len < k); a window is valid when its
 * k bytes are all A, C, G, T in either case.
 *
 * Window class.  A valid window w has period q when w[i] == w[i + q] for every i < k - q, compared without regard to
 * case.  Its smallest period p in 1..6, if any, makes it a periodic window with the word w[0:p], upper-cased (a
 * smallest period is primitive).  Its canonical word is the smallest (A < C < G < T) among the p rotations of the word
 * and the p rotations of the word's reverse complement; its class id is (4^p - 4) / 3 + the canonical word read as a
 * base-4 number, first base most significant (0 .. 5459).  The window is forward when the canonical word is a rotation
 * of the word itself, else reverse; a class that is its own reverse complement (AT, ACGT) has forward windows only.
 *
 * Islands.  For read r and class C, the positions of C's windows in ascending order, cut wherever two neighbours differ
 * by more than max_gap; each piece is an island with start = its first position, end = its last position + k, windows =
 * its number of positions and fwd_windows = the forward ones among them.  The islands with end - start >= min_span are
 * the runs, ordered by (read, start, end, class).  Islands of different classes may overlap.  DESIGN.md section 29. */
#define NRA_SCAN_MAX_N   4000000   /* bases of a read */
#define NRA_SCAN_MAX_GAP 100000

typedef struct nra_scan_stats {
    int64_t n_windows;    /* valid windows */
    int64_t n_periodic;   /* periodic windows among them */
    int64_t n_segments;   /* what the kernel wrote: runs of consecutive windows of one class and orientation in a tile */
    int64_t n_chunks;     /* uploads */
    double kernel_ms;     /* k_scan_repeats, summed over the chunks (HIP events) */
} nra_scan_stats_t;

/* read r = bytes [seq_off[r], seq_off[r+1]) of `seqs`.  On entry *n_runs is the capacity of the six run arrays, on
 * return the number of runs; with too small a capacity nothing is written, *n_runs is the number needed and the call
 * returns NRA_E_RANGE.  `stats` may be NULL.  k outside 8..15, max_gap outside 1..100 000, min_span < k, a negative
 * count or capacity, offsets that decrease or a NULL array that is needed are NRA_E_ARG; a read of more than 4 000 000
 * bases is NRA_E_RANGE.  Arguments are checked before the device is touched.  Empty reads, reads shorter than k and
 * n_reads = 0 are fine. */
int nra_scan_repeats(int device, int32_t n_reads, const char* seqs, const int64_t* seq_off, int32_t k,
                     int32_t max_gap, int32_t min_span, int64_t* n_runs, int32_t* run_read, int32_t* run_start,
                     int32_t* run_end, int32_t* run_class, int32_t* run_windows, int32_t* run_fwd_windows,
                     nra_scan_stats_t* stats);

/* ---- Sketch pairs: which sequences of a group share k-mers (no counterpart in the reference)
 *
 * All of it is integer arithmetic; the result depends on neither the order of the sequences nor the other groups.
 *
 * Windows, valid windows and canon are the anchor screen's: a k-window (k odd, 11..15) is valid when all its bytes are
 * ACGTacgt, canon(w) = min(code(w), code(revcomp(w))), 2 bits per base, first base most significant.  A valid window is
 * periodic when w[i] == w[i+q] for all i < k - q and some q in 1..6, case ignored.  The sketch of a sequence is the set
 * of the distinct canon(w) over its valid windows that are not periodic; a sequence shorter than k or without such a
 * window has an empty sketch.  For a < b with group[a] == group[b] >= 0, shared(a, b) = |sketch(a) & sketch(b)|; the
 * result is every such pair with shared >= min_shared, ordered by (a, b).  A negative group id pairs with nobody; group
 * ids need not be contiguous or sorted.  DESIGN.md section 30. */
#define NRA_SKETCH_MAX_N     2048    /* bases of a sequence */
#define NRA_SKETCH_MAX_GROUP 65536   /* sequences of one group */

typedef struct nra_sketch_stats {
    int64_t n_windows;    /* valid windows */
    int64_t n_kmers;      /* the sum of the sketch sizes */
    int64_t n_compared;   /* pairs (a, b) compared: n (n - 1) / 2 summed over the groups */
    int64_t n_tiles;      /* workgroups of k_sketch_pairs: a sequence against up to 64 later ones of its group */
    double kernel_ms;     /* sketch_ms + pairs_ms (HIP events) */
    double sketch_ms;     /* k_sketch */
    double pairs_ms;      /* k_sketch_pairs, both runs when the pair list had to grow */
    double upload_ms;     /* host: offsets, allocations and the copies to the device (wall clock) */
    double sort_ms;       /* host: the sort of the pairs (wall clock) */
} nra_sketch_stats_t;

/* sequence s = bytes [seq_off[s], seq_off[s+1]) of `seqs`.  On entry *n_pairs is the capacity of the three pair arrays,
 * on return the number of pairs; with too small a capacity nothing is written, *n_pairs is the number needed and the
 * call returns NRA_E_RANGE.  sketch_size (n_seqs values, may be NULL) receives every sequence's sketch size, stats may
 * be NULL.  k even or outside 11..15, min_shared < 1, a negative count or capacity, offsets that decrease or a NULL
 * array that is needed are NRA_E_ARG; a sequence of more than 2048 bases or a group of more than 65 536 sequences is
 * NRA_E_RANGE.  Arguments are checked before the device is touched.  n_seqs = 0 is fine. */
int nra_sketch_pairs(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, const int32_t* group,
                     int32_t k, int32_t min_shared, int64_t* n_pairs, int32_t* pair_a, int32_t* pair_b,
                     int32_t* pair_shared, int32_t* sketch_size, nra_sketch_stats_t* stats);

/* ---- Placement: where short query sequences (the flanks of discovered loci) lie on a target that is streamed past
 * them (seed and vote; no counterpart in the reference)
 *
 * All of it is integer arithmetic; the result depends on neither the order of the queries, nor the order or the cut of
 * the chunks, nor the other queries except through max_occ.
 *
 * Windows, valid windows, code, canon and periodic windows (periods 1..6) are the anchor screen's.  k is odd, 11..15, so
 * no window is its own reverse complement; a valid window w is forward when code(w) == canon(w).
 *
 * Postings.  Every valid window of query q at position j that is not periodic is a posting (q, j, f), f its forward
 * bit, under the key canon(w).  A key with more than max_occ postings over all queries (a k-mer twice in one query
 * counts twice) has none: it is not in the index.
 *
 * Target windows.  nra_place_scan gives bases [pos0, pos0 + n) of contig `contig`, a label >= 0 of the caller's
 * choice.  Every window that lies wholly inside the chunk is a target window (t, i, g): contig t, contig position i of
 * its first base, forward bit g.  The caller overlaps successive chunks of a contig by k - 1 bases so that every window
 * of the contig is given exactly once; A WINDOW GIVEN TWICE COUNTS TWICE.  occ(c) is the number of valid target windows
 * with canon c over all scans of the handle.
 *
 * Hits.  A target window (t, i, g) and a posting (q, j, f) of its canon make a hit on strand s = 0 when f == g, else 1,
 * with the start diagonal d = i - j for s = 0 and d = i + j + k - len(q) for s = 1: the contig position on which base 0
 * of the query (of its reverse complement for s = 1) falls; it may be negative.  A hit counts when
 * occ(canon) <= max_target_occ.
 *
 * Votes.  v(q, t, s, b) = the counting hits with floor(d / bin) in {b, b + 1}, floor towards minus infinity: the bins
 * overlap, so that a diagonal drifting over a bin edge is not split.  The result is every (q, t, s, b) with
 * v >= min_votes, ordered by (q, t, s, b).
 *
 * The handle keeps the target windows of every index key until the key has more than NRA_PLACE_OCC_CEILING of them;
 * max_target_occ above that ceiling is NRA_E_RANGE.  DESIGN.md section 31. */
#define NRA_PLACE_MAX_QUERY    2048      /* bases of a query */
#define NRA_PLACE_MAX_QUERIES  1048576
#define NRA_PLACE_MAX_POS      (1 << 30) /* pos0 + n of a chunk */
#define NRA_PLACE_OCC_CEILING  1024      /* the largest max_target_occ of nra_place_candidates */
#define NRA_PLACE_MAX_HITS     (1 << 26) /* target windows a handle keeps */

typedef struct nra_place nra_place_t;

typedef struct nra_place_stats {
    int64_t n_keys;            /* distinct canonical k-mers in the index */
    int64_t n_postings;        /* their postings */
    int64_t n_masked_periodic; /* distinct periodic k-mers of the queries, left out */
    int64_t n_masked_max_occ;  /* distinct k-mers with more than max_occ postings, left out */
    int64_t index_bytes;       /* device bytes of the table and the occurrence counters */
    int64_t target_bases;      /* the sum of n over the scans (the k - 1 overlaps counted each time) */
    int64_t n_target_windows;  /* valid target windows */
    int64_t n_hits_kept;       /* hits of the keys with occ <= NRA_PLACE_OCC_CEILING */
    int64_t n_keys_over;       /* keys with occ > max_target_occ of the last nra_place_candidates (0 before one) */
    int64_t n_chunks;          /* nra_place_scan calls that succeeded */
    int64_t tile_windows;      /* target windows per workgroup of k_place_hits */
    double  build_ms;          /* host time of the index build in nra_place_create */
    double  kernel_ms;         /* k_place_hits, summed over the scans (HIP events) */
    double  upload_ms;         /* host: the copies of the chunks to the device, summed (wall clock) */
    double  reduce_ms;         /* host: the last nra_place_candidates (wall clock) */
} nra_place_stats_t;

/* query q = bytes [seq_off[q], seq_off[q+1]) of `seqs`.  k even or outside 11..15, max_occ outside 1..255, a negative
 * count, offsets that decrease or a NULL array that is needed are NRA_E_ARG; more than 1 048 576 queries, a query of
 * more than 2048 bases or more than 2^26 postings are NRA_E_RANGE; all before the device is touched.  Empty queries,
 * queries shorter than k and n_queries = 0 are fine.  Builds the index on the host and keeps its table on the device. */
int nra_place_create(int device, int32_t n_queries, const char* seqs, const int64_t* seq_off, int32_t k,
                     int32_t max_occ, nra_place_t** out);
/* One chunk of one contig (above).  A negative contig, pos0 or n, or NULL bases with n > 0, are NRA_E_ARG;
 * pos0 + n > 2^30 is NRA_E_RANGE; both leave the handle as it was.  n = 0 and chunks shorter than k are fine.  When the
 * handle would keep more than NRA_PLACE_MAX_HITS target windows the call returns NRA_E_RANGE (lower max_occ: fewer
 * repeated k-mers stay in the index) and every later scan or candidates call on the handle returns NRA_E_STATE. */
int nra_place_scan(nra_place_t* h, int32_t contig, int64_t pos0, const char* bases, int64_t n);
/* The candidates of everything scanned so far.  bin in 1..4096, max_target_occ in 1..65535 (else NRA_E_ARG) and at most
 * NRA_PLACE_OCC_CEILING (else NRA_E_RANGE), min_votes >= 1.  On entry *n_cand is the capacity of the five arrays, on
 * return the number of candidates; with too small a capacity nothing is written, *n_cand is the number needed and the
 * call returns NRA_E_RANGE.  It changes nothing but the stats: it may be called again with other values, and more
 * chunks may be scanned after it. */
int nra_place_candidates(nra_place_t* h, int32_t bin, int32_t max_target_occ, int32_t min_votes, int64_t* n_cand,
                         int32_t* cand_query, int32_t* cand_contig, int32_t* cand_strand, int32_t* cand_bin,
                         int32_t* cand_votes);
int nra_place_stats(nra_place_t* h, nra_place_stats_t* st);
int nra_place_destroy(nra_place_t* h);

#ifdef __cplusplus
}
#endif
#endif /* NANOREPEAT_AMD_H */
