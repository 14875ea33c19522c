// nra_internal.h -- structures shared by the host side (nra_host.cpp) and the gfx950
// kernels (nra_kernels.hip).  Not part of the public ABI (include/nanorepeat_amd.h).
#ifndef NRA_INTERNAL_H
#define NRA_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime.h>

// Base codes.  Real bases 0..3, N = 4.  The two pad codes never compare equal to
// anything (including each other), so padded rows / columns only ever mismatch.
#define NRA_CODE_N    4
#define NRA_PAD_T     0x20   // target column outside [0, tlen)
#define NRA_PAD_Q     0x40   // query row >= qlen

// A candidate template is three consecutive pieces (1D: L+unit*k | - | R;
// 2D: L+unit1*k1 | mid+unit2*k2 | R).  Pieces 1 and 2 are stored pre-expanded to their
// largest k in the code pool, so a template is fully described by three lengths.
struct NraDevRegion {
    uint32_t p1_off;   // L + unit1 * k1max   (byte codes in the pool)
    uint32_t p2_off;   // mid + unit2 * k2max
    uint32_t p3_off;   // R
    uint32_t pr_off;   // rev(R) + rev(unit1) * k1max  (1D reverse sweep)
    int32_t  l1, m1;   // left_len, unit1_len
    int32_t  l2, m2;   // mid_len,  unit2_len (both 0 for 1D regions)
    int32_t  l3;       // right_len
};

struct NraDevRead {
    uint32_t qoff;     // first base of the read in the 2-bit pool (multiple of 16 bases)
    int32_t  qlen;
    int32_t  region;
    int32_t  rc;       // 1: the kernels read the reverse complement (2D '-' strand reads)
};

// Two candidates of one read scored by one wave (int16 halves A / B).
struct NraPairTask {
    int32_t read;
    int32_t k1a, k2a, k1b, k2b;
    int32_t out_a, out_b;  // index into the per-candidate score array; out_b < 0: no B half
    int32_t flags;         // bit 0: half B is the reverse complement of the template (strand probe);
                           // bit 1: store raw scores, no min_dp_score threshold
};

// Two reads of one region swept together (int16 halves A / B) by the junction-decomposition
// kernels; [kmin, kmax] is the union of their candidate windows.
struct NraSweepTask {
    int32_t read_a, read_b;   // read_b < 0: no second read
    int32_t kmin, kmax;
    uint64_t snap_off;        // the task's R-side snapshot (int32 index): 3 planes of R x 64 per row block
    int32_t read_c, read_d;   // k_sweep_ring32: the second pair of the wave (lanes 32..63); < 0: none
};

// R side of the junction as the half-wave kernel (k_sweep_ring32) keeps it: lane-major, [lane][H - o1 | E_in | E2_in][row],
// NRA_SNAP_LANE_STRIDE(R) dwords per lane (a multiple of 4: a lane stores its rows as 16-byte pieces, all in the one
// step it spends on the snapshot column, so every 64-byte sector it touches is complete when it leaves the wave; with
// the [row][lane] planes of the full-wave kernels two lanes per step add 4 bytes each to 128-byte lines that take 32
// steps to fill, and the half-wave kernel's WRITE_SIZE came to 2.6 x the bytes stored)
#define NRA_SNAP_LANE_STRIDE(R) ((3 * (R) + 3) / 4 * 4)

// One (task, row block) of the chained sweeps with concurrent blocks (k_sweep_ringmt): waves take these by ticket,
// in list order -- a producer (block b) precedes its consumer (block b + 1).
struct NraChainBlock {
    int32_t task;                  // index into the launch's sweep tasks
    int32_t blk, nblk;
    int32_t strip_in, strip_out;   // strips (5 planes of chain_cap 8-byte granules each) above / below the block; -1: none
};

// Tasks of the joint sweeps (nra_joint.hip).
//   tail sweep: one (read, k1) row of the 2D grid -- the read's cells with this k1 are
//     k2 = k2lo + n*k2step, n < n2, and sit at out + n in the cell arrays; `state` = where the
//     prefix sweep left the wave state for this (read, k1) (index into the int32 state buffer);
//   prefix sweep: one per read; its nk1 distinct k1 values, ascending, start at k1list[k1_off];
//     state of the i-th goes to state + i * (3R+7) * 64;
//   reverse sweep over R: one per read, only `read` is used.
//   resume != 0 (reverse and prefix sweeps): the first NRA_JOINT_PACKED_COLS columns were swept by k_joint_pk16;
//     the wave state it left is at pstate (index into the packed-state buffer), this read in half `phalf`.
//   Junction at the end of `mid` (routed grids, round 3 of the build): the reverse sweep runs on over rev(u2)^k2hi
//     and leaves, at the column of every k2 = k2lo + n*k2step, n < n2, its rows' column state in slot n of `state`
//     (3 planes of 64 * R int32: the wave's rows, padding included) and A(k2) at out + n; a MID sweep (one per (read, k1)) resumes like a tail, sweeps
//     the last prefix column + mid, and leaves its rows' column state at `pstate` and B(k1) at `out`.
//   k_joint_midscan: the column state of repeat count k1 is slot (k1 - task.k1) / task.k2step of `state` (the prefix
//     sweep may have left more of them than this grid asks for: kept column states).
struct NraJointTask {
    int32_t read;
    int32_t k1;
    int32_t k2lo, k2step, n2;
    int32_t out;
    int32_t k1_off, nk1;
    uint64_t state;
    uint64_t pstate;
    int32_t phalf, resume;
};

// One read's share of a routed grid (nra_batch2d_set_grid): its cells are the product of n1 values of k1 from k1lo in
// steps of the grid's step1 and n2 values of k2 from k2lo in steps of step2, k1-major.
struct NraGridRow { int32_t k1lo, n1, k2lo, n2; };

// One read of a routed grid for k_joint_combine: its n1 x n2 cells (k1-major at `out`) from the column states the
// MID sweeps (fs: n1 slots of 3 x qlen) and the extended reverse sweep (rs: n2 slots) left, B(k1) at fb, A(k2) at ra.
// The R side's slots may hold more k2 values than the grid asks for (kept column states): the grid's n-th k2 is slot
// rs_first + n * rs_stride of `rs` and of `ra`.
struct NraJointCombineTask {
    int32_t read, n1, n2, out;
    int32_t fb, ra, rs_first, rs_stride;
    uint64_t fs, rs;
    int32_t rs_plane, pad0;                     // rows of a plane of `rs`: 64 * (rows per lane of the read's bucket)
};

// Two reads of one rows-per-lane bucket whose payload-free columns -- L up to the scoring window, or rev(R) up to
// it -- are swept together in packed int16 cells (k_joint_pk16); the wave state goes to `state` (index into the
// packed-state buffer): NRA_JOINT_NPSTATE(R) planes of 64 dwords, both reads in the halves of every dword.
struct NraJointPairTask {
    int32_t read_a, read_b;   // read_b < 0: no second read
    uint64_t state;
};
#define NRA_JOINT_NPSTATE(R) (3 * (R) + 4)     // Hq, E_in, E2_in per row; diagonal, F, F2, running maximum
// columns without window payload at the start of a joint sweep: the window takes the last 10 bases of L
// (forward, dir 1) and the first 10 of R (the reverse sweep reads R backwards, dir 0)
#define NRA_JOINT_PACKED_COLS(flank) ((flank) > 10 ? (flank) - 10 : 0)
#define NRA_JOINT_PACKED_MIN_COLS 64           // shorter stretches stay in the int32 sweep

// One (query, target) pair whose path is wanted (nra_trace.hip).
struct NraTraceTask {
    int32_t read;        // query (2-bit pool)
    int32_t region;      // target = piece 1 of this region
    int32_t ops_cap;     // qlen + tlen
    int32_t blk0;        // k_trace_fill_mt: the slot of the pair's first row block in the best-cell records
    uint64_t trace_off;  // qlen * tlen bytes, row-major
    uint64_t ops_off;
};

// One (pair, row block) of the trace fill in row blocks (k_trace_fill_mt): waves take these by ticket, in list
// order -- a producer (block b) precedes its consumer (block b + 1).  A strip is 3 planes (6 in 64-bit cells) of
// the pair's columns, rounded up to 64, in 8-byte granules; strip_in / strip_out are granule offsets.
struct NraTraceBlock {
    int32_t task;
    int32_t blk, nblk;
    int32_t pad;
    uint64_t strip_in, strip_out;
};
#define NRA_TRACE_CHAIN_R NRA_CHAIN_R          // rows per lane of a row block: the height the chained payload sweeps use
// the rows per lane k_trace_fill_mt is built for: NRA_TRACE_CHAIN_R, and the smaller ones the tests may ask for
// (NRA_TEST_TRACE_BLOCK_ROWS = 64 * one of these).  48 rows per lane of 64-bit cells would spill.
#define NRA_TRACE_MT_R_LIST(X) X(1) X(2) X(3) X(4) X(6) X(8) X(12) X(16) X(24)

// One candidate scored with a payload (extents / window kernels).
struct NraTask {
    int32_t read;
    int32_t k1, k2;
    int32_t out;
};

struct NraScoreParams {
    int32_t match, mismatch;       // +a, b (penalty)
    int32_t open1, ext1;           // q+e, e   (cost of a gap's first base / each further base)
    int32_t open2, ext2;           // q2+e2, e2
    int32_t ambi;                  // N penalty
    int32_t min_score;
};

// What every sequence kernel reads (1D and joint sweeps, payload and score kernels, trace fills): the reads and regions
// of the batch, the code pool, the 2-bit query pool with its N mask, and the scores.  Passed by value to the launchers
// (every nra_launch_* below that scores sequences takes one); a launch that needs another field copies the struct and
// replaces that field.  Most kernels keep parameters of their own, filled from these fields (nra_device.h).
struct NraSeqArgs {
    const NraDevRead* reads;
    const NraDevRegion* regions;
    const uint8_t* pool;
    const uint32_t* q2bit;
    const uint32_t* qnmask;
    NraScoreParams sp;
};

// ... and what every 1D sweep adds: per read its candidate window [kmin, kmax] and the offset of its candidates (coff);
// the R-side snapshots and A (read_a) that the reverse sweeps write and the forward sweeps read; the candidates' scores
// and flank verdicts that the forward sweeps write (a reverse launcher nulls these two in its copy).  What differs from
// launch to launch -- tasks and their number, relax_c, redo, the quanta words, strips, epochs, give-up words -- stays a
// parameter of its own.
struct NraSweepArgs {
    NraSeqArgs seq;
    const int32_t* kmin;
    const int32_t* kmax;
    const uint32_t* coff;
    int32_t* snap;
    int32_t* read_a;
    int32_t* cand_score;
    uint8_t* cand_flag;
};

// rows-per-lane instantiations (a read of qlen rows uses the smallest R with 64*R >= qlen)
#ifndef NRA_R_LIST
#define NRA_R_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) \
                      X(15) X(16) X(18) X(20) X(22) X(24) X(28) X(32) X(40) X(48)
#endif
#define NRA_MAX_R 48
#define NRA_MAX_QLEN_1BLOCK (64 * NRA_MAX_R)   // rows one wave holds in registers
// longer reads are swept in row blocks of 64*NRA_CHAIN_R rows chained through a scratch strip, one read
// per wave in int32 cells (1D sweeps) or int32 / int64 payload cells (extents, windows, free pairs)
#define NRA_CHAIN_R 24
#define NRA_CHAIN_R_TEST 2                     // tiny row blocks, for the tests (NRA_F_TEST_CHAIN)
#define NRA_CHAIN_STRIPS 512                   // waves of a chained launch = scratch strips, at most (the host sizes them by
                                               // the tasks there are and by NRA_CHAIN_SCRATCH_BUDGET)
#define NRA_CHAIN_SCRATCH_BUDGET (3ull << 30)  // bytes of scratch strips per buffer: a wider template gets fewer waves
#define NRA_MAX_QLEN 200000                    // read bases (chained row blocks above NRA_MAX_QLEN_1BLOCK)
// int32 values per lane in one dumped wave state of the 2D prefix sweep (3 per row + 7), shared by
// the kernel and the host so that the two cannot disagree
#define NRA_JOINT_NSTATE(R) (3 * (R) + 7)
// a COLUMN state of the prefix sweep (DIR 5, for k_joint_midscan) lives in the same slot, lane-major: per lane
// [Hq | E_in | E2_in | Hup_prev, M] padded to 16-byte pieces (<= 3R + 5 < NSTATE dwords)
#define NRA_JOINT_COLSTATE(R) ((3 * (R) + 2 + 3) / 4 * 4)
// wave states of one group of 2D prefix sweeps: at most this many int32 (16 GiB)
#define NRA_JOINT_STATE_CAP_INTS (4ull << 30)
#define NRA_JOINT_KEEP_BUDGET (96ull << 30)    // bytes of column states kept from one routed grid for the next (else: not kept): a third of the
                                               // device, and never more than half of what is free.  Kept states pay at every size measured (config 3's
                                               // reads x 12 / x 16: 33 / 45 GiB kept, 76.6 -> 64.0 / 101.8 -> 88.1 ms per run); the loss round 3 saw
                                               // at 32 GB was the runtime pinning pageable task arrays of >= 1 MB under running kernels (copy_h2d)
#define NRA_MAX_TLEN 65000     // int32 payload cells: tstart is 16 bits; + 64 pipeline columns
#define NRA_MAX_TLEN_WIDE 4000000   // int64 payload cells (score << 32 | payload)
// rows per lane of the int64 payload kernels' unchained instantiations (a rare path: three sizes suffice)
#define NRA_WIDE_R_SMALL 16
#define NRA_WIDE_R_LARGE 48

// Anchor k-mer screen (nra_screen.hip, nra_screen_host.cpp).  The index is an open-addressing table of 8-byte slots: the
// canonical k-mer in bits 0..29, its number of postings in bits 30..37 and the first of them in bits 38..63; a posting
// is region * 2 + side.  An empty slot is all ones (no canonical k-mer has all 30 key bits set: its reverse complement
// would be smaller).
#define NRA_SCREEN_TILE 4096                  // window positions per workgroup
#define NRA_SCREEN_THREADS 256
#define NRA_SCREEN_MAP 128                    // (region, side) counters per workgroup in LDS; more overflow to global entries
#define NRA_SCREEN_EMPTY (~0ull)
#define NRA_SCREEN_KEY_BITS 30
#define NRA_SCREEN_CNT_BITS 8
#define NRA_SCREEN_START_BITS 26
#define NRA_SCREEN_HASH_MUL 0x9E3779B97F4A7C15ull

// one tile: n_win window positions of one read, the first at byte `base` of the chunk's device copy
struct NraScreenTile {
    int64_t base;
    int32_t read;
    int32_t n_win;
};

// hits of one tile on one (region, side) set; a (read, set) pair may have several entries (tiles, overflow)
struct NraScreenEntry {
    int32_t read, set, count;
};

// Motif screen (nra_screen_motifs.hip): the class table is indexed directly with NRA_MOTIF_TAB_OFF(p) + code(p-mer) for
// p = 1..NRA_MOTIF_MAX_ROOT; an entry is class + 1, or 0.  Its entries are NraScreenEntry with the class in `set`.
#define NRA_MOTIF_MAX_ROOT 6
#define NRA_MOTIF_TAB_OFF(p) (((1u << (2 * (p))) - 4u) / 3u)           // 4 + 16 + ... + 4^(p-1)
#define NRA_MOTIF_TAB_ENTRIES (NRA_MOTIF_TAB_OFF(NRA_MOTIF_MAX_ROOT) + (1u << (2 * NRA_MOTIF_MAX_ROOT)))   // 5460
#define NRA_MOTIF_MAX_LEN 64

// Repeat scan (nra_scan.hip, nra_scan_host.cpp): the tiles of the screen with the position of a
// tile's first window in its read; the table has the layout above, filled for every primitive p-mer with
// (class id + 1) << 1 | reverse.
struct NraScanTile {
    int64_t base;
    int32_t read;
    int32_t n_win;
    int32_t pos;
    int32_t pad;
};

// `len` consecutive windows of one table entry, the first at window position `start` of `read`, all inside one tile
struct NraScanSegment {
    int32_t read, start, len, entry;
};

// K-mer sketches and their pairs (nra_sketch.hip, nra_sketch_host.cpp).  A sequence has at most
// NRA_SKETCH_MAX_LEN bases, so its sketch fits the NRA_SKETCH_MAX_LEN sort slots of one workgroup and, in the pair
// kernel, fills the NRA_SKETCH_SET_SLOTS slots of the LDS set at most half.  A tile of the pair kernel is one sequence i
// against up to NRA_SKETCH_BLOCK later sequences of its group.
#define NRA_SKETCH_MAX_LEN 2048
#define NRA_SKETCH_THREADS 256
#define NRA_SKETCH_SET_SLOTS 4096
#define NRA_SKETCH_BLOCK 64
#define NRA_SKETCH_LAUNCH_TILES (1 << 23)        // tiles per launch: a grid of 2^32 threads or more runs only in part
#define NRA_SKETCH_EMPTY 0xffffffffu            // no k-mer: k <= 15, so a code has at most 30 bits

// one returned pair, original sequence indices, a < b
struct NraSketchPair {
    int32_t a, b, shared, pad;
};

// Placement (nra_place.hip, nra_place_host.cpp).  The index is the screen's table (key, number
// of postings, first posting; the postings stay on the host) with one 32-bit occurrence counter per slot.  A record is
// one target window whose canonical k-mer is a key: the slot, the contig and position << 1 | forward bit.
#define NRA_PLACE_TILE 4096                   // target windows per workgroup
#define NRA_PLACE_THREADS 256
#define NRA_PLACE_LAUNCH_WINDOWS (1 << 23)    // target windows per launch: the record list holds one record per window

struct NraPlaceRecord {
    uint32_t slot;
    int32_t contig;
    uint32_t pos_fwd;
};

// Repeat structure (nra_structure.hip, nra_structure_host.cpp): the wraparound edit-distance alignment of a read's tract
// against its motif repeated without end, one lane per read.  A launch takes reads of one phase
// capacity P (motif length p <= P), sorted by tract length, descending, 64 to a wave.
#define NRA_STRUCT_MAX_P 64
#define NRA_STRUCT_MAX_N 200000
#define NRA_STRUCT_BLOCK 16                   // tract bases per code load / path store / traceback block (16-byte aligned)
#define NRA_STRUCT_CODE_OTHER 4               // a tract byte other than ACGT (either case): mismatches every motif base

// eq[c] bit j: the motif base a diagonal step into phase j consumes, u[(j - 1) mod p], has code c (A=0 C=1 G=2 T=3)
struct NraStructMotif {
    uint64_t eq[4];
    int32_t p;
    int32_t pad;
};

// one read of a launch: its codes (and its path bytes) start at byte `tract` of the chunk's buffers (a multiple of
// NRA_STRUCT_BLOCK), its wave's traceback pointers at dword `ptr` ([row][lane] of the wave, the words of a row per lane)
struct NraStructRead {
    uint64_t tract;
    uint64_t ptr;
    int32_t n;
    int32_t motif;
};

// traceback pointer words per (row, lane): ins bits of the P phases, then del bits
#define NRA_STRUCT_WORDS(P) ((P) <= 16 ? 1 : (P) <= 32 ? 2 : 4)

// Motif runs (nra_segment.hip, nra_segment_host.cpp): the alignment of a tract against a set of motifs with a price for
// changing motif, one lane per tract.  A launch takes tracts of one state class SC in {8, 16, 32}
// (the set's states S <= SC), sorted by tract length, descending, 64 to a wave.  Codes, blocks and tract records are
// those of the repeat structure (NraStructRead.motif = the tract's set).
#define NRA_SEG_MAX_MOTIFS 8
#define NRA_SEG_MAX_STATES 32
#define NRA_SEG_MAX_SWITCH 1000

// a motif set as masks over its S states, state g = (motif m, phase j) in (m, j) order: eq[c] bit g: the motif base a
// diagonal step into g consumes, u_m[(j - 1) mod p_m], has code c; first / last bit g: g is the first / last state of
// its motif
struct NraSegSet {
    uint32_t eq[4];
    uint32_t first;
    uint32_t last;
    int32_t S;
    int32_t pad;
};

// traceback pointer words per (row, lane).  SC 8: ins | del << 8 | sw << 16 | s1 << 24 | s2 << 27; SC 16: (ins |
// del << 16, sw | s1 << 16 | s2 << 20); SC 32: (ins, del, sw, s1 | s2 << 8).  s1, s2: the states of b1 and b2
#define NRA_SEG_WORDS(SC) ((SC) <= 8 ? 1 : (SC) <= 16 ? 2 : 4)

// Tandem motifs (nra_motif.hip, nra_motif_host.cpp): per read tract, the tandem positions of each period 1..6 and
// the counts of their motif classes.  A class is a Lyndon word of p <= 6 bases; its code is the
// word in base 4, first base most significant; its dense id orders the 964 classes by (p, code).
#define NRA_MOTIF_MAX_P 6
#define NRA_MOTIF_MAX_TOP 8
#define NRA_MOTIF_MAX_N 200000
#define NRA_MOTIF_CODES 5460                  // sum of 4^p, p = 1..6: the code-to-dense-id table
#define NRA_MOTIF_CLASSES 964                 // Lyndon words of 1..6 bases over ACGT
#define NRA_MOTIF_BLOCK 16                    // positions per lane step; tracts start 16-byte aligned
#define NRA_MOTIF_CODE_OTHER 4                // a tract byte other than ACGT (either case): breaks every window
#define NRA_MOTIF_PAD 32                      // bytes after the last tract of a chunk: a block loads 32 bytes

// one tract of a launch: its codes start at byte `off` of the chunk's buffer (a multiple of NRA_MOTIF_BLOCK)
struct NraMotifTract {
    uint64_t off;
    int32_t n;
    int32_t pad;
};

// Tandem periods (nra_period.hip, nra_period_host.cpp): per tract and lag p = 1..64, the positions i with s[i] and
// s[i + p] both ACGT and those of them with s[i] == s[i + p].  One wave per tract, a lane per
// lag; codes as for the tandem motifs, tracts start 16-byte aligned and are read in words of 32 bases.
#define NRA_PERIOD_MAX_P 64
#define NRA_PERIOD_MAX_N 200000
#define NRA_PERIOD_WORD 32                    // bases per packed word: a lane loads 32 bytes
#define NRA_PERIOD_ALIGN 16                   // tracts start at multiples of it
#define NRA_PERIOD_PAD 32                     // bytes after the last tract of a chunk: a word may end beyond its tract
typedef NraMotifTract NraPeriodTract;         // (off, n): the tract's codes start at byte `off` of the chunk's buffer

// Mixture fits (nra_mixture.hip, nra_mixture_host.cpp): one workgroup of 256 threads per fit.
// A problem of up to 256 * KREG_SMALL or 256 * KREG points keeps its points in registers, a larger one streams them.
#define NRA_MIX_THREADS 256
#define NRA_MIX_MAX_COMPONENTS 32
#define NRA_MIX_MAX_N (1 << 22)
#define NRA_MIX_KREG_SMALL 4
#define NRA_MIX_KREG 20
#define NRA_MIX_LLOYD_STEPS 10
#define NRA_MIX_MAX_ITER 100
#define NRA_MIX_TOL 1e-3

// one problem: n rows of d doubles from double `off` of the sample buffer (even, so a row of two is 16-byte aligned)
struct NraMixProblem {
    uint64_t off;
    int32_t n;
    int32_t d;
};

// one fit: n components on `problem`; its start rows and its per-component results begin at entry `off`
struct NraMixFit {
    int64_t off;
    int32_t problem;
    int32_t n;
};

// Bootstrap of the mixture fits (nra_bootstrap.hip, nra_bootstrap_host.cpp): one workgroup of 256 threads runs the whole
// order search of one replicate of one problem.
#define NRA_BOOT_MAX_B 1000
#define NRA_BOOT_STARTS 10
#define NRA_BOOT_COPIES 100          // rows of the sample per kept read

// one problem: m kept reads of d axes from double `x_off` of the size buffer, their noise (100 m d doubles) from double
// `z_off` of the noise buffer, its replicates' indices (m per replicate) from entry `idx_off`, its start rows (orders
// max(first_n, 2) .. n_cap, ten starts each, n rows per start) from entry `start_off`, and the results of its
// replicate b at entry `rep_off + b` (status, order, best start, lb) and `comp_off + b n_cap` (w; mu and var at twice
// that)
struct NraBootProblem {
    int64_t x_off, z_off, idx_off, start_off, rep_off, comp_off;
    double e, z_o;
    int32_t m, d, first_n, n_cap, max_n, pad;
};

// Censored allele fit (nra_censored.hip, nra_censored_host.cpp): one wavefront per fit.  A problem
// of up to 64 * NRA_CENS_KREG values keeps them in registers, a larger one streams them.
#define NRA_CENS_KREG 8

// one fit, or one model of the posteriors: its problem's n_points values from double `off` of the value buffer (the
// first n_exact exact), tau, n closed components and `open`; its means (start and result) from entry `nu_off`, its
// n + open weights from entry `w_off`, its posteriors (k_censored_resp) from entry `resp_off`
struct NraCensFit {
    int64_t off, nu_off, w_off, resp_off;
    double tau;
    int32_t n_points, n_exact, n, open;
};

// Bootstrap of the censored fit (k_censored_boot, k_censored_pick).  One problem of a launch
// group: its n_points sorted values (the first n_exact exact) from double `off` of the value buffer, its replicates'
// index rows (n_points per replicate) from entry `idx_off`, tau and ln(n_points) as the host computed it
struct NraCensBootProblem {
    int64_t off, idx_off;
    double tau, ln_n;
    int32_t n_points, n_exact;
};

// what one wave leaves for (replicate, n, open): fitted = 0 when the replicate does not fit that model; else the best
// of the three starts.  Entries beyond n (nu) and n + open (w) are not written
struct NraCensBootRec {
    double ll;
    double w[9];             // NRA_CENS_MAX_COMPONENTS + 1: the open weight at n
    double nu[8];            // NRA_CENS_MAX_COMPONENTS
    int32_t fitted, start, n_iter, pad;
};

// Allele consensus (nra_consensus.hip, nra_consensus_host.cpp): banded unit-cost alignment of every tract of a group to
// the group's backbone, one wave per tract, votes into the group's tables, then a new backbone per group (DESIGN.md
// section 18).  Band class c: a lane owns c consecutive diagonals, the band holds 64 c.
#define NRA_CONS_MAX_N 200000
#define NRA_CONS_CLASSES 5                    // c = 1, 2, 4, 8, 16
#define NRA_CONS_CODE_OTHER 4                 // a tract byte other than ACGT: mismatches every base, abstains from votes
#define NRA_CONS_CODE_PAD 5                   // beyond the backbone
#define NRA_CONS_INF (1 << 28)
#define NRA_CONS_TAB 9                        // table ints per backbone position j: col[j][0..4], ins[j][0..3]
#define NRA_CONS_WIDEN (-1)                   // status: the band could not decide, align again in the next class
#define NRA_CONS_LEFT_OUT (-2)                // status: distance > max_dist

// one group of a round: backbone at byte `bb` of the backbone buffer (t bases), the new one (and its supports) from
// byte / entry `nb` of the new buffers (room for 2 t + 1), its tables at int `tab` ((t + 1) * NRA_CONS_TAB ints)
struct NraConsGroup {
    uint64_t bb;
    uint64_t nb;
    uint64_t tab;
    int32_t t;
    int32_t pad;
};

// one alignment of a launch: codes at byte `seq` of the tract buffer (a multiple of 16), traceback pointers from
// uint4 `ptr` ([row block][lane], 64 / c rows to a block), group slot of the round, status slot of the launch
struct NraConsItem {
    uint64_t seq;
    uint64_t ptr;
    int32_t n;
    int32_t group;
};

// Allele split (nra_split.hip, nra_split_host.cpp): pileup rows by the consensus alignment, column
// counts and site calls, two haplotypes per group.
#define NRA_SPLIT_SYM_DELETED 5               // row byte: the tract deleted the column (0..3 base, 4 a code-4 base)
#define NRA_SPLIT_SYM_NONE 6                  // matrix byte of a tract without a row
#define NRA_SPLIT_UNDECIDED 2                 // label of a row on neither haplotype
#define NRA_SPLIT_SITE_INTS 12                // column, two symbols, 4 + 4 counts, supported
#define NRA_SPLIT_RES_INTS 8                  // split, reads in 0, in 1, undecided, left out, sites, supported, iterations
#define NRA_SPLIT_THREADS 256                 // k_split_count and k_split_phase

// one alignment of a launch, as NraConsItem; its row starts at byte `row` of the row buffer (a multiple of 16)
struct NraSplitItem {
    uint64_t seq;
    uint64_t ptr;
    uint64_t row;
    int32_t n;
    int32_t group;
};

// one group: backbone at byte `bb` (t codes); rowtab[rows .. rows + m): the byte offset of each tract's row, -1 without
// one; its t column entries from `col`; its [site][tract] matrix from byte `mat` (min(max_sites, t) * m bytes); its site
// records from record `site` (room for min(max_sites, t)); its tracts' labels from `first`
struct NraSplitGroup {
    uint64_t bb;
    uint64_t rows;
    uint64_t col;
    uint64_t mat;
    uint64_t site;
    int32_t t, m, mv, first;
};

// one workgroup of k_split_count: 256 columns of a group from col0
struct NraSplitBlock {
    int32_t group, col0;
};

struct NraSplitParams {
    int32_t min_count, min_share_pct, min_purity_pct, min_sites, max_sites, max_iter;
};

// Flank haplotypes (nra_flank.hip, nra_flank_host.cpp): pileup rows of the reads' flank segments on
// the two reference flanks of a region, by the band DP with a pinned start and a free end, site calls with a coverage
// per column, and k_split_phase for the two haplotypes.  A group's device columns are its left side, padded to a
// multiple of 16, then its right side: both sides of a row start on a 16-byte boundary, and the host maps the columns
// back.
#define NRA_FLANK_SYM_NONE 6                  // row byte: the segment does not cover the column (= NRA_SPLIT_SYM_NONE)

// one (row, side) alignment of a launch: segment codes at byte `seq` (a multiple of 16, n codes), its side's codes at
// byte `bb` (t codes), traceback pointers from uint4 `ptr`, the side's part of the row from byte `row` (a multiple of 16)
struct NraFlankItem {
    uint64_t seq;
    uint64_t ptr;
    uint64_t row;
    uint64_t bb;
    int32_t n, t;
};

#ifdef __cplusplus
extern "C" {
#endif

// flank haplotypes (nra_flank.hip).  Alignment: workgroup i (one wave) aligns items[i] in band class c; a decided
// segment leaves status[2 i] = its distance, status[2 i + 1] = j*, and the codes of the columns below j* in its row
// (the rest of the row keeps the NRA_FLANK_SYM_NONE the host set); else status[2 i] = NRA_CONS_WIDEN or
// NRA_CONS_LEFT_OUT.  Count: as nra_launch_split_count with the rows that cover the column in place of m_v, and no site
// at a side offset below `skip`; lpad[g] = the device column of group g's right side
int nra_launch_flank_align(hipStream_t st, int c, int n_items, const NraFlankItem* items, const uint8_t* seqs,
                           const uint8_t* backbones, uint4* ptrs, uint8_t* rows, int32_t* status, int max_dist);
int nra_launch_flank_count(hipStream_t st, int n_blocks, const NraSplitBlock* blocks, const NraSplitGroup* groups,
                           const int32_t* lpad, const int64_t* rowtab, const uint8_t* rows, NraSplitParams prm, int skip,
                           int32_t* col_nb, uint8_t* col_ab);

// allele consensus (nra_consensus.hip).  Alignment: workgroup i (one wave) aligns items[i] in band class c (1, 2, 4, 8
// or 16) and, when its banded distance d proves exact and d <= max_dist, adds its votes to the group's tables, 1 to
// voters[group], and writes status[i] = d; else status[i] = NRA_CONS_WIDEN or NRA_CONS_LEFT_OUT.  Build: wave g writes
// the new backbone and supports of groups[g] and res[3 g ..] = new length, changed (0 / 1), voters
int nra_launch_cons_align(hipStream_t st, int c, int n_items, const NraConsItem* items, const NraConsGroup* groups,
                          const uint8_t* seqs, const uint8_t* backbones, uint4* ptrs, int32_t* tabs, int32_t* voters,
                          int32_t* status, int max_dist);
int nra_launch_cons_build(hipStream_t st, int n_groups, const NraConsGroup* groups, const uint8_t* backbones,
                          const int32_t* tabs, const int32_t* voters, uint8_t* new_backbones, int32_t* support,
                          int32_t* res);

// allele split (nra_split.hip).  Alignment: as nra_launch_cons_align, but a decided tract leaves its row of column
// symbols at rows + item.row instead of votes.  Count: per column of every group the base counts over its rows; a site
// leaves n[b] in col_nb and (a << 2 | b) in col_ab, any other column 0.  Phase: workgroup g lists the sites of group g,
// cuts them to max_sites, gathers the matrix and runs steps 3 and 4 of the contract; col_pos and col_key are its
// scratch lists (t entries per group, like col_nb)
int nra_launch_split_align(hipStream_t st, int c, int n_items, const NraSplitItem* items, const NraSplitGroup* groups,
                           const uint8_t* seqs, const uint8_t* backbones, uint4* ptrs, uint8_t* rows, int32_t* status,
                           int max_dist);
int nra_launch_split_count(hipStream_t st, int n_blocks, const NraSplitBlock* blocks, const NraSplitGroup* groups,
                           const int64_t* rowtab, const uint8_t* rows, NraSplitParams prm, int32_t* col_nb,
                           uint8_t* col_ab);
int nra_launch_split_phase(hipStream_t st, int n_groups, const NraSplitGroup* groups, const int64_t* rowtab,
                           const uint8_t* rows, NraSplitParams prm, const int32_t* col_nb, const uint8_t* col_ab,
                           int32_t* col_pos, int32_t* col_key, uint8_t* mats, int32_t* labels, int32_t* sites,
                           int32_t* res);

// the error message nra_last_error() returns; returns `code` (nra_host.cpp)
int nra_set_error(int code, const char* msg);

// mixture fits (nra_mixture.hip): workgroup b fits fits[fit_ids[b]].  d in {1, 2}; kreg in {NRA_MIX_KREG_SMALL,
// NRA_MIX_KREG, 0 = streaming} and every problem of the launch has n <= 256 * kreg unless kreg is 0.  Writes lb[f],
// iter[2 f] = E-steps, iter[2 f + 1] = converged, and w[off + c], mu / var[2 (off + c) + axis]
int nra_launch_mixture(hipStream_t st, int d, int kreg, int n, const int32_t* fit_ids, const NraMixFit* fits,
                       const NraMixProblem* probs, const double* samples, const int32_t* starts, double* lb, double* w,
                       double* mu, double* var, int32_t* iter);

// bootstrap of the mixture fits (nra_bootstrap.hip): workgroup g runs replicate jobs[g] % n_rep of problem
// jobs[g] / n_rep.  d and kreg as for nra_launch_mixture, with n = 100 m
int nra_launch_mixture_boot(hipStream_t st, int d, int kreg, int n, const int32_t* jobs, int n_rep,
                            const NraBootProblem* probs, const double* x, const double* z, const int32_t* idx,
                            const int32_t* starts, int32_t* status, int32_t* order, int32_t* best_start, double* lb,
                            double* w, double* mu, double* var);

// censored allele fit (nra_censored.hip).  Fit: workgroup b (one wave) fits fits[ids[b]] from the means at starts[nu_off
// ..]; kreg is NRA_CENS_KREG (every problem of the launch has n_points <= 64 * kreg) or 0 = streaming.  Writes ll[f],
// iter[2 f] = E-steps, iter[2 f + 1] = converged, nu[nu_off + k], w[w_off + k].  Resp: workgroup b (one wave) writes
// the n_points x (n + open) posteriors of models[b] from w and nu
int nra_launch_censored_fit(hipStream_t st, int kreg, int n, const int32_t* ids, const NraCensFit* fits,
                            const double* values, const double* starts, int max_iter, double tol, double* ll, double* w,
                            double* nu, int32_t* iter);
int nra_launch_censored_resp(hipStream_t st, int n, const NraCensFit* models, const double* values, const double* w,
                             const double* nu, double* resp);
// bootstrap of the censored fit (nra_censored.hip).  Boot: workgroup g (one wave) runs model (n, open) = slot
// g % (2 max_alleles) of replicate jobs[g / (2 max_alleles)] (replicate r = problem r / n_rep, row r % n_rep, rep_m[r]
// exact positions) and writes recs[r * 2 max_alleles + slot]; kreg is NRA_CENS_KREG (every problem of the launch has n_points <= 64 * kreg
// and its replicates' values are staged in LDS) or 0 = streaming.  Pick: one lane per
// replicate 0 .. n_replicates - 1 reads its records and writes its outputs (nu: 8 per replicate, w: 9)
int nra_launch_censored_boot(hipStream_t st, int kreg, int n_jobs, const int32_t* jobs, int n_rep, int max_alleles,
                             const NraCensBootProblem* probs, const double* values, const int32_t* idx,
                             const int32_t* rep_m, int max_iter, double tol, NraCensBootRec* recs);
int nra_launch_censored_pick(hipStream_t st, int n_replicates, int n_rep, int max_alleles,
                             const NraCensBootProblem* probs, const int32_t* rep_m, const NraCensBootRec* recs,
                             int32_t* status, int32_t* model_n, int32_t* model_open, int32_t* best_start,
                             int32_t* n_iter, double* ll, double* bic, double* nu, double* w);

// copies between pageable host memory and the device through the calling thread's pinned stage (nra_host.cpp);
// they return a hipError_t
int nra_copy_h2d(void* dst, const void* src, size_t bytes);
int nra_copy_d2h(void* dst, const void* src, size_t bytes);

// anchor screen (nra_screen.hip): one workgroup per tile.  Entries go to entries[0, cap); *count ends as the number of
// entries wanted, which may exceed cap (the host then grows the list and runs again)
int nra_launch_screen_hits(hipStream_t st, int64_t n_tiles, const NraScreenTile* tiles, const uint8_t* seqs, int k,
                           const uint64_t* table, int log2_slots, const uint32_t* postings, NraScreenEntry* entries,
                           unsigned long long cap, unsigned long long* count);
// motif screen (nra_screen_motifs.hip): the same tiles and chunk copy; entries and *count as above, `set` = class
int nra_launch_screen_motifs(hipStream_t st, int64_t n_tiles, const NraScreenTile* tiles, const uint8_t* seqs, int k,
                             const uint16_t* class_tab, NraScreenEntry* entries, unsigned long long cap,
                             unsigned long long* count);
// repeat scan (nra_scan.hip): one workgroup per tile.  Segments go to segments[0, cap); *count ends as the number of
// segments the tiles have, which may exceed cap (the host then grows the list and runs again); tile_valid[i] = the
// valid windows of tile i (a store per tile: one counter for all tiles would be one more contended atomic per tile)
int nra_launch_scan_repeats(hipStream_t st, int64_t n_tiles, const NraScanTile* tiles, const uint8_t* seqs, int k,
                            const uint16_t* class_tab, NraScanSegment* segments, unsigned long long cap,
                            unsigned long long* count, uint32_t* tile_valid);

// sketches (nra_sketch.hip): one workgroup per sequence.  Sequence s = bytes [seq_base[s], seq_base[s] + seq_len[s]) of
// `seqs` (padded by 64 bytes); its sketch goes, ascending, to sketch[sk_off[s] ...], its size to sk_len[s] and its
// number of valid windows to n_valid[s]
int nra_launch_sketch(hipStream_t st, int32_t n_seqs, const uint8_t* seqs, const int64_t* seq_base, const int32_t* seq_len,
                      int k, const int64_t* sk_off, uint32_t* sketch, int32_t* sk_len, int32_t* n_valid);
// sketch pairs (nra_sketch.hip): workgroups [tile0, tile0 + n_tiles) of the implicit tile list, n_tiles at most
// NRA_SKETCH_LAUNCH_TILES.  Position s of the
// sorted order (sequences by group, then index) owns the tiles [tile_first[s], tile_first[s + 1]): block t of it is the
// positions s + 1 + 64 t ... below grp_end[s].  order[s] is the sequence at position s.  Pairs with at least min_shared
// shared k-mers go to pairs[0, cap); *count ends as their number, which may exceed cap
int nra_launch_sketch_pairs(hipStream_t st, int64_t tile0, int64_t n_tiles, int32_t n_sorted, const int64_t* tile_first,
                            const int32_t* order, const int32_t* grp_end, const int64_t* sk_off, const uint32_t* sketch,
                            const int32_t* sk_len, int min_shared, NraSketchPair* pairs, unsigned long long cap,
                            unsigned long long* count);

// placement (nra_place.hip): one workgroup per tile of NRA_PLACE_TILE windows of the n_win windows whose bytes start at
// `seqs` (16-byte aligned, padded by 64 bytes); the window at byte w has contig position pos0 + w.  A window whose
// canonical k-mer is a key adds 1 to occ[slot] and appends a record, unless it read occ[slot] > ceiling.  `records`
// holds n_win records: it cannot overflow.  *count ends as the number of records, *n_valid grows by the valid windows
int nra_launch_place_hits(hipStream_t st, int64_t n_win, const uint8_t* seqs, int k, const uint64_t* table,
                          int log2_slots, uint32_t* occ, uint32_t ceiling, int32_t contig, int64_t pos0,
                          NraPlaceRecord* records, unsigned long long* count, unsigned long long* n_valid);

// repeat structure (nra_structure.hip): one lane per read, forward DP then traceback.  P in {1..6, 8, 16, 32, 64};
// res[2 i] = edits, res[2 i + 1] = start phase of read i
int nra_launch_structure(hipStream_t st, int P, int n_reads, const NraStructRead* reads, const NraStructMotif* motifs,
                         const uint8_t* codes, uint32_t* ptrs, uint8_t* path, int32_t* res);

// motif runs (nra_segment.hip): one lane per tract, forward DP then traceback.  SC in {8, 16, 32}; res[4 i ..] = edits,
// start phase, start motif of tract i; `which`: the motif index per tract base, laid out as `path`
int nra_launch_segment(hipStream_t st, int SC, int n_tracts, const NraStructRead* tracts, const NraSegSet* sets,
                       const uint8_t* codes, int switch_cost, uint32_t* ptrs, uint8_t* path, uint8_t* which,
                       int32_t* res);

// anchored extension (nra_extend.hip): one lane per read, forward only, reads and motifs as for nra_launch_structure
// (NraStructRead.ptr unused).  P in {1..6, 8, 16, 32, 64}; res[4 i ..] = score, end row, end phase, motif bases of read i
int nra_launch_extend(hipStream_t st, int P, int n_reads, const NraStructRead* reads, const NraStructMotif* motifs,
                      const uint8_t* codes, int match, int mismatch, int gap, int32_t* res);

// tandem motifs (nra_motif.hip): one wave per tract, n_grid workgroups of four waves.  n_tandem[t * 6 + p - 1] and
// top_key[t * 8 + q] (count << 10 | (1023 - dense id), 0 for an unused slot) for q < top_n
int nra_launch_tract_motifs(hipStream_t st, int n_grid, int n_tracts, const NraMotifTract* tracts,
                            const uint8_t* codes, const int16_t* dense_of, int max_p, int top_n, int32_t* n_tandem,
                            uint32_t* top_key);

// tandem periods (nra_period.hip): one wave per tract, n_grid workgroups of four waves.  match / valid[t * 64 + p - 1]
int nra_launch_tract_periods(hipStream_t st, int n_grid, int n_tracts, const NraPeriodTract* tracts,
                             const uint8_t* codes, int32_t* match, int32_t* valid);

// CpG methylation (nra_methyl.hip, nra_methyl_host.cpp): one workgroup of 256 threads per read.
#define NRA_METH_THREADS 256
#define NRA_METH_F_REVERSED 1                 // bit 0 of a read's flags: stored reversed
#define NRA_METH_F_IMPLICIT 2                 // bit 1: a C the list skips is unmodified
#define NRA_METH_F_TOO_MANY 4                 // set by the host: m > n, BAD_TAG without being decoded
// one read of a launch: its bytes start at byte `seq` of the chunk's sequence buffer, its list at entry `mod` of the
// chunk's deltas (overwritten by the ranks L) and call bytes; its result is row `out` of the chunk's results
struct NraMethRead {
    uint64_t seq;
    uint64_t mod;
    int32_t n;
    int32_t m;
    int32_t lo;
    int32_t hi;
    int32_t flags;
    int32_t pad;
};
// n_grid workgroups stride over the reads.  counts[r][2 nb + 1][5], n_c[r], status[r]; ranks: the deltas, in place
int nra_launch_read_methylation(hipStream_t st, int n_grid, int n_reads, const NraMethRead* reads, const uint8_t* seqs,
                                int32_t* ranks, const uint8_t* probs, int flank, int bin, int nb, int lo_byte,
                                int hi_byte, int32_t* counts, int32_t* n_c, int32_t* status);

// launchers (nra_kernels.hip).  All asynchronous on `st`; return hipError_t as int.
int nra_launch_score_pk16(int R, int has_n, hipStream_t st, int n_tasks,
                          const NraPairTask* tasks, NraSeqArgs seq, int32_t* out_score);

// payload kernels walk a device-side queue of *count tasks with a grid stride.  ORIGIN outputs (score, tstart,
// tend); WINDOW outputs (score, wscore).  chain_buf != NULL: row-block chaining (n_waves strips of
// 6 * chain_cap cells each); wide: int64 cells (R = NRA_WIDE_R_SMALL / NRA_WIDE_R_LARGE, or chained)
int nra_launch_payload_origin(int R, int has_n, hipStream_t st, int n_waves,
                              const NraTask* tasks, const int32_t* count, NraSeqArgs seq,
                              int32_t* out_score, int32_t* out_p, int32_t* out_tend,
                              void* chain_buf, int chain_cap, int wide);
int nra_launch_payload_window(int R, int has_n, hipStream_t st, int n_waves,
                              const NraTask* tasks, const int32_t* count, NraSeqArgs seq,
                              int32_t* out_score, int32_t* out_p, int32_t* out_tend,
                              void* chain_buf, int chain_cap, int wide);

// junction decomposition (nra_sweep.hip): the reverse sweep over rev(R) writes the R-side snapshot and A
// (per read: read_a); the forward sweep combines and writes Score(k) + the flank-test verdict (0 fail,
// 1 pass, 2 ambiguous).  chain: int32 cells, one read per task, min(n_tasks, n_strips) waves
int nra_launch_sweep_bwd(int R, int has_n, int chain, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                         NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips);
int nra_launch_sweep_fwd(int R, int has_n, int chain, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                         NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips);

// the same sweeps with the lane-to-lane hand-off through an LDS ring (k_sweep_ring: one read block per wave,
// forward sweep skewed by the unit length so that the junction combine runs on every m-th step only);
// unchained reads, unit length <= NRA_SWEEP_RING_MAX_M.  half: the half-wave kernel (k_sweep_ring32), reads of up to
// 32 * NRA_RING32_MAX_R bases, two read pairs of one region per wave (32 lanes each); R from NRA_R_LIST up to
// NRA_RING32_MAX_R (16: 301.8, 20: 299.7, 24: 297.4 ms on config 4; 32, which would take config 2's 950-base reads too:
// 5.65 -> 7.1 ms there, 281 -> 288 ms on config 4)
#define NRA_SWEEP_RING_MAX_M 8
#define NRA_RING32_MAX_R 24
int nra_launch_sweep_ring_bwd(int R, int has_n, int half, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                              NraSweepArgs a, int relax_c, int32_t* redo);
int nra_launch_sweep_ring_fwd(int R, int has_n, int half, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                              NraSweepArgs a, int relax_c, int32_t* redo);
// relax_c > 0 (these and the quanta launcher): the taint scheme -- the anchor columns up to
// relax_c bases from the junction run the relaxed cell, and redo[task] is set where that may have reached an output;
// relax_c <= 0 and redo non-null: the exact sweeps of the flagged tasks only (the re-sweep); both 0 / null: the exact sweeps.
// The switch step is flank - max(relax_c, 64) itself, where that is >= 64 (sweep_relax_steps): no multiple of anything.
#define NRA_RELAX_C_DEFAULT 256

// The lean run, one switch per item so that each can be measured by itself (-DNRA_...=0: as before it):
#ifndef NRA_RELAX_ROUND64
#define NRA_RELAX_ROUND64 0      // 1: the switch step rounded down to a multiple of 64, as before
#endif
#ifndef NRA_LEAN_CLEARS
#define NRA_LEAN_CLEARS 1        // no per-run clear of an array that a kernel of the run writes in full (run_1d)
#endif
#ifndef NRA_FETCH_ONE_COPY
#define NRA_FETCH_ONE_COPY 1     // the give-up words travel in the result block: no blocking copy of their own
#endif

// a bucket's reverse and forward sweeps as one launch of quanta taken by ticket (k_sweep_ringq).  A sweep is cut every
// `qsteps` steps (a multiple of 64; a forward sweep also at NRA_Q_CUT of its first boundary step) into parts; qlist holds one entry per part, direction << 31 | part << NRA_Q_PART_SHIFT |
// task, ordered [reverse parts 0 of every task | reverse parts 1 | ... | forward parts 0 | ...]; the host and the kernel
// count a sweep's steps with the same macros.  `arrivals`: two counters per task (finished reverse / forward parts) and
// `ticket`, zeroed before the launch; `giveup` the launch-wide give-up word; qstate: slots of NRA_QSTATE_INTS(R) x 64 int32
// (the registers, the ring's places, then the pending outputs and boundary accumulators), one per forward sweep and then,
// where a reverse sweep has more than one part, one per reverse sweep; half: the half-wave buckets, as above
#define NRA_QSTATE_INTS(R) (((4 * (R) + 2 + 3) / 4 + NRA_SWEEP_RING_MAX_M + 1) * 4)
#define NRA_Q_PART_SHIFT 27
#define NRA_Q_PART_MASK 15u
#define NRA_Q_TASK_MASK ((1u << NRA_Q_PART_SHIFT) - 1u)
#define NRA_Q_MAX_PARTS 16
#define NRA_Q_STEPS 384          // steps of a part (config 2: a reverse sweep in 3 parts, a forward sweep in 7)
#define NRA_Q_CUT(jfirst) ((jfirst) < 0 ? 0 : (jfirst) / 64 * 64)      /* a forward sweep's first cut: before its first boundary step */
#define NRA_Q_WHOLE (1 << 30)   // "steps of a part" of a batch too small for more cuts (longer than any sweep): a reverse sweep, a forward sweep to
                                // its first cut, the rest
// The saturation exit: a forward sweep whose wave state repeats from one unit boundary to the next ends there and
// writes the last emission for every repeat count left.  The exiting wave sets the sweep's forward arrival word to
// NRA_Q_FINISHED, which no count of parts reaches: the sweep's later parts leave at their poll.  sat_steps: the state is
// compared m steps behind a part's start and, > 0, m steps behind a checkpoint every so many steps; < 0: no exit.
// sat_count: four words of the run per bucket, 8-byte aligned: [0] sweeps that left, [2..3] the steps they skipped (64 bits).
#ifndef NRA_SAT_EXIT
#define NRA_SAT_EXIT 1           // 0: the body without the check, as before it
#endif
#ifndef NRA_SAT_STEPS
#define NRA_SAT_STEPS 192        // steps between the checkpoints inside a part (0: a part's start only).  Config 2, ms per step,
                                 // medians of 7: no exit 4.41; 0: 4.29; 128: 4.33; 192: 4.26 (a checkpoint a never-repeating sweep stores is lost time)
#endif
#define NRA_Q_FINISHED (1 << 30)
#define NRA_Q_STEPS_REV(l3, half) ((l3) + ((half) ? 31 : 63))
#define NRA_Q_STEPS_FWD(l1, m, kmax, half) ((l1) + (m) * (kmax) + ((half) ? 31 : 63) * (m))
int nra_launch_sweep_ringq(int R, int has_n, int half, hipStream_t st, int n_quanta, const uint32_t* qlist, int qsteps, int n_tasks, int32_t* ticket,
                           int32_t* arrivals, int32_t* giveup, int32_t* qstate, const NraSweepTask* tasks, NraSweepArgs a,
                           int relax_c, int32_t* redo, int sat_steps, int32_t* sat_count);

// chained LDS-ring sweeps (k_sweep_ringchain): reads of more than NRA_RING_CHAIN_MIN_ROWS rows as row blocks of
// 64 * NRA_RING_CHAIN_R; wide = 0: two reads per wave in packed int16, 1: one read per wave in int32 cells.
// chain_buf: n_strips strips of 10 * chain_cap int32; the launch has min(n_tasks, n_strips) waves
#define NRA_RING_CHAIN_R 20
#define NRA_RING_CHAIN_MIN_ROWS NRA_MAX_QLEN_1BLOCK   // shorter reads stay unchained: a block costs a pipeline fill and half a block of padding
#define NRA_RING_CHAIN_STRIPS 4096
// rows per lane of the chained sweeps whose row blocks run as concurrent waves (k_sweep_ringmt): 15 keeps the forward
// sweep within the 168 registers of three waves per SIMD (20: two)
#ifndef NRA_RING_MT_R
#define NRA_RING_MT_R 15
#endif
#define NRA_RING_MT_FROM 1536                  // reads of more rows than this may run as row blocks: one register block would take 28 - 48
                                               // rows per lane, one wave per SIMD (the batch takes the cheaper form: nra_batch1d_create)
#define NRA_RING_MT_R_MIN 12                   // ... down to 12: the host takes the height that pads a bucket's reads least
int nra_launch_sweep_ringchain_bwd(int R, int has_n, int wide, hipStream_t st, int n_tasks,
                                   const NraSweepTask* tasks, NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips);
int nra_launch_sweep_ringchain_fwd(int R, int has_n, int wide, hipStream_t st, int n_tasks,
                                   const NraSweepTask* tasks, NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips);

// chained LDS-ring sweeps with the row blocks of a read as concurrent waves (k_sweep_ringmt).  `ticket`: one int32
// (zeroed by the launcher); `strips`: n strips x 5 x chain_cap granules, zeroed once; `epoch`: unique per launch,
// never 0; `error`: launch-wide give-up word (zeroed by the host before the run, read back after it)
int nra_launch_sweep_ringmt_bwd(int R, int has_n, int wide, hipStream_t st, int n_blocks,
                                const NraChainBlock* blocks, int32_t* ticket, const NraSweepTask* tasks,
                                NraSweepArgs a, uint64_t* strips, int chain_cap, uint32_t epoch, int32_t* error);
int nra_launch_sweep_ringmt_fwd(int R, int has_n, int wide, hipStream_t st, int n_blocks,
                                const NraChainBlock* blocks, int32_t* ticket, const NraSweepTask* tasks,
                                NraSweepArgs a, uint64_t* strips, int chain_cap, uint32_t epoch, int32_t* error);

// 2D junction decomposition (nra_joint.hip)
int nra_launch_joint_bwd(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                         int32_t* snap, int32_t* read_a, const int32_t* pstate);
int nra_launch_joint_prefix(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                            const int32_t* k1list, int32_t* state, const int32_t* pstate);
// packed int16 sweep of the payload-free columns (dir 1: L, dir 0: rev(R)), two reads per wave; dir < 0: both sides in one
// launch, an L-side task marked in bit 63 of its state index and leaving its state at pstate_l
int nra_launch_joint_pk16(int R, int has_n, hipStream_t st, int n_tasks, const NraJointPairTask* tasks, NraSeqArgs seq, int dir,
                          int32_t* pstate, int32_t* pstate_l);
// junction at the end of mid: extended reverse sweeps, MID sweeps, the per-cell combine
int nra_launch_joint_bwd_ext(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                             int32_t* rsnap, int32_t* ra, const int32_t* pstate);
int nra_launch_joint_mid(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                         int32_t* state, int32_t* fsnap, int32_t* fb);
// ... with the MID part as column-parallel scans (k_joint_midscan): the prefix sweep leaves column states (each lane on its own step)
int nra_launch_joint_prefix_cols(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                                 const int32_t* k1list, int32_t* state, const int32_t* pstate);
int nra_launch_joint_midscan(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                             const int32_t* k1list, const int32_t* state, int32_t* fsnap, int32_t* fb,
                             const NraGridRow* rows);
int nra_launch_joint_combine(hipStream_t st, int n_tasks, const NraJointCombineTask* tasks, const NraDevRead* reads,
                             NraScoreParams sp, const int32_t* fsnap, const int32_t* rsnap, const int32_t* fb,
                             const int32_t* ra, int32_t* cell_score, int32_t* cell_wscore, const NraGridRow* rows);
// a refinement routed on the device (nra_batch2d_refine): rows != NULL in the two launchers above
int nra_launch_joint_refine_route(hipStream_t st, int n_reads, const uint8_t* status, const int32_t* n_ties,
                                  const int64_t* sum_k1, const int64_t* sum_k2, const double* lo1, const double* hi1,
                                  const double* lo2, const double* hi2, int buf1, int buf2, const NraGridRow* keep,
                                  NraGridRow* rows, uint32_t* cell_cnt, const int32_t* rowspad, const NraDevRead* reads,
                                  const NraDevRegion* regions, unsigned long long* words);
int nra_launch_joint_tail(int R, int has_n, hipStream_t st, int n_tasks, const NraJointTask* tasks, NraSeqArgs seq,
                          int32_t* state, int32_t* snap, int32_t* read_a, int32_t* cell_score,
                          int32_t* cell_wscore);

// alignment paths (nra_trace.hip)
int nra_launch_trace_fill(int R, int has_n, hipStream_t st, int n_tasks, const NraTraceTask* tasks, NraSeqArgs seq,
                          uint8_t* trace, int32_t* out);
int nra_launch_trace_back(hipStream_t st, int n_tasks, const NraTraceTask* tasks, const NraDevRead* reads,
                          const NraDevRegion* regions, const uint8_t* trace, const int32_t* fill_out,
                          uint8_t* ops, int32_t* out);
int nra_launch_trace_fill_mt(int R, int has_n, int wide, hipStream_t st, int n_blocks, const NraTraceBlock* blocks,
                             int32_t* ticket, const NraTraceTask* tasks, NraSeqArgs seq, uint8_t* trace,
                             int32_t* blk_best, uint64_t* strips, uint32_t epoch, int32_t* error);
int nra_launch_trace_best(hipStream_t st, int n_tasks, const NraTraceTask* tasks, const NraDevRead* reads,
                          int block_rows, int wide, const int32_t* blk_best, NraScoreParams sp, int32_t* out);

// 1D selectors (one wave per read).  append_mode: 0 none, 1 ambiguous ties only, 2 every tie.  cand_tstart / cand_tend
// non-null: every candidate's extents are set to -1 ("not computed") on the way -- the extents kernel, which runs behind
// this one, overwrites those of the ties it resolves (null: it has run already, NRA_F_ALL_EXTENTS).
// q_giveup / mt_giveup (either may be null) -> giveup_out[0 / 1]: the give-up words of the run's quanta and row blocks,
// copied by the run's last kernel into the result block, so that a fetch needs no copy of their own for them
int nra_launch_select_best_1d(hipStream_t st, int n_reads, const int32_t* kmin, const int32_t* kmax,
                              const uint32_t* coff, const int32_t* cand_score, const uint8_t* cand_flag,
                              const int32_t* read_bucket, const uint32_t* bucket_task_base,
                              int append_mode, NraTask* ext_tasks, int32_t* ext_count,
                              int32_t* best_score, int32_t* cand_tstart, int32_t* cand_tend);
int nra_launch_select_final_1d(hipStream_t st, int n_reads, const int32_t* kmin, const int32_t* kmax,
                               const uint32_t* coff, const NraDevRead* reads,
                               const NraDevRegion* regions,
                               const int32_t* cand_score, const uint8_t* cand_flag,
                               const int32_t* cand_tstart, const int32_t* cand_tend,
                               const int32_t* best_score,
                               int64_t* sum_k, int32_t* n_ties, uint8_t* status,
                               const int32_t* q_giveup, const int32_t* mt_giveup, int32_t* giveup_out);
// 2D: strand choice from the probe scores, then the per-read selector over its cells
int nra_launch_pick_strand(hipStream_t st, int n_reads, const int32_t* probe_score,
                           const int8_t* strand_in, int8_t* strand_out, NraDevRead* reads);
int nra_launch_select_2d(hipStream_t st, int n_reads, const uint32_t* cell_first,
                         const uint32_t* cell_cnt, const int32_t* cell_k1, const int32_t* cell_k2,
                         const NraGridRow* grid_rows, int grid_step1, int grid_step2,
                         const int32_t* cell_score, const int32_t* cell_wscore,
                         int32_t* best_w, int64_t* sum_k1, int64_t* sum_k2, int32_t* n_ties,
                         uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif
