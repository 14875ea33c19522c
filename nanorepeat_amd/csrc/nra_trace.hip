// nra_trace.hip -- alignment paths (CIGAR) for chosen (query, target) pairs (gfx950).
// Row 8f-2 of SURVEY.md: PAF/CIGAR emission in the reference's wire format (paf.py:32-79,
// consumers tk.py:405-500), for the few alignments a caller wants to look at -- not the hot path.
//
//   k_trace_fill<R,HAS_N>  the ORIGIN-payload DP of k_payload_i32 that also writes one byte per
//                          cell: which input gave H (with the oracle's preference d, E, F, E2, F2
//                          and "continue" vs "start here" for the diagonal), whether each of the
//                          four gap states leaving the cell extends or opens (extend preferred on
//                          ties, like the oracle's traceback), and whether the bases are equal.
//   k_trace_back           one thread per alignment walks the bytes back from the best cell
//                          (smallest column, then smallest row, holding the maximum) and writes
//                          the operations in reverse; the host run-length encodes them.
// The result is the string the CPU oracle's traceback produces, bit for bit.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#define TNEG (-(1 << 29))
#define T_SRC_DIAG 0      // H came through the diagonal and the path continues at (i-1, j-1)
#define T_SRC_E 1
#define T_SRC_F 2
#define T_SRC_E2 3
#define T_SRC_F2 4
#define T_SRC_START 5     // diagonal from an empty alignment: the path starts at this cell
#define T_E_EXT 0x08      // E(i, j+1) extends E(i, j)   (else it opens from H(i, j))
#define T_F_EXT 0x10      // F(i+1, j) extends F(i, j)
#define T_E2_EXT 0x20
#define T_F2_EXT 0x40
#define T_EQ 0x80         // the two bases are equal ('=' rather than 'X')

template <int R, bool HAS_N>
__global__ __launch_bounds__(WAVE) void k_trace_fill(int n_tasks, const NraTraceTask* __restrict__ tasks, NraSeqArgs seq,
                                                     uint8_t* __restrict__ trace,
                                                     int32_t* __restrict__ out)   // 5 per task: score, tstart, tend, best_i, best_j
{
    NRA_SEQ_LOCALS(seq)
    const int task = blockIdx.x;
    if (task >= n_tasks) return;
    const int lane = threadIdx.x;
    const NraTraceTask tk = tasks[task];
    const NraDevRead rd = reads[tk.read];
    const NraDevRegion rg = regions[tk.region];
    const uint8_t* __restrict__ tgt = pool + rg.p1_off;
    const int ncols = rg.l1;
    uint8_t* __restrict__ tr = trace + tk.trace_off;

    int qc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) qc[i] = query_code<HAS_N>(rd, q2bit, qnmask, lane * R + i);

    int Hprev[R], E[R], E2[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { Hprev[i] = TNEG; E[i] = TNEG; E2[i] = TNEG; }
    int Hbot = TNEG, Fout = TNEG, F2out = TNEG, Hup_prev = TNEG;
    int best = 0xffff, bestj = -1, besti = -1;
    int tt = NRA_PAD_T;
    int j = -lane;
    const int sA = sp.match << 16, sB = -(sp.mismatch << 16), sN = -(sp.ambi << 16);
    const int o1 = -(sp.open1 << 16), x1 = -(sp.ext1 << 16);
    const int o2 = -(sp.open2 << 16), x2 = -(sp.ext2 << 16);

    const int nchunks = (ncols + 63 + 63) >> 6;
    for (int c = 0; c < nchunks; ++c) {
        const int col = c * 64 + lane;
        int feed = col < ncols ? tgt[col] : NRA_PAD_T;
#pragma unroll 1
        for (int s = 0; s < 64; ++s) {
            int F = dpp_shr1(TNEG, Fout);
            int F2 = dpp_shr1(TNEG, F2out);
            tt = dpp_shr1(feed, tt);
            feed = dpp_rol1(feed);
            const int fresh = j;
            int diag = Hup_prev;
            Hup_prev = dpp_shr1(TNEG, Hbot);
            const bool live = j >= 0 && j < ncols;
            int colmax = TNEG, rowmax = 0, h = TNEG;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const bool eq = qc[i] == tt;
                int sc = eq ? sA : sB;
                if (HAS_N) {
                    if ((qc[i] | tt) & 4) sc = sN;
                }
                const int d = imax(diag, fresh) + sc;
                h = imax(imax(d, E[i]), F);
                h = imax(imax(h, E2[i]), F2);
                int src = d == h ? (diag >= fresh ? T_SRC_DIAG : T_SRC_START)
                                 : (E[i] == h ? T_SRC_E : (F == h ? T_SRC_F : (E2[i] == h ? T_SRC_E2 : T_SRC_F2)));
                if (h > colmax) { colmax = h; rowmax = i; }
                diag = Hprev[i];
                Hprev[i] = h;
                const int ee = E[i] + x1, eo = h + o1;
                const int fe = F + x1, fo = h + o1;
                const int ee2 = E2[i] + x2, eo2 = h + o2;
                const int fe2 = F2 + x2, fo2 = h + o2;
                if (ee >= eo) src |= T_E_EXT;
                if (fe >= fo) src |= T_F_EXT;
                if (ee2 >= eo2) src |= T_E2_EXT;
                if (fe2 >= fo2) src |= T_F2_EXT;
                if (eq) src |= T_EQ;
                E[i] = imax(ee, eo);
                F = imax(fe, fo);
                E2[i] = imax(ee2, eo2);
                F2 = imax(fe2, fo2);
                const int row = lane * R + i;
                if (live && row < rd.qlen) tr[(size_t)row * ncols + j] = (uint8_t)src;
            }
            if (colmax > best) { best = colmax; bestj = j; besti = lane * R + rowmax; }
            Hbot = h; Fout = F; F2out = F2;
            ++j;
        }
    }
    // wave reduce: max packed value, then smallest column, then smallest row
    int vmax = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmax = imax(vmax, __shfl_xor(vmax, off, WAVE));
    int jm = (best == vmax) ? bestj : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) jm = imin(jm, __shfl_xor(jm, off, WAVE));
    int im = (best == vmax && bestj == jm) ? besti : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) im = imin(im, __shfl_xor(im, off, WAVE));
    if (lane == 0) {
        int32_t* o = out + (size_t)task * 5;
        const int sc = vmax >> 16;
        const int lo = sp.min_score > 1 ? sp.min_score : 1;
        if (sc >= lo && jm >= 0 && jm != 0x7fffffff) {
            o[0] = sc; o[1] = vmax & 0xffff; o[2] = jm + 1; o[3] = im; o[4] = jm;
        } else {
            o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; o[4] = -1;
        }
    }
}

// ops are written back to front: ops[cap-1], ops[cap-2], ...; n_ops and the start cell are returned
__global__ void k_trace_back(int n_tasks, const NraTraceTask* __restrict__ tasks,
                             const NraDevRead* __restrict__ reads, const NraDevRegion* __restrict__ regions,
                             const uint8_t* __restrict__ trace, const int32_t* __restrict__ fill_out,
                             uint8_t* __restrict__ ops, int32_t* __restrict__ out)   // 3 per task: n_ops, qstart, tstart
{
    const int task = blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= n_tasks) return;
    const NraTraceTask tk = tasks[task];
    const int ncols = regions[tk.region].l1;
    const int32_t* f = fill_out + (size_t)task * 5;
    int32_t* o = out + (size_t)task * 3;
    if (f[0] < 0) { o[0] = 0; o[1] = -1; o[2] = -1; return; }
    const uint8_t* __restrict__ tr = trace + tk.trace_off;
    uint8_t* __restrict__ op = ops + tk.ops_off;
    const int cap = tk.ops_cap;
    int i = f[3], j = f[4], st = 0, n = 0;
    int qs = -1, ts = -1;
    // bounded by qlen + tlen operations: every step moves up, left or both
    for (int guard = reads[tk.read].qlen + ncols + 2; guard > 0 && n < cap; --guard) {
        const int b = tr[(size_t)i * ncols + j];
        if (st == 0) {
            const int src = b & 7;
            if (src == T_SRC_DIAG || src == T_SRC_START) {
                op[cap - 1 - n++] = (b & T_EQ) ? '=' : 'X';
                if (src == T_SRC_START) { qs = i; ts = j; break; }
                --i; --j;
            } else st = src;                       // 1 E, 2 F, 3 E2, 4 F2: no operation yet
        } else if (st == T_SRC_E || st == T_SRC_E2) {
            op[cap - 1 - n++] = 'D';               // target base j against a gap
            const int prev = tr[(size_t)i * ncols + (j - 1)];
            if (!(prev & (st == T_SRC_E ? T_E_EXT : T_E2_EXT))) st = 0;
            --j;
        } else {
            op[cap - 1 - n++] = 'I';               // query base i against a gap
            const int prev = tr[(size_t)(i - 1) * ncols + j];
            if (!(prev & (st == T_SRC_F ? T_F_EXT : T_F2_EXT))) st = 0;
            --i;
        }
    }
    o[0] = n; o[1] = qs; o[2] = ts;
}

// ------------------------------------------------------------------------------------
// k_trace_fill_mt: the trace fill for queries of any length, in row blocks of 64 * R rows (nra_align_paths).
//
// A wave is one (pair, row block) and fills the block's rows of the pair's one qlen x tlen trace.  Block b + 1 gets,
// per column, what block b's last row leaves below it: H of that row and the two vertical-gap states entering the
// row beneath (whether they extend or open is already in the trace byte of block b's last row, which the block
// writes like any other).  The hand-off and its ordering are those of k_sweep_ringmt (nra_sweep.hip): lane 63 of
// block b stores 8-byte granules {epoch, value}, one agent-scope store each, into the strip between the two
// blocks; block b + 1 loads the granules of the 64 columns it is about to feed its lane 0 with agent-scope loads
// and polls until every tag carries the launch's epoch.  Waves take their (pair, block) by ticket from a list in
// which a producer precedes its consumer, so a producer is running or done and never waits for a larger ticket;
// the spin sleeps, is bounded (NRA_TRACE_SPIN_LIMIT polls) and watches a launch-wide error word.  The strips of a
// call are its own, zeroed before the launch, and the epoch is never 0.
//
// W: cells of 64 bits (score << 32 | origin column) for pairs whose score does not fit the 15 bits above the
// 16-bit origin of an int32 cell; a value then crosses the strip as two granules.  The origin column is part of
// every comparison, as in the oracle's packed (score, origin) cells, so it cannot be dropped from the cell.
// Each block leaves its best cell (value, column, row); k_trace_best reduces them with the tie-break of the one-block
// kernel: the maximum, then the smallest column, then the smallest row.
typedef unsigned long long nra_tu64;
typedef __attribute__((address_space(1))) nra_tu64 nra_tgu64;
typedef __attribute__((address_space(1))) int nra_tgi32;
#define NRA_TRACE_SPIN_LIMIT (1u << 20)   // as NRA_MT_SPIN_LIMIT: ~2.5 s, a hang guard and not a path

template <bool W> struct TraceCell { typedef int type; static constexpr int neg = TNEG, none = 0xffff; };
template <> struct TraceCell<true> { typedef long long type; static constexpr long long neg = -(1ll << 60), none = 0xffffffffll; };

template <int R, bool HAS_N, bool W>
__global__ __launch_bounds__(WAVE) void k_trace_fill_mt(int n_blocks, const NraTraceBlock* __restrict__ blocks,
                                                        int32_t* ticket, const NraTraceTask* __restrict__ tasks,
                                                        const NraDevRead* __restrict__ reads,
                                                        const NraDevRegion* __restrict__ regions,
                                                        const uint8_t* __restrict__ pool,
                                                        const uint32_t* __restrict__ q2bit,
                                                        const uint32_t* __restrict__ qnmask,
                                                        NraScoreParams sp, uint8_t* __restrict__ trace,
                                                        int32_t* __restrict__ blk_best,   // 4 per block: value lo, hi, column, row
                                                        nra_tu64* strips, uint32_t epoch, int32_t* error)
{
    typedef typename TraceCell<W>::type cell_t;
    constexpr int SH = W ? 32 : 16;
    constexpr int NV = W ? 2 : 1;                      // granules per value
    constexpr cell_t NEG = TraceCell<W>::neg;
    const int lane = threadIdx.x;
    int my = 0;
    if (lane == 0) my = atomicAdd(ticket, 1);
    my = __builtin_amdgcn_readfirstlane(my);
    if (my >= n_blocks) return;
    const NraTraceBlock cb = blocks[my];
    const NraTraceTask tk = tasks[cb.task];
    const NraDevRead rd = reads[tk.read];
    const NraDevRegion rg = regions[tk.region];
    const uint8_t* __restrict__ tgt = pool + rg.p1_off;
    const int ncols = rg.l1;
    const size_t cap = (size_t)((ncols + 63) & ~63);   // granules per plane of this pair's strips
    const bool first_blk = cb.blk == 0, last_blk = cb.blk == cb.nblk - 1;
    const nra_tgu64* cin = (const nra_tgu64*)(strips + (first_blk ? 0 : cb.strip_in));
    nra_tgu64* cout = (nra_tgu64*)(strips + (last_blk ? 0 : cb.strip_out));
    nra_tgi32* err = (nra_tgi32*)error;
    const nra_tu64 tag = (nra_tu64)epoch << 32;
    const int row_base = cb.blk * 64 * R;
    uint8_t* __restrict__ tr = trace + tk.trace_off;

    // what block b left under its last row at column `col` (each lane its own column): polled until the granules
    // carry this launch's epoch.  Wave-uniform control flow; false when the launch has failed.
    auto fetch = [&](int col, cell_t& h, cell_t& f, cell_t& f2) -> bool {
        h = NEG; f = NEG; f2 = NEG;
        if (first_blk) return true;
        const bool mine = col < ncols;
        const nra_tgu64* g = cin + (mine ? col : 0);
        for (unsigned spins = 0;; ++spins) {
            bool ok = true;
            if (mine) {
                nra_tu64 x[3 * NV];
#pragma unroll
                for (int p = 0; p < 3 * NV; ++p) {
                    x[p] = __hip_atomic_load(g + (size_t)p * cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = ok && (x[p] >> 32) == epoch;
                }
                if constexpr (W) {
                    h = (cell_t)((x[1] << 32) | (x[0] & 0xffffffffull));
                    f = (cell_t)((x[3] << 32) | (x[2] & 0xffffffffull));
                    f2 = (cell_t)((x[5] << 32) | (x[4] & 0xffffffffull));
                } else {
                    h = (cell_t)(int)(unsigned)x[0]; f = (cell_t)(int)(unsigned)x[1]; f2 = (cell_t)(int)(unsigned)x[2];
                }
            }
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) return true;
            __builtin_amdgcn_s_sleep(32);
            if ((spins & 15) == 15) {
                int failed = 0;
                if (lane == 0) failed = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane(failed) != 0) return false;
                if (spins >= NRA_TRACE_SPIN_LIMIT) {
                    if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return false;
                }
            }
        }
    };
    auto publish = [&](int value, int col, cell_t v) {
#pragma unroll
        for (int p = 0; p < NV; ++p)
            __hip_atomic_store(cout + (size_t)(value * NV + p) * cap + col,
                               tag | (nra_tu64)(unsigned)(int)(p ? (long long)v >> 32 : (long long)v), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    };

    int qc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) qc[i] = query_code<HAS_N>(rd, q2bit, qnmask, row_base + lane * R + i);

    cell_t Hprev[R], E[R], E2[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { Hprev[i] = NEG; E[i] = NEG; E2[i] = NEG; }
    cell_t Hbot = NEG, Fout = NEG, F2out = NEG, Hup_prev = NEG;
    cell_t best = TraceCell<W>::none;                  // score 0: only a positive score is a best cell
    int bestj = -1, besti = -1;
    int tt = NRA_PAD_T;
    int j = -lane;
    const cell_t sA = (cell_t)sp.match << SH, sB = -((cell_t)sp.mismatch << SH), sN = -((cell_t)sp.ambi << SH);
    const cell_t o1 = -((cell_t)sp.open1 << SH), x1 = -((cell_t)sp.ext1 << SH);
    const cell_t o2 = -((cell_t)sp.open2 << SH), x2 = -((cell_t)sp.ext2 << SH);

    const int nchunks = (ncols + 63 + 63) >> 6;
    for (int c = 0; c < nchunks; ++c) {
        const int col = c * 64 + lane;
        int feed = col < ncols ? tgt[col] : NRA_PAD_T;
        cell_t sH, sF, sF2;                            // lane l: what enters row 0 of the block at column c * 64 + l
        if (!fetch(col, sH, sF, sF2)) return;
#pragma unroll 1
        for (int s = 0; s < 64; ++s) {
            cell_t F = dpp_shr1(sF, Fout);             // lane 0 keeps its own sF: the column it is on
            cell_t F2 = dpp_shr1(sF2, F2out);
            tt = dpp_shr1(feed, tt);
            feed = dpp_rol1(feed);
            const cell_t fresh = (cell_t)j;
            cell_t diag = Hup_prev;
            Hup_prev = dpp_shr1(sH, Hbot);
            sH = dpp_rol1(sH); sF = dpp_rol1(sF); sF2 = dpp_rol1(sF2);
            const bool live = j >= 0 && j < ncols;
            cell_t colmax = NEG, h = NEG;
            int rowmax = 0;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const bool eq = qc[i] == tt;
                cell_t sc = eq ? sA : sB;
                if (HAS_N) {
                    if ((qc[i] | tt) & 4) sc = sN;
                }
                const cell_t d = imax(diag, fresh) + sc;
                h = imax(imax(d, E[i]), F);
                h = imax(imax(h, E2[i]), F2);
                int src = d == h ? (diag >= fresh ? T_SRC_DIAG : T_SRC_START)
                                 : (E[i] == h ? T_SRC_E : (F == h ? T_SRC_F : (E2[i] == h ? T_SRC_E2 : T_SRC_F2)));
                if (h > colmax) { colmax = h; rowmax = i; }
                diag = Hprev[i];
                Hprev[i] = h;
                const cell_t ee = E[i] + x1, eo = h + o1;
                const cell_t fe = F + x1, fo = h + o1;
                const cell_t ee2 = E2[i] + x2, eo2 = h + o2;
                const cell_t fe2 = F2 + x2, fo2 = h + o2;
                if (ee >= eo) src |= T_E_EXT;
                if (fe >= fo) src |= T_F_EXT;
                if (ee2 >= eo2) src |= T_E2_EXT;
                if (fe2 >= fo2) src |= T_F2_EXT;
                if (eq) src |= T_EQ;
                E[i] = imax(ee, eo);
                F = imax(fe, fo);
                E2[i] = imax(ee2, eo2);
                F2 = imax(fe2, fo2);
                const int row = row_base + lane * R + i;
                if (live && row < rd.qlen) tr[(size_t)row * ncols + j] = (uint8_t)src;
            }
            if (colmax > best) { best = colmax; bestj = j; besti = row_base + lane * R + rowmax; }
            Hbot = h; Fout = F; F2out = F2;
            if (lane == 63 && !last_blk && live) { publish(0, j, h); publish(1, j, F); publish(2, j, F2); }
            ++j;
        }
    }
    // wave reduce: max packed value, then smallest column, then smallest row
    cell_t vmax = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int lo = __shfl_xor((int)vmax, off, WAVE);
        cell_t o = (cell_t)lo;
        if constexpr (W) o = ((cell_t)__shfl_xor((int)(vmax >> 32), off, WAVE) << 32) | (unsigned)lo;
        vmax = imax(vmax, o);
    }
    int jm = (best == vmax) ? bestj : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) jm = imin(jm, __shfl_xor(jm, off, WAVE));
    int im = (best == vmax && bestj == jm) ? besti : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) im = imin(im, __shfl_xor(im, off, WAVE));
    if (lane == 0) {
        int32_t* o = blk_best + (size_t)(tk.blk0 + cb.blk) * 4;
        o[0] = (int)vmax; o[1] = W ? (int)((long long)vmax >> 32) : 0; o[2] = jm; o[3] = im;
    }
}

// the best cell of each pair from those of its row blocks (ascending rows): the record k_trace_fill leaves
__global__ void k_trace_best(int n_tasks, const NraTraceTask* __restrict__ tasks, const NraDevRead* __restrict__ reads,
                             int block_rows, int wide, const int32_t* __restrict__ blk_best, NraScoreParams sp,
                             int32_t* __restrict__ out)
{
    const int task = blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= n_tasks) return;
    const NraTraceTask tk = tasks[task];
    const int nblk = (reads[tk.read].qlen + block_rows - 1) / block_rows;
    long long vmax = -1;
    int jm = -1, im = -1;
    for (int b = 0; b < nblk; ++b) {
        const int32_t* p = blk_best + (size_t)(tk.blk0 + b) * 4;
        const long long v = wide ? (((long long)p[1] << 32) | (unsigned)p[0]) : (long long)p[0];
        if (v > vmax || (v == vmax && p[2] < jm)) { vmax = v; jm = p[2]; im = p[3]; }
    }
    int32_t* o = out + (size_t)task * 5;
    const int sc = (int)(vmax >> (wide ? 32 : 16));
    const int lo = sp.min_score > 1 ? sp.min_score : 1;
    if (sc >= lo && jm >= 0 && jm != 0x7fffffff) {
        o[0] = sc; o[1] = (int)(vmax & (wide ? 0xffffffffll : 0xffffll)); o[2] = jm + 1; o[3] = im; o[4] = jm;
    } else {
        o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; o[4] = -1;
    }
}

#if NRA_HAS_PART(9)
extern "C" int nra_launch_trace_fill(int R, int has_n, hipStream_t st, int n_tasks, const NraTraceTask* tasks,
                                     NraSeqArgs seq, uint8_t* trace, int32_t* out)
{
    if (n_tasks <= 0) return 0;
#define CASE(r)                                                                                     \
    case r:                                                                                         \
        if (has_n) k_trace_fill<r, true><<<n_tasks, WAVE, 0, st>>>(n_tasks, tasks, seq, trace, out); \
        else k_trace_fill<r, false><<<n_tasks, WAVE, 0, st>>>(n_tasks, tasks, seq, trace, out);      \
        break;
    switch (R) {
        NRA_R_LIST(CASE)
    default: return (int)hipErrorInvalidValue;
    }
#undef CASE
    return (int)hipGetLastError();
}

extern "C" int nra_launch_trace_back(hipStream_t st, int n_tasks, const NraTraceTask* tasks, const NraDevRead* reads,
                                     const NraDevRegion* regions, const uint8_t* trace, const int32_t* fill_out,
                                     uint8_t* ops, int32_t* out)
{
    if (n_tasks <= 0) return 0;
    k_trace_back<<<(n_tasks + 63) / 64, 64, 0, st>>>(n_tasks, tasks, reads, regions, trace, fill_out, ops, out);
    return (int)hipGetLastError();
}

// the strips and the error word belong to the call; `ticket` is zeroed here, ahead of the launch
extern "C" int nra_launch_trace_fill_mt(int R, int has_n, int wide, hipStream_t st, int n_blocks,
                                        const NraTraceBlock* blocks, int32_t* ticket, const NraTraceTask* tasks,
                                        NraSeqArgs seq, uint8_t* trace, int32_t* blk_best, uint64_t* strips,
                                        uint32_t epoch, int32_t* error)
{
    if (n_blocks <= 0) return 0;
    hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
#define ARGS n_blocks, blocks, ticket, tasks, NRA_SEQ_FIELDS(seq), trace, blk_best, (nra_tu64*)strips, epoch, error
#define CASE(r)                                                                                      \
    case r:                                                                                          \
        if (wide) { if (has_n) k_trace_fill_mt<r, true, true><<<n_blocks, WAVE, 0, st>>>(ARGS);      \
                    else k_trace_fill_mt<r, false, true><<<n_blocks, WAVE, 0, st>>>(ARGS); }         \
        else { if (has_n) k_trace_fill_mt<r, true, false><<<n_blocks, WAVE, 0, st>>>(ARGS);          \
               else k_trace_fill_mt<r, false, false><<<n_blocks, WAVE, 0, st>>>(ARGS); }             \
        break;
    switch (R) {
        NRA_TRACE_MT_R_LIST(CASE)
    default: return (int)hipErrorInvalidValue;
    }
#undef CASE
#undef ARGS
    return (int)hipGetLastError();
}

extern "C" int nra_launch_trace_best(hipStream_t st, int n_tasks, const NraTraceTask* tasks, const NraDevRead* reads,
                                     int block_rows, int wide, const int32_t* blk_best, NraScoreParams sp, int32_t* out)
{
    if (n_tasks <= 0) return 0;
    k_trace_best<<<(n_tasks + 63) / 64, 64, 0, st>>>(n_tasks, tasks, reads, block_rows, wide, blk_best, sp, out);
    return (int)hipGetLastError();
}
#endif
