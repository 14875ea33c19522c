// nra_sweep.hip -- junction decomposition of the 1D candidate bank (gfx950).
//
// The K candidates of a read, L + unit^k + R for k in [kmin,kmax], share L + unit^k as a
// prefix and R as a suffix.  An optimal local alignment of the read against candidate k
// either lies entirely in L+unit^k, or entirely in unit^k+R, or consumes R[0].  So with
//
//   B_k = best score entirely inside L + unit^k          (forward sweep, running maximum)
//   A_k = best score entirely inside unit^k + R          (reverse sweep, running maximum)
//   S_k = best score of an alignment that consumes R[0]  (junction combine, below)
//
// Score(k) = max(S_k, B_k, A_k) is the oracle's score exactly (optimal DP decomposes at a
// node column; a gap spanning the junction is handled per gap piece by refunding one open).
// Both sweeps are ONE alignment-sized DP per read instead of K:
//
//   reverse sweep (DIR 0): reversed read vs rev(R).  At its last column every lane stores H, E_in,
//     E2_in of its rows (the "R side" of the junction: best paths starting at node (i, R[0]) --
//     closed, or inside a piece-1 / piece-2 gap); the maximum over all its cells is A = the best
//     score entirely inside R.
//   forward sweep (DIR 1): read vs L + unit^kmax.  At every unit boundary L + m*k - 1 each
//     row combines its three states with the stored R side:
//        H + Hb,   E_in + Eb_in + q,   E2_in + E2b_in + q2        -> S_k
//     and the running maximum gives B_k.
//
// The origin bit.  A_k is only needed to know whether an optimal alignment STARTS at a column >= |L|,
// and that is one bit of payload: all scores are doubled and the low bit of a state says "the best
// path into this state (largest bit among co-optimal ones) starts at column >= |L|".  An
// alignment starting at column j enters through max(H(i-1,j-1), 0): the 0 becomes 0|1 for
// j >= |L| (a flag travelling with the template column), every other operation adds even
// numbers, and max() on 2*score+bit is the lexicographic max.  So the forward sweep alone
// yields (Score, bit) of S_k and B_k, the reverse sweep never needs rev(unit)^kmax, and
//   left  flank (tstart < |L|)    passes  iff  the bit of V = max(S_k, B_k, 2A+1) is 0
//                                              (oracle: the largest tstart among co-optimal paths wins)
//   right flank (tend > |L|+m*k)  passes  if  B_k < Score;  fails if B_k == Score > S_k;
//                                 B_k == S_k == Score is ambiguous -> explicit extents DP.
//
// Two kernels run these sweeps: k_sweep_ring (reads <= 3072 bases, unit <= 8 bases: two reads per wave
// in the int16 halves of every VGPR, lane-to-lane hand-off through an LDS ring, the combine on every
// m-th step) and k_sweep_pk16 (DPP hand-off: longer units; and -- CHAIN -- reads of any length as
// chained row blocks in int32 cells, one read per wave).  E is updated lazily in both (E_in of the
// current column stays in the register, which the combine needs).
#include "nra_pk16.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

// The fields of a launcher's NraSweepArgs in the order the kernels below take them (the kernels keep parameters of their
// own: NRA_SEQ_FIELDS, nra_device.h).
#define SWEEP_FIELDS(a) NRA_SEQ_FIELDS((a).seq), (a).kmin, (a).kmax, (a).coff, (a).snap, (a).read_a, (a).cand_score, (a).cand_flag

#define FLAG_BOUNDARY 0x00000080      // bit 7 of table byte 0
#define FLAG_SNAPSHOT 0x00008000      // bit 7 of table byte 1 (reverse sweep)
#define FLAG_INREP    0x80008000      // bits 7 of table bytes 1 and 3 (forward sweep, origin bit): column >= |L|

// A value parked in an accumulation register (AGPR).  A wave addresses 256 arch VGPRs; a forward sweep with
// R rows per lane wants 8R + ~35, so from R = 28 on something has to live in the 256 AGPRs.  The compiler's
// own choice costs a v_accvgpr move at every use of whatever it picked; the R side of the junction is read
// on every m-th step only, so it is parked there by hand.
__device__ __forceinline__ int agpr_put(int v) { int a; asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v)); return a; }
__device__ __forceinline__ int agpr_get(int a) { int v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; }

// selector byte of one query row for v_perm_b32: 0..3 base, 4 padding row, 5 N
template <bool HAS_N>
__device__ __forceinline__ int sweep_query_sel(const NraDevRead& rd, const uint32_t* q2bit,
                                               const uint32_t* qnmask, int gi, bool rev)
{
    if (gi >= rd.qlen) return 4;
    uint32_t b = rd.qoff + (uint32_t)(rev ? (rd.qlen - 1 - gi) : gi);
    int c = (q2bit[b >> 4] >> ((b & 15u) * 2u)) & 3u;
    if (HAS_N) {
        if ((qnmask[b >> 5] >> (b & 31u)) & 1u) c = 5;
    }
    return c;
}

// junction combine of one cell's rows at a boundary column (values biased twice).  The forward H is
// taken as it is, not as max(H, 0): a term with H < 0 is below Hb alone, an alignment inside R, and
// that is in the final maximum anyway (A, or A_k for chained reads).
template <int OFF, int N, int R, bool W = false, bool PARK = false>
__device__ __forceinline__ int sweep_combine(const int (&Hq)[R], const int (&E)[R], const int (&E2)[R],
                                             const int (&Hbo)[R], const int (&Ebo)[R],
                                             const int (&E2bo)[R], int tS)
{
    int t3_prev = 0;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int i = OFF + n;
        const int t1 = Hq[i] + (PARK ? agpr_get(Hbo[i]) : Hbo[i]);
        const int t2 = E[i] + (PARK ? agpr_get(Ebo[i]) : Ebo[i]);
        const int t3 = E2[i] + (PARK ? agpr_get(E2bo[i]) : E2bo[i]);
        tS = mx3<W>(tS, t1, t2);
        if (n & 1) tS = mx3<W>(tS, t3_prev, t3);
        else if (n == N - 1) tS = mx2<W>(tS, t3);
        else t3_prev = t3;
    }
    return tS;
}

// R side of the junction, as the reverse sweep's registers hold it (both reads packed, biased):
// per task and row block three planes [H - o1 | E_in | E2_in] of R x 64 dwords, [row of the lane][lane],
// so that every store of the reverse sweep and every load of the forward sweep is one coalesced line.
template <int OFF, int N, int R>
__device__ __forceinline__ void sweep_snapshot(const int (&Hq)[R], const int (&E)[R], const int (&E2)[R],
                                               int32_t* __restrict__ snap_blk, int lane)
{
    int32_t* p = snap_blk + lane;
    asm volatile("" : "+v"(p));    // keeps the 3N store addresses out of the step loop's registers
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int i = OFF + n;
        p[(0 * R + i) * 64] = Hq[i];
        p[(1 * R + i) * 64] = E[i];
        p[(2 * R + i) * 64] = E2[i];
    }
}

// The same for the half-wave kernel: lane-major (NRA_SNAP_LANE_STRIDE), p = the lane's own piece, 16-byte aligned.
template <int R>
__device__ __forceinline__ void sweep_snapshot_lane(const int (&Hq)[R], const int (&E)[R], const int (&E2)[R],
                                                    int32_t* __restrict__ p)
{
    constexpr int N4 = NRA_SNAP_LANE_STRIDE(R) / 4;
    int v[4 * N4];
#pragma unroll
    for (int i = 0; i < 4 * N4; ++i) v[i] = i < R ? Hq[i] : i < 2 * R ? E[i - R] : i < 3 * R ? E2[i - 2 * R] : 0;
    int4* __restrict__ p4 = reinterpret_cast<int4*>(p);
#pragma unroll
    for (int i = 0; i < N4; ++i) p4[i] = make_int4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// ------------------------------------------------------------------------------------
// fragments the sweep bodies share
// ------------------------------------------------------------------------------------
// The score constants of a sweep whose cells hold SC * score (+ payload bits in the low ones): WIDE = plain int32
// cells without a bias, otherwise the two biased int16 halves of a register.
template <int SC, bool WIDE>
struct SweepScores {
    static constexpr int BIASW = WIDE ? 0 : BIAS;
    static constexpr int P1 = WIDE ? 1 : 0x00010001;
    int o1;
    int v_floor;                          // max(H,0) - o1 (even: the payload bits are free)
    int v_o1, v_e1, v_o2, v_e2;
    int NEG1, NEG2;                       // "minus infinity", biased once / twice
    int s_match, s_mis;                   // substitution scores + o1 (the diagonal is read from Hq = H - o1): all in [0, 127]
    int tbl_hi;                           // selector 4: padding row, 5: N in the read
    int tbl_mis4, tbl_ambi4;
    __device__ __forceinline__ explicit SweepScores(const NraScoreParams& sp)
    {
        o1 = SC * sp.open1;
        const int o2 = SC * sp.open2;
        v_floor = (BIASW - o1) * P1;
        v_o1 = o1 * P1; v_e1 = SC * sp.ext1 * P1; v_o2 = o2 * P1; v_e2 = SC * sp.ext2 * P1;
        NEG1 = WIDE ? -(1 << 28) : NEGB * P1;
        NEG2 = WIDE ? -(1 << 28) : 2 * NEGB * P1;
        s_match = SC * sp.match + o1; s_mis = o1 - SC * sp.mismatch;
        const int s_ambi = o1 - SC * sp.ambi;
        tbl_hi = s_mis | (s_ambi << 8);
        tbl_mis4 = s_mis * 0x01010101; tbl_ambi4 = s_ambi * 0x01010101;
    }
};

// the substitution table (+ flags) of template column `col` of the LDS-ring sweeps; padding outside the template
template <int DIR, class Scores>
__device__ __forceinline__ int sweep_column_table(const Scores& sc, const uint8_t* __restrict__ piece, int ncols, int flank, int col)
{
    int t = sc.tbl_mis4;
    if (col >= 0 && col < ncols) {
        const int code = piece[col];
        t = code < 4 ? sc.tbl_mis4 + ((sc.s_match - sc.s_mis) << (8 * code)) : sc.tbl_ambi4;
        if (DIR == 0 && col == flank - 1) t |= FLAG_SNAPSHOT;
        if (DIR == 1 && col + 1 >= flank) t |= FLAG_INREP;         // origin bit of an alignment starting at the NEXT column
    }
    return t;
}

// One emission: Score(k) and the flank verdict of one read from the boundary accumulators S and B of its last row
// (wide, or half s2 of the packed pair) and A + 1 = a1, as (score << 2) | verdict, score -1 below min_dp_score.
template <bool WIDE>
__device__ __forceinline__ int sweep_emit(int accS, int accB, int s2, int a1, int min_score)
{
    constexpr int BIASW = WIDE ? 0 : BIAS;
    const int B = (WIDE ? accB : (s2 ? half_hi(accB) : half_lo(accB))) - BIASW;
    const int S = (WIDE ? accS : (s2 ? half_hi(accS) : half_lo(accS))) - 2 * BIASW;
    const int lo = min_score > 1 ? min_score : 1;
    // packed 2*score + origin bit; an alignment inside R starts at a column >= |L|
    const int V = imax(imax(S, B), a1);
    const int best = V >> 1;
    int flag = 1;
    if (V & 1) flag = 0;                                                  // an optimal alignment starts at >= |L|
    else if ((B >> 1) >= best) flag = ((S >> 1) >= best) ? 2 : 0;         // one ends inside L+unit^k
    return ((best >= lo ? best : -1) << 2) | flag;
}

// The candidate store.  Score(k) and the flank verdict leave through lane 63, one boundary column at a time.  They
// are collected in a lane-indexed register -- rotated one lane down per boundary, the newest value in lane 63 -- and
// written 64 candidates at a time, one coalesced line per read.
struct SweepCands {                       // a pair's windows of repeat counts and where each read's candidates start
    bool has_b;
    int kmin_a, kmax_a, kmin_b, kmax_b;
    uint32_t coff_a, coff_b;
    __device__ __forceinline__ SweepCands(int ra, int rb, bool has_b_, const int32_t* __restrict__ kmin_arr,
                                          const int32_t* __restrict__ kmax_arr, const uint32_t* __restrict__ coff)
        : has_b(has_b_), kmin_a(kmin_arr[ra]), kmax_a(kmax_arr[ra]), kmin_b(kmin_arr[rb]), kmax_b(kmax_arr[rb]),
          coff_a(coff[ra]), coff_b(coff[rb]) {}
};
// lane l holds k = kcur - 64 + l; the oldest n_valid values sit in lanes [64 - n_valid, 64); each read has its own window
__device__ __forceinline__ void sweep_flush(const SweepCands& c, int n_valid, int kcur, int lane, int out_a, int out_b,
                                            int32_t* __restrict__ cand_score, uint8_t* __restrict__ cand_flag)
{
    const int k = kcur - 64 + lane;
    if (lane < 64 - n_valid) return;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        if (s2 == 1 && !c.has_b) break;
        const int lo_k = s2 ? c.kmin_b : c.kmin_a, hi_k = s2 ? c.kmax_b : c.kmax_a;
        if (k < lo_k || k > hi_k) continue;
        const uint32_t idx = (s2 ? c.coff_b : c.coff_a) + (uint32_t)(k - lo_k);
        const int v = s2 ? out_b : out_a;
        cand_score[idx] = v >> 2;                           // (score << 2) | verdict; -1: below min_dp_score
        cand_flag[idx] = (uint8_t)(v & 3);
    }
}

// CHAIN = the WIDE sweeps: reads longer than one register block (3072 bases) are swept as consecutive row
// blocks of 64*R rows by one wave, ONE read per wave in plain int32 cells (2*score + origin bit: no range
// limit worth naming), the last cell of a block leaving its per-column hand-off in a scratch strip that
// the next block's first cell picks up.  A launch has at most as many waves as there are strips and walks
// its tasks with a grid stride.
template <int R, bool HAS_N, int DIR, bool CHAIN>
__device__ __forceinline__ void sweep_dpp_task(int task, const NraSweepTask* __restrict__ tasks,
                                               const NraDevRead* __restrict__ reads,
                                               const NraDevRegion* __restrict__ regions,
                                               const uint8_t* __restrict__ pool,
                                               const uint32_t* __restrict__ q2bit,
                                               const uint32_t* __restrict__ qnmask,
                                               const NraScoreParams& sp,
                                               const int32_t* __restrict__ kmin_arr,
                                               const int32_t* __restrict__ kmax_arr,
                                               const uint32_t* __restrict__ coff,
                                               int32_t* __restrict__ snap,
                                               int32_t* __restrict__ read_a,
                                               int32_t* __restrict__ cand_score,
                                               uint8_t* __restrict__ cand_flag,
                                               int32_t* chain_buf, int chain_cap)
{
    constexpr bool W = CHAIN;             // wide cells
    constexpr int SC = 2;                 // origin-bit scheme: doubled scores, reverse sweep over rev(R) only
    constexpr int BIASW = W ? 0 : BIAS;
    const int lane = threadIdx.x;
    const NraSweepTask tk = tasks[task];
    const bool has_b = tk.read_b >= 0;
    const int ra = tk.read_a, rb = has_b ? tk.read_b : tk.read_a;
    const NraDevRead rda = reads[ra], rdb = reads[rb];
    const NraDevRegion rg = regions[rda.region];
    const int m = rg.m1;
    const int flank = DIR ? rg.l1 : rg.l3;
    const uint8_t* __restrict__ piece = pool + (DIR ? rg.p1_off : rg.pr_off);
    const int ncols = DIR == 0 ? flank : flank + m * tk.kmax;
    // boundary column of k = kmin (>= 0: flank >= 1); the reverse sweep has one: R[0]
    const int jfirst = DIR == 0 ? flank - 1 : flank + m * tk.kmin - 1;
    const SweepCands cands(ra, rb, has_b, kmin_arr, kmax_arr, coff);
    int32_t* __restrict__ snap_task = snap + tk.snap_off;
    const SweepScores<SC, W> sc(sp);
    constexpr int P1 = SweepScores<SC, W>::P1;

    // the outputs (sweep_flush): lane 63 produces one value per boundary
    int out_a = 0, out_b = 0;
    int n_out = 0;                                          // wave-uniform: boundaries collected
    int kcur = tk.kmin;                                     // wave-uniform: k of the next boundary to leave
    auto flush = [&](int n_valid) { sweep_flush(cands, n_valid, kcur, lane, out_a, out_b, cand_score, cand_flag); };

    // CHAIN: row blocks of 64*R, one after the other in this wave; the strip belongs to the wave (blockIdx)
    const int n_blk = CHAIN ? (imax(rda.qlen, rdb.qlen) + 64 * R - 1) / (64 * R) : 1;
    volatile int32_t* strip = CHAIN ? chain_buf + (size_t)blockIdx.x * 10 * chain_cap : nullptr;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int row_base = blk * 64 * R;
    const bool first_blk = blk == 0, last_blk = blk == n_blk - 1;
    volatile int32_t* cin = CHAIN ? strip + ((blk + 1) & 1) * 5 * chain_cap : nullptr;
    volatile int32_t* cout = CHAIN ? strip + (blk & 1) * 5 * chain_cap : nullptr;

    int qc[R];       // v_perm selectors: {selA, zero, selB, zero}
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gi = row_base + lane * R + i;
        const int ca = sweep_query_sel<HAS_N>(rda, q2bit, qnmask, gi, DIR == 0);
        const int cb = W ? 0x0c : sweep_query_sel<HAS_N>(rdb, q2bit, qnmask, gi, DIR == 0);
        qc[i] = ca | (0x0c << 8) | (cb << 16) | (0x0c << 24);
    }

    // forward sweep: the R side of the junction, row r pairs with reverse-sweep row Q-2-r.  A row without
    // a partner (the read's last row, padding rows) gets "-1": its terms stay below B_k, which holds the
    // forward H of that very cell, so they never decide anything.
    int Hbo[DIR ? R : 1], Ebo[DIR ? R : 1], E2bo[DIR ? R : 1];
    if (DIR) {
        const int q1 = SC * (sp.open1 - sp.ext1), q2 = SC * (sp.open2 - sp.ext2);     // the refunded gap opens
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int r = row_base + lane * R + i;
            int h[2], e[2], e2[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int a = (s ? rdb.qlen : rda.qlen) - 2 - r;
                if (a >= 0) {
                    const int ablk = CHAIN ? a / (64 * R) : 0;
                    const int w = a - ablk * 64 * R;
                    const int al = w / R, ai = w - al * R;
                    const int32_t* __restrict__ p = snap_task + ((size_t)ablk * 3 * R + ai) * 64 + al;
                    const int vh = p[0], ve = p[R * 64], ve2 = p[2 * R * 64];
                    h[s] = (W ? vh : (s ? half_hi(vh) : half_lo(vh))) + 2 * sc.o1;    // Hq carries -o1 on either side
                    e[s] = (W ? ve : (s ? half_hi(ve) : half_lo(ve))) + q1;
                    e2[s] = (W ? ve2 : (s ? half_hi(ve2) : half_lo(ve2))) + q2;
                } else { h[s] = BIASW + sc.o1 - SC; e[s] = BIASW - SC; e2[s] = BIASW - SC; }
            }
            Hbo[i] = W ? h[0] : pack2(h[0], h[1]);
            Ebo[i] = W ? e[0] : pack2(e[0], e[1]);
            E2bo[i] = W ? e2[0] : pack2(e2[0], e2[1]);
        }
    }

    int Hq[R], Hq2[R], E[R], E2[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { Hq[i] = sc.v_floor; Hq2[i] = sc.NEG1; E[i] = sc.NEG1; E2[i] = sc.NEG1; }

    // Every lane hosts TWO virtual systolic cells -- A = its first RA rows, B = the other RB --
    // one template column apart (cell v works on column t - v, lane l hosts cells 2l and 2l+1).
    // A is fed by lane l-1's B through DPP, B by this lane's A from the previous step, so each
    // step carries two independent dependency chains per wave: the sweeps run with only a few
    // waves per SIMD and need the instruction-level parallelism.
    constexpr int RA = (R + 1) / 2, RB = R - RA;
    int HbotA = sc.v_floor, FoutA = sc.NEG1, F2outA = sc.NEG1, HupA_prev = sc.v_floor, MA = BIASW * P1;
    int HbotB = sc.v_floor, FoutB = sc.NEG1, F2outB = sc.NEG1, HupB_prev = sc.v_floor, MB = BIASW * P1;
    int accS_A = sc.NEG2, accB_A = sc.NEG1, accS_B = sc.NEG2, accB_B = sc.NEG1;
    int ttA = sc.tbl_mis4, ttB = sc.tbl_mis4;                   // padding column: everything mismatches
    n_out = 0; kcur = tk.kmin;

    // One flat step loop (128 cells deep; a chunk loop around a 64-step loop costs registers: the
    // compiler keeps the row arrays twice).  Every 64 steps the lanes fetch the next 64 columns.
    const int nsteps = ncols + 127;                       // cell 127 finishes the last column at step ncols + 126
    int feed = sc.tbl_mis4;
    // what enters cell 0 at each column: constants for the first row block, else the strip
    int inH = sc.v_floor, inF = sc.NEG1, inF2 = sc.NEG1, inS = sc.NEG2, inB = sc.NEG1;
#pragma unroll 1   // two steps per trip would turn the hand-offs into renames but cost ~14 registers
    for (int step = 0; step < nsteps; ++step) {
        {
            if ((step & 63) == 0) {
                const int col = step + lane;
                feed = sc.tbl_mis4;
                if (col < ncols) {
                    const int code = piece[col];
                    feed = code < 4 ? sc.tbl_mis4 + ((sc.s_match - sc.s_mis) << (8 * code)) : sc.tbl_ambi4;
                    if (col >= jfirst && (col - jfirst) % m == 0) feed |= FLAG_BOUNDARY;
                    if (DIR == 0 && col == flank - 1) feed |= FLAG_SNAPSHOT;
                    if (DIR == 1 && col >= flank) feed |= FLAG_INREP;
                }
                if (CHAIN) {
                    inH = sc.v_floor; inF = sc.NEG1; inF2 = sc.NEG1; inS = sc.NEG2; inB = sc.NEG1;
                    if (!first_blk && col < ncols) {
                        inH = cin[col]; inF = cin[chain_cap + col]; inF2 = cin[2 * chain_cap + col];
                        inS = cin[3 * chain_cap + col]; inB = cin[4 * chain_cap + col];
                    }
                }
            }
            // inputs of cell A: cell B of the lane above, as it stood after the previous step
            const int hupA = dpp_shr1(CHAIN ? inH : sc.v_floor, HbotB);
            int FA = dpp_shr1(CHAIN ? inF : sc.NEG1, FoutB);
            int F2A = dpp_shr1(CHAIN ? inF2 : sc.NEG1, F2outB);
            const int ttA_new = dpp_shr1(feed, ttB);      // lane 0 takes the next template column
            feed = dpp_rol1(feed);
            const int accS_Ain = dpp_shr1(CHAIN ? inS : sc.NEG2, accS_B);
            const int accB_Ain = dpp_shr1(CHAIN ? inB : sc.NEG1, accB_B);
            if (CHAIN) {
                inH = dpp_rol1(inH); inF = dpp_rol1(inF); inF2 = dpp_rol1(inF2);
                inS = dpp_rol1(inS); inB = dpp_rol1(inB);
            }
            // inputs of cell B: this lane's cell A after the previous step
            const int hupB = HbotA;
            int FB = FoutA, F2B = F2outA;
            const int ttB_new = ttA;
            const int accS_Bin = accS_A, accB_Bin = accB_A;

            // the empty alignment a path may start from at this column: score 0, origin bit from the flag
            const int floorA = DIR == 1 ? (int)((((unsigned)ttA_new >> 15) & (unsigned)P1) | (unsigned)sc.v_floor) : sc.v_floor;
            const int floorB = DIR == 1 ? (int)((((unsigned)ttB_new >> 15) & (unsigned)P1) | (unsigned)sc.v_floor) : sc.v_floor;
            sweep_cell<0, RA, R, W>(Hq, Hq2, E, E2, qc, HupA_prev, FA, F2A, MA, ttA_new & 0x7f7f7f7f, sc.tbl_hi,
                                    floorA, sc.v_e1, sc.v_e2, sc.v_o1, sc.v_o2);
            HupA_prev = hupA; HbotA = Hq[RA - 1]; FoutA = FA; F2outA = F2A;
            if (RB > 0) {
                sweep_cell<RA, RB, R, W>(Hq, Hq2, E, E2, qc, HupB_prev, FB, F2B, MB, ttB_new & 0x7f7f7f7f, sc.tbl_hi,
                                         floorB, sc.v_e1, sc.v_e2, sc.v_o1, sc.v_o2);
                HbotB = Hq[R - 1];
            } else {
                HbotB = hupB;                             // empty cell: hand everything through
            }
            HupB_prev = hupB; FoutB = FB; F2outB = F2B;
            ttA = ttA_new; ttB = ttB_new;

            const bool atA = (ttA & FLAG_BOUNDARY) != 0, atB = (ttB & FLAG_BOUNDARY) != 0;
            const unsigned long long at_mask = __builtin_amdgcn_ballot_w64(atA || atB);
            int tSA = sc.NEG2, tSB = sc.NEG2;
            if constexpr (DIR != 0) {
                if (at_mask != 0) {
                    tSA = sweep_combine<0, RA, R, W>(Hq, E, E2, Hbo, Ebo, E2bo, tSA);
                    tSB = sweep_combine<RA, RB, R, W>(Hq, E, E2, Hbo, Ebo, E2bo, tSB);
                }
            }
            accS_A = mx2<W>(accS_Ain, tSA);
            accB_A = mx2<W>(accB_Ain, MA);
            accS_B = mx2<W>(accS_Bin, tSB);
            accB_B = RB > 0 ? mx2<W>(accB_Bin, MB) : accB_Bin;  // an empty cell adds nothing of its own

            if (DIR == 0) {
                int32_t* __restrict__ snap_blk = snap_task + (size_t)blk * 3 * R * 64;
                if (ttA & FLAG_SNAPSHOT) sweep_snapshot<0, RA, R>(Hq, E, E2, snap_blk, lane);
                if (ttB & FLAG_SNAPSHOT) sweep_snapshot<RA, RB, R>(Hq, E, E2, snap_blk, lane);
            }
            if (CHAIN) {
                const int col_out = step - 127;           // the column cell 127 has just finished
                if (lane == 63 && !last_blk && col_out >= 0 && col_out < ncols) {
                    cout[col_out] = HbotB; cout[chain_cap + col_out] = FoutB; cout[2 * chain_cap + col_out] = F2outB;
                    cout[3 * chain_cap + col_out] = accS_B; cout[4 * chain_cap + col_out] = accB_B;
                }
            }
            // cell 127 (lane 63, cell B) has finished a boundary column: wave-uniform branch
            if (last_blk && (__builtin_amdgcn_ballot_w64(atB) >> 63) != 0) {
                if (DIR == 0) {
                    // the one boundary of the reverse sweep: A = best alignment inside R (doubled)
                    if (lane == 63) {
                        read_a[ra] = (W ? accB_B : half_lo(accB_B)) - BIASW;
                        if (has_b) read_a[rb] = half_hi(accB_B) - BIASW;
                    }
                } else {
                    int va = 0, vb = 0;
                    if (lane == 63) {
#pragma unroll
                        for (int s2 = 0; s2 < (W ? 1 : 2); ++s2) {
                            const int B = (W ? accB_B : (s2 ? half_hi(accB_B) : half_lo(accB_B))) - BIASW;
                            const int S = (W ? accS_B : (s2 ? half_hi(accS_B) : half_lo(accS_B))) - 2 * BIASW;
                            const int lo = sp.min_score > 1 ? sp.min_score : 1;
                            // packed 2*score + origin bit; an alignment inside R starts at a column >= |L|
                            const int V = imax(imax(S, B), read_a[s2 ? rb : ra] + 1);
                            const int best = V >> 1;
                            int flag = 1;
                            if (V & 1) flag = 0;                                  // an optimal alignment starts at >= |L|
                            else if ((B >> 1) >= best) flag = ((S >> 1) >= best) ? 2 : 0;   // one ends inside L+unit^k
                            const int v = ((best >= lo ? best : -1) << 2) | flag;
                            if (s2) vb = v; else va = v;
                        }
                    }
                    out_a = dpp_rol1(out_a); out_b = dpp_rol1(out_b);
                    if (lane == 63) { out_a = va; out_b = vb; }
                    ++kcur; ++n_out;
                    if (n_out == 64) { flush(64); n_out = 0; }
                }
            }
        }
    }
    if (DIR == 1 && last_blk && n_out > 0) flush(n_out);
  }   // row blocks
}

template <int R, bool HAS_N, int DIR, bool CHAIN>
__global__ __launch_bounds__(WAVE) void k_sweep_pk16(int n_tasks, const NraSweepTask* __restrict__ tasks,
                                                     const NraDevRead* __restrict__ reads,
                                                     const NraDevRegion* __restrict__ regions,
                                                     const uint8_t* __restrict__ pool,
                                                     const uint32_t* __restrict__ q2bit,
                                                     const uint32_t* __restrict__ qnmask,
                                                     NraScoreParams sp,
                                                     const int32_t* __restrict__ kmin_arr,
                                                     const int32_t* __restrict__ kmax_arr,
                                                     const uint32_t* __restrict__ coff,
                                                     int32_t* __restrict__ snap,
                                                     int32_t* __restrict__ read_a,
                                                     int32_t* __restrict__ cand_score,
                                                     uint8_t* __restrict__ cand_flag,
                                                     int32_t* chain_buf, int chain_cap)
{
    // unchained: one task per wave; chained: the launch has one wave per scratch strip (trip count wave-uniform)
    for (int task = blockIdx.x; task < n_tasks; task += gridDim.x)
        sweep_dpp_task<R, HAS_N, DIR, CHAIN>(task, tasks, reads, regions, pool, q2bit, qnmask, sp, kmin_arr, kmax_arr,
                                             coff, snap, read_a, cand_score, cand_flag, chain_buf, chain_cap);
}

// ------------------------------------------------------------------------------------
// k_sweep_ring: the same sweep with the lane-to-lane hand-off through an LDS ring.
//
// Lane l owns all R rows of its row block as ONE systolic cell and works on column t - skew*l at step t.
// What a cell leaves for the cell below -- H of its last row, the two vertical-gap states and the template
// column itself (its substitution table) -- is one 16-byte LDS write into the next lane's place of slot
// (t mod skew); the lane below reads it `skew` steps later (a wave's LDS operations execute in order, and
// every lane reads its place of a slot before any lane writes it again: no barrier).  Lane 63 also writes
// lane 0's place: the constants that enter row 0 and the next template column.
//
// skew = 1 for the reverse sweep.  The forward sweep uses skew = m, the unit length: then ALL lanes sit on
// a unit boundary in the same steps -- every m-th -- and the junction combine, the only work that is not
// the DP recurrence, runs under a wave-uniform branch 1/m of the time instead of on every step (with the
// 128 columns in flight of k_sweep_pk16 some lane is always on a boundary).  The per-boundary accumulators
// S and B travel through a second, one-slot LDS array on those steps only.  Price: the pipeline is 64*m
// columns deep instead of 128.  No DPP moves, one cell per lane: ~12 instead of ~35 instructions of
// per-step overhead.  (m <= SWEEP_RING_D; other regions and chained reads use k_sweep_pk16.)
//
// Measured and not kept (round 2, config 2 at 6.2 ms per step): persistent waves taking tasks from a global
// counter (1-6 waves per SIMD: 6.3-6.6 ms; the task loop keeps ~35 more registers live); issuing the
// hand-off's LDS read one step ahead (6.5 ms); a two- or three-column skew in the reverse sweep (6.6-6.7 ms);
// two or four waves (= tasks) per workgroup (6.1-6.3 ms, SWEEP_RING_WPB below).
#define SWEEP_RING_D NRA_SWEEP_RING_MAX_M
#define NRA_Q_SPIN_LIMIT (1u << 20)         // polls (~2 us each) before a waiting second part gives up: a hang guard, not a path

#ifndef SWEEP_RING_WPB
#define SWEEP_RING_WPB 1
#endif
// QUANTA (the sweeps in quanta, k_sweep_ringq): the body runs the steps [s_begin, s_end) of the sweep only.  `load`: it
// starts from the wave state another wave left in `qs` -- the lane's registers, its places of the ring and of the boundary
// accumulators, its pending outputs (lane-major 16-byte pieces) -- instead of the initial state; `store`: it leaves that state
// instead of finishing the sweep.  Cuts are multiples of 64 steps (the column tables are reloaded every 64 / 32 steps), the
// wave-uniform counters of the forward sweep follow from the step number, and a resumed wave is the uninterrupted sweep bit
// for bit (the joint prefix / tail pair works the same way).  COMB: this part of a forward sweep meets unit boundaries --
// it needs the R side's junction rows (the reverse sweep finished) and carries the combine; a part that ends before the
// first boundary step needs neither.  Without QUANTA the arguments are constants and the body is the whole sweep.
// (piece by piece, straight between the registers and memory: an array of the whole state in between costs the
// merged kernel 60 registers)
template <int R>
__device__ __forceinline__ int qstate_get(int i, const int (&Hq)[R], const int (&Hq2)[R], const int (&E)[R], const int (&E2)[R],
                                          int Hup_prev, int M)
{
    return i < R ? Hq[i] : i < 2 * R ? Hq2[i - R] : i < 3 * R ? E[i - 2 * R] : i < 4 * R ? E2[i - 3 * R] : i == 4 * R ? Hup_prev : i == 4 * R + 1 ? M : 0;
}
// (LEAN: between two runs of a step loop, where the whole wave state and the R side are live -- 8-byte pieces one at a time,
// so that what is in flight costs two registers and not thirty-two: at R = 4 two more would cost the kernel a wave)
template <int R, bool LEAN = false>
__device__ __forceinline__ void qstate_store(int32_t* __restrict__ q, const int (&Hq)[R], const int (&Hq2)[R], const int (&E)[R],
                                             const int (&E2)[R], int Hup_prev, int M, const int4* ring, const int2* racc,
                                             int out_a, int out_b, int lane)
{
    constexpr int NR = (4 * R + 2 + 3) / 4;            // 16-byte pieces of the registers; the ring's places follow, then the outputs
    if constexpr (LEAN) {
        int l = lane;
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) {
            asm volatile("" : "+v"(l));
            reinterpret_cast<int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[i] =
                make_int2(qstate_get<R>(2 * i, Hq, Hq2, E, E2, Hup_prev, M), qstate_get<R>(2 * i + 1, Hq, Hq2, E, E2, Hup_prev, M));
        }
#pragma unroll
        for (int h = 0; h < 2 * SWEEP_RING_D; ++h) {
            asm volatile("" : "+v"(l));
            reinterpret_cast<int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[2 * NR + h] =
                reinterpret_cast<const int2*>(ring + (h >> 1) * 64 + l)[h & 1];
        }
        asm volatile("" : "+v"(l));
        reinterpret_cast<int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[2 * (NR + SWEEP_RING_D)] = make_int2(out_a, out_b);
        reinterpret_cast<int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[2 * (NR + SWEEP_RING_D) + 1] = racc[l];
        return;
    }
    int4* __restrict__ q4 = reinterpret_cast<int4*>(q + (size_t)lane * NRA_QSTATE_INTS(R));
#pragma unroll
    for (int i = 0; i < NR; ++i)
        q4[i] = make_int4(qstate_get<R>(4 * i, Hq, Hq2, E, E2, Hup_prev, M), qstate_get<R>(4 * i + 1, Hq, Hq2, E, E2, Hup_prev, M),
                          qstate_get<R>(4 * i + 2, Hq, Hq2, E, E2, Hup_prev, M), qstate_get<R>(4 * i + 3, Hq, Hq2, E, E2, Hup_prev, M));
#pragma unroll
    for (int sl = 0; sl < SWEEP_RING_D; ++sl) q4[NR + sl] = ring[sl * 64 + lane];
    const int2 acc = racc[lane];
    q4[NR + SWEEP_RING_D] = make_int4(out_a, out_b, acc.x, acc.y);
}
template <int R>
__device__ __forceinline__ void qstate_load(const int32_t* __restrict__ q, int (&Hq)[R], int (&Hq2)[R], int (&E)[R], int (&E2)[R],
                                            int& Hup_prev, int& M, int4* ring, int2* racc, int& out_a, int& out_b, int lane)
{
    constexpr int NR = (4 * R + 2 + 3) / 4;
    const int4* __restrict__ q4 = reinterpret_cast<const int4*>(q + (size_t)lane * NRA_QSTATE_INTS(R));
#pragma unroll
    for (int sl = 0; sl < SWEEP_RING_D; ++sl) ring[sl * 64 + lane] = q4[NR + sl];
    const int4 o = q4[NR + SWEEP_RING_D];
    out_a = o.x; out_b = o.y;
    racc[lane] = make_int2(o.z, o.w);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int4 x = q4[i];
        const int v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * i + c;
            if (k < R) Hq[k] = v[c];
            else if (k < 2 * R) Hq2[k - R] = v[c];
            else if (k < 3 * R) E[k - 2 * R] = v[c];
            else if (k < 4 * R) E2[k - 3 * R] = v[c];
            else if (k == 4 * R) Hup_prev = v[c];
            else if (k == 4 * R + 1) M = v[c];
        }
    }
}
// The saturation check: is the wave state, bit for bit in every lane, the one `q` holds -- the words of
// qstate_store but the pending outputs?  8-byte loads, xor / or into one word per lane, one ballot.  The whole wave
// state is live here, so the pieces go one after the other, two registers in flight: each load's offset is made to
// depend on the word so far (an empty asm), or the compiler issues all loads first and keeps a hundred registers in
// flight.  tools/ringq_registers.py holds every instantiation's registers and waves against the body without the check.
template <int R>
__device__ __forceinline__ bool qstate_equal(const int32_t* __restrict__ q, const int (&Hq)[R], const int (&Hq2)[R], const int (&E)[R],
                                             const int (&E2)[R], int Hup_prev, int M, const int4* ring, const int2* racc, int lane)
{
    constexpr int NR = (4 * R + 2 + 3) / 4;
    int d = 0, l = lane;
#pragma unroll
    for (int i = 0; i < 2 * NR; ++i) {
        asm volatile("" : "+v"(l), "+v"(d));
        const int2 x = reinterpret_cast<const int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[i];
        d |= (x.x ^ qstate_get<R>(2 * i, Hq, Hq2, E, E2, Hup_prev, M)) | (x.y ^ qstate_get<R>(2 * i + 1, Hq, Hq2, E, E2, Hup_prev, M));
    }
#pragma unroll
    for (int h = 0; h < 2 * SWEEP_RING_D; ++h) {
        asm volatile("" : "+v"(l), "+v"(d));
        const int2 x = reinterpret_cast<const int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[2 * NR + h];
        const int2 y = reinterpret_cast<const int2*>(ring + (h >> 1) * 64 + l)[h & 1];
        d |= (x.x ^ y.x) | (x.y ^ y.y);
    }
    asm volatile("" : "+v"(l), "+v"(d));
    const int2 o = reinterpret_cast<const int2*>(q + (size_t)l * NRA_QSTATE_INTS(R))[2 * (NR + SWEEP_RING_D) + 1];
    const int2 acc = racc[l];
    d |= (o.x ^ acc.x) | (o.y ^ acc.y);
    return __builtin_amdgcn_ballot_w64(d != 0) == 0;
}
// the forward sweep's wave-uniform counters at step s (what the loop below would have counted up to there): boundary steps
// so far, the next repeat count lane LAG + 1 puts out, outputs waiting for their flush of W
struct SweepCounters { int bidx, kcur, n_out; };
__device__ __forceinline__ SweepCounters sweep_counters_at(int s, int jfirst, int m, int kmin, int kmax, int lag, int w)
{
    SweepCounters c;
    c.bidx = (jfirst >= 0 && s > jfirst) ? (s - 1 - jfirst) / m + 1 : 0;
    int outs = c.bidx - lag;
    if (outs < 0) outs = 0;
    if (outs > kmax - kmin + 1) outs = kmax - kmin + 1 > 0 ? kmax - kmin + 1 : 0;
    c.kcur = kmin + outs;
    c.n_out = outs % w;
    return c;
}

// The taint scheme (TAINT): cells hold 4 * score + 2 * taint + origin.  Steps [0, s_relax) of a sweep run
// the relaxed cell (nra_pk16.h), whose every value is a tainted upper bound; from step s_relax on the exact cell runs,
// seeded from the relaxed states.  s_relax = flank - c (c: the host's margin, >= 64), any step, not only a cut of the
// quanta or a start of a block of columns: the relaxed loop ends at any step, a part that straddles s_relax runs both
// loops, and slot, pcnt and the column tables go by the step number.  It is the same for every lane: lane l is exact
// from column s_relax - skew * l on.  0: no relaxed step (fewer than 64 of them: the anchor is too short).
__device__ __forceinline__ int sweep_relax_steps(int flank, int c)
{
    if (c <= 0) return 0;
    const int t = flank - (c < 64 ? 64 : c);
#if NRA_RELAX_ROUND64
    return t >= 64 ? t / 64 * 64 : 0;
#else
    return t >= 64 ? t : 0;
#endif
}
// the switch to the exact cell: E2 := E (E_r >= E1, E2), Hq2 := Hq - (o2 - o1) (H_r - o2 >= H - o2); F2 arrives as F on the ring
template <int R>
__device__ __forceinline__ void sweep_relax_switch(const int (&Hq)[R], int (&Hq2)[R], const int (&E)[R], int (&E2)[R], int v_do)
{
#pragma unroll
    for (int i = 0; i < R; ++i) { E2[i] = E[i]; Hq2[i] = Hq[i] - v_do; }
}
// the reverse sweep's junction rows: any tainted one sends the task to the exact re-sweep (the combine adds two
// biased states, and two taint bits would carry into the score)
template <int R>
__device__ __forceinline__ void sweep_rside_taint(const int (&Hq)[R], const int (&E)[R], const int (&E2)[R], int T2, int32_t* flag)
{
    int t = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) t |= Hq[i] | E[i] | E2[i];
    if (t & T2) *flag = 1;
}

// HALF: the two 32-lane halves of the wave sweep a read pair each (k_sweep_ring32).  W lanes hold a pair, hl is a lane's
// place among them and hoff the pair's first lane.  Rows, ring places and boundary accumulators are a pair's own: the
// pair's last lane hands out what enters its first.
template <int R, bool HAS_N, bool HALF, int DIR, bool COMB, bool QUANTA, bool TAINT>
__device__ __forceinline__ int sweep_ring_body(const int task, const int lane, int4* ring, int2* racc,
                                                const NraSweepTask* __restrict__ tasks,
                                                const NraDevRead* __restrict__ reads,
                                                const NraDevRegion* __restrict__ regions,
                                                const uint8_t* __restrict__ pool,
                                                const uint32_t* __restrict__ q2bit,
                                                const uint32_t* __restrict__ qnmask,
                                                NraScoreParams sp,
                                                const int32_t* __restrict__ kmin_arr,
                                                const int32_t* __restrict__ kmax_arr,
                                                const uint32_t* __restrict__ coff,
                                                int32_t* __restrict__ snap,
                                                int32_t* __restrict__ read_a,
                                                int32_t* __restrict__ cand_score,
                                                uint8_t* __restrict__ cand_flag,
                                                int32_t* __restrict__ qs, const int s_begin, const int s_end,
                                                const bool load, const bool store, const int relax_c,
                                                int32_t* __restrict__ redo, const int sat_steps = -1)
{
    static_assert(DIR == 1 || !COMB, "only a forward sweep meets unit boundaries");
    constexpr bool SAT = NRA_SAT_EXIT != 0 && QUANTA && COMB;     // the saturation exit (below); sat_steps < 0: off
    constexpr int SAT_NEVER = 0x7fffffff;
    constexpr int SC = TAINT ? 4 : 2;     // origin-bit scheme: doubled scores; TAINT: 4 * score + 2 * taint + origin
    constexpr int W = HALF ? 32 : 64;
    const int hoff = HALF ? lane & 32 : 0;
    const int hl = HALF ? lane & 31 : lane;
    const NraSweepTask tk = tasks[task];
    // the upper half's own pair (a half without reads repeats pair a/b and stores nothing)
    const bool half_on = hoff == 0 || tk.read_c >= 0;
    const int r0 = (hoff && tk.read_c >= 0) ? tk.read_c : tk.read_a;
    const int r1 = (hoff && tk.read_c >= 0) ? tk.read_d : tk.read_b;
    const bool has_b = r1 >= 0;
    const int ra = r0, rb = has_b ? r1 : r0;
    const NraDevRead rda = reads[ra], rdb = reads[rb];
    const NraDevRegion rg = regions[HALF ? reads[tk.read_a].region : rda.region];
    const int m = rg.m1;
    const int flank = DIR ? rg.l1 : rg.l3;
    const uint8_t* __restrict__ piece = pool + (DIR ? rg.p1_off : rg.pr_off);
    const int ncols = DIR ? flank + m * tk.kmax : flank;
    const int jfirst = DIR ? flank + m * tk.kmin - 1 : flank - 1;     // boundary column of k = kmin
    const int skew = DIR ? m : 1;
    const int kmin_a = kmin_arr[ra], kmax_a = kmax_arr[ra];
    const int kmin_b = kmin_arr[rb], kmax_b = kmax_arr[rb];
    const uint32_t coff_a = coff[ra], coff_b = coff[rb];
    int32_t* __restrict__ snap_task = snap + tk.snap_off;
    const SweepScores<SC, false> sc(sp);
    constexpr int P1 = SweepScores<SC, false>::P1;
    // the taint scheme: the steps [0, s_relax) run the relaxed cell; T2 = the taint bit of both halves
    const int s_relax = TAINT ? sweep_relax_steps(flank, relax_c) : 0;
    const int T2 = 2 * P1;
    constexpr int SH = TAINT ? 2 : 1;     // score = state >> SH

    auto column_table = [&](int col) { return sweep_column_table<DIR>(sc, piece, ncols, flank, col); };

    // outputs: lane W - 1 of a pair produces one value per boundary; the pair keeps its last W in a lane-indexed register
    // (rotated within the pair) and writes them W candidates at a time
    int out_a = 0, out_b = 0;
    int n_out = 0, kcur = tk.kmin;                          // wave-uniform
    const int rot_src = HALF ? (hoff | ((hl + 1) & 31)) << 2 : 0;      // ds_bpermute address: the next lane of the half
    auto flush = [&](int n_valid) {
        const int k = kcur - W + hl;
        if (hl < W - n_valid || !half_on) return;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if (s2 == 1 && !has_b) break;
            const int lo_k = s2 ? kmin_b : kmin_a, hi_k = s2 ? kmax_b : kmax_a;
            if (k < lo_k || k > hi_k) continue;
            const uint32_t idx = (s2 ? coff_b : coff_a) + (uint32_t)(k - lo_k);
            const int v = s2 ? out_b : out_a;
            cand_score[idx] = v >> 2;
            cand_flag[idx] = (uint8_t)(v & 3);
        }
    };

    int qc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gi = hl * R + i;
        const int ca = sweep_query_sel<HAS_N>(rda, q2bit, qnmask, gi, DIR == 0);
        const int cb = sweep_query_sel<HAS_N>(rdb, q2bit, qnmask, gi, DIR == 0);
        qc[i] = ca | (0x0c << 8) | (cb << 16) | (0x0c << 24);
    }
    constexpr bool PARK = R >= 28;        // the R side of the junction in AGPRs
    int Hbo[COMB ? R : 1], Ebo[COMB ? R : 1], E2bo[COMB ? R : 1];
    if (COMB) {
        const int q1 = SC * (sp.open1 - sp.ext1), q2 = SC * (sp.open2 - sp.ext2);
        // the R side as the reverse sweep stored it: [row][lane] planes (sweep_snapshot) or lane-major (sweep_snapshot_lane)
        constexpr int PL = HALF ? R : R * 64;               // from H to E to E2
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int r = hl * R + i;
            int h[2], e[2], e2[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int a = (s ? rdb.qlen : rda.qlen) - 2 - r;
                if (a >= 0) {
                    const int al = a / R, ai = a - al * R;      // reverse-sweep row a sits in lane al of the pair
                    const int32_t* __restrict__ p = HALF ? snap_task + (size_t)(hoff + al) * NRA_SNAP_LANE_STRIDE(R) + ai
                                                         : snap_task + (size_t)ai * 64 + al;
                    const int vh = p[0], ve = p[PL], ve2 = p[2 * PL];
                    h[s] = (s ? half_hi(vh) : half_lo(vh)) + 2 * sc.o1;
                    e[s] = (s ? half_hi(ve) : half_lo(ve)) + q1;
                    e2[s] = (s ? half_hi(ve2) : half_lo(ve2)) + q2;
                } else { h[s] = BIAS + sc.o1 - SC; e[s] = BIAS - SC; e2[s] = BIAS - SC; }
            }
            Hbo[i] = PARK ? agpr_put(pack2(h[0], h[1])) : pack2(h[0], h[1]);
            Ebo[i] = PARK ? agpr_put(pack2(e[0], e[1])) : pack2(e[0], e[1]);
            E2bo[i] = PARK ? agpr_put(pack2(e2[0], e2[1])) : pack2(e2[0], e2[1]);
        }
    }
    int Hq[R], Hq2[R], E[R], E2[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { Hq[i] = s_relax > 0 ? sc.v_floor | T2 : sc.v_floor; Hq2[i] = sc.NEG1; E[i] = sc.NEG1; E2[i] = sc.NEG1; }

    // ring: padding columns everywhere, then the first lane's first `skew` columns
#pragma unroll
    for (int s = 0; s < SWEEP_RING_D; ++s) ring[s * 64 + lane] = make_int4(sc.v_floor, sc.NEG1, sc.NEG1, sc.tbl_mis4);
    racc[lane] = make_int2(sc.NEG2, sc.NEG1);
    if (hl < skew) ring[hl * 64 + hoff] = make_int4(sc.v_floor, sc.NEG1, sc.NEG1, column_table(hl));
    ring_order();

    int Hup_prev = s_relax > 0 ? sc.v_floor | T2 : sc.v_floor, M = BIAS * P1;      // (tainted, as Hq: the diagonal into row 0)
    int feed = sc.tbl_mis4;
    const int nsteps = ncols + (W - 1) * skew;              // lane W - 1 finishes the last column at step ncols - 1 + (W - 1)*skew
    const int nx = (hl + 1) & (W - 1);
    const int wr = hoff | nx;
    const int s0 = QUANTA ? s_begin : 0, s1 = QUANTA ? (s_end < nsteps ? s_end : nsteps) : nsteps;
    if (QUANTA && load) {
        qstate_load<R>(qs, Hq, Hq2, E, E2, Hup_prev, M, ring, racc, out_a, out_b, lane);
        ring_order();
        const SweepCounters c = sweep_counters_at(s0, jfirst, m, tk.kmin, tk.kmax, W - 1, W);
        kcur = c.kcur; n_out = c.n_out;
    }
    int slot = QUANTA ? s0 % skew : 0;                      // step mod skew
    // A (best alignment inside R, doubled) of the two reads: written by the reverse sweep, constant here
    const int a_of_a = COMB ? read_a[ra] : 0, a_of_b = COMB ? read_a[rb] : 0;
    int phase = jfirst % m;                                 // boundary steps: step mod m == phase, step >= jfirst
    int pcnt = QUANTA ? s0 % m : 0;                         // step mod m
    int bidx = QUANTA ? sweep_counters_at(s0, jfirst, m, tk.kmin, tk.kmax, W - 1, W).bidx : 0;      // boundary steps so far
    int sx = s0;                                            // the first step of the exact cell
    if (TAINT && s0 < s_relax) {
        // the relaxed steps: columns of the anchor far from the junction (no boundary, snapshot or table flag among
        // them: s_relax <= flank - 64); one gap state per direction, F in both places of the hand-off
        sx = s1 < s_relax ? s1 : s_relax;
        const int flr = BIAS * P1 | T2, hfl = flr - sc.v_o1, v_er = SC * imin(sp.ext1, sp.ext2) * P1;
#pragma unroll 1
        for (int step = s0; step < sx; ++step) {
            if ((step & (W - 1)) == 0) feed = column_table(step + skew + nx);
            const int4 in = ring[slot * 64 + lane];
            int F = pmaxi(in.y, flr);
            sweep_cell_relaxed<R>(Hq, E, qc, Hup_prev, F, M, in.w, sc.tbl_hi, flr, v_er, sc.v_o1);
            Hup_prev = pmaxi(in.x, hfl);
            ring[slot * 64 + wr] = make_int4(Hq[R - 1], F, F, in.w);
            if (hl == W - 1) ring[slot * 64 + hoff] = make_int4(sc.v_floor, sc.NEG1, sc.NEG1, feed);
            ring_order();
            feed = dpp_rol1(feed);
            if (++slot == skew) slot = 0;
        }
        pcnt = sx % m;
    }
    if (TAINT && sx == s_relax && sx < s1) sweep_relax_switch<R>(Hq, Hq2, E, E2, sc.v_o2 - sc.v_o1);
    // The saturation exit (SAT).  The wave is a deterministic machine whose only input, the column tables
    // lane W - 1 hands out, has period m between the columns |L| and ncols.  If its state at the top of step b + m is
    // the state at the top of step b (the `base`) bit for bit -- registers, ring places, boundary accumulators, the
    // running maximum among them --, every later state repeats with period m, and every repeat count still to leave
    // gets the value of the last emission: the sweep ends here (behind the loop).  A base is the state this part
    // loaded (still in `qs`) or, every sat_steps steps, a checkpoint stored there (the slot is free between this
    // part's load and its store), and with them the last base there is, ncols - 2 m, so that a sweep whose state
    // repeats at all leaves somewhere.  Bases, all wave-uniform: lane W - 1 inside the repeat (b >= |L| + (W - 1) m), an
    // emission in (b, b + m] (b + m > the step of the first one), every column held or handed out in both windows
    // below ncols (b + 2 m <= ncols), and the compare inside this part with a step left to skip.
    int sat_evt = SAT_NEVER, sat_skip = 0;                  // the step of the next event; steps skipped on exit
    bool sat_cmp = false;                                   // the next event compares (else: stores a checkpoint)
    const int sat_every = sat_steps > 0 ? imax(sat_steps, 64) : 0;
    const int sat_hi = imin(ncols - 2 * m, s1 - 1 - m);     // the last base worth having
    auto sat_next = [&](int from) {                         // the first base at or behind step `from` (> s0)
        int b = SAT_NEVER;
        if (sat_every > 0) {
            b = s0 + imax(1, (from - s0 + sat_every - 1) / sat_every) * sat_every;
            if (ncols - 2 * m >= from && ncols - 2 * m < b) b = ncols - 2 * m;
        }
        return b <= sat_hi ? b : SAT_NEVER;
    };
    if (SAT && sat_steps >= 0) {
        const int sat_lo = imax(flank, jfirst + 1 - m) + (W - 1) * m;
        if (load && sx == s0 && s0 >= sat_lo && s0 <= sat_hi) { sat_evt = s0 + m; sat_cmp = true; }
        else sat_evt = sat_next(imax(sat_lo, sx + 1));
    }
    // (the events sit between runs of the step loop, not in it: the loop is the one of a body without the check)
    for (int s_from = sx;;) {
      const int s_to = SAT ? imin(s1, sat_evt) : s1;
#pragma unroll 1
    for (int step = s_from; step < s_to; ++step) {
        // lane W - 1 hands out column step + skew.  (Both halves sweep the same template: the column tables repeat
        // with period 32 across the wave, and a full-wave rotation keeps them so.)
        if ((step & (W - 1)) == 0) feed = column_table(step + skew + nx);
        const int4 in = ring[slot * 64 + lane];
        const int tt = in.w;
        // the floor lives in F (sweep_cell, FF): score 0 with the origin bit of the next column.  What enters a
        // lane's first row is at the floor already, but for a pair's first lane, which takes constants: one max each
        const int fl = DIR == 1 ? (int)((((unsigned)tt >> 15) & (unsigned)P1) | (unsigned)(BIAS * P1)) : BIAS * P1;
        int F = pmaxi(in.y, fl), F2 = in.z;
        sweep_cell<0, R, R, false, true>(Hq, Hq2, E, E2, qc, Hup_prev, F, F2, M, tt & 0x7f7f7f7f, sc.tbl_hi, fl, sc.v_e1, sc.v_e2, sc.v_o1, sc.v_o2);
        Hup_prev = pmaxi(in.x, fl - sc.v_o1);
        ring[slot * 64 + wr] = make_int4(Hq[R - 1], F, F2, tt);
        if (hl == W - 1) ring[slot * 64 + hoff] = make_int4(sc.v_floor, sc.NEG1, sc.NEG1, feed);
        ring_order();                                       // the next steps' loads stay behind these stores
        feed = dpp_rol1(feed);
        if (++slot == skew) slot = 0;

        if constexpr (DIR == 0) {
            if (tt & FLAG_SNAPSHOT) {
                if constexpr (HALF) sweep_snapshot_lane<R>(Hq, E, E2, snap_task + (size_t)lane * NRA_SNAP_LANE_STRIDE(R));
                else sweep_snapshot<0, R, R>(Hq, E, E2, snap_task, lane);
                if (TAINT) sweep_rside_taint<R>(Hq, E, E2, T2, redo + task);
            }
        } else if constexpr (COMB) {
            if (pcnt == phase && step >= jfirst) {          // every lane is on a unit boundary: wave-uniform
                const int tS = sweep_combine<0, R, R, false, PARK>(Hq, E, E2, Hbo, Ebo, E2bo, sc.NEG2);
                const int2 acc = racc[lane];
                const int accS = pmaxi(acc.x, tS), accB = pmaxi(acc.y, M);
                racc[wr] = make_int2(accS, accB);
                if (hl == W - 1) racc[hoff] = make_int2(sc.NEG2, sc.NEG1);
                ring_order();
                if (bidx >= W - 1 && kcur <= tk.kmax) {     // lane W - 1 of each pair is on the boundary of k = kcur
                    int va = 0, vb = 0;
                    if (hl == W - 1) {
#pragma unroll
                        for (int s2 = 0; s2 < 2; ++s2) {
                            const int B = (s2 ? half_hi(accB) : half_lo(accB)) - BIAS;
                            const int S = (s2 ? half_hi(accS) : half_lo(accS)) - 2 * BIAS;
                            const int lo = sp.min_score > 1 ? sp.min_score : 1;
                            // packed 2*score + origin bit; an alignment inside R starts at a column >= |L|
                            const int V = imax(imax(S, B), (s2 ? a_of_b : a_of_a) + 1);
                            const int best = V >> SH;
                            int flag = 1;
                            if (V & 1) flag = 0;                                  // an optimal alignment starts at >= |L|
                            else if ((B >> SH) >= best) flag = ((S >> SH) >= best) ? 2 : 0;
                            if (TAINT && (V & 2)) redo[task] = 1;                 // a relaxed cell is on a winning path
                            const int v = ((best >= lo ? best : -1) << 2) | flag;
                            if (s2) vb = v; else va = v;
                        }
                    }
                    if constexpr (HALF) {                   // within the half: through the LDS crossbar
                        out_a = __builtin_amdgcn_ds_bpermute(rot_src, out_a);
                        out_b = __builtin_amdgcn_ds_bpermute(rot_src, out_b);
                    } else {
                        out_a = dpp_rol1(out_a); out_b = dpp_rol1(out_b);
                    }
                    if (hl == W - 1) { out_a = va; out_b = vb; }
                    ++kcur; ++n_out;
                    if (n_out == W) { flush(W); n_out = 0; }
                }
                ++bidx;
            }
            if (++pcnt == m) pcnt = 0;
        }
    }
      if (!SAT || s_to >= s1) break;
      if (sat_cmp) {
          if (qstate_equal<R>(qs, Hq, Hq2, E, E2, Hup_prev, M, ring, racc, lane)) { sat_skip = nsteps - s_to; break; }
          sat_evt = sat_next(s_to);
          sat_cmp = false;
      } else {
          qstate_store<R, true>(qs, Hq, Hq2, E, E2, Hup_prev, M, ring, racc, out_a, out_b, lane);
          sat_evt = s_to + m; sat_cmp = true;
      }
      s_from = s_to;
    }
    if (SAT && sat_skip > 0) {
        // the exit: the pending outputs as `flush` writes them, then the last emission -- it sits in lane W - 1 of each
        // pair, the outputs rotate on emissions only -- for every repeat count from kcur on, through the same per-read
        // window filter, W candidates per store: this family keeps writing every candidate (NRA_LEAN_CLEARS).  The
        // repeated value raised redo[task] when it was emitted, if it is tainted.
        const int va = __builtin_amdgcn_ds_bpermute((hoff | (W - 1)) << 2, out_a);
        const int vb = __builtin_amdgcn_ds_bpermute((hoff | (W - 1)) << 2, out_b);
        if (n_out > 0) flush(n_out);
        for (int k = kcur + hl; k <= tk.kmax && half_on; k += W) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (s2 == 1 && !has_b) break;
                const int lo_k = s2 ? kmin_b : kmin_a, hi_k = s2 ? kmax_b : kmax_a;
                if (k < lo_k || k > hi_k) continue;
                const uint32_t idx = (s2 ? coff_b : coff_a) + (uint32_t)(k - lo_k);
                const int v = s2 ? vb : va;
                cand_score[idx] = v >> 2;
                cand_flag[idx] = (uint8_t)(v & 3);
            }
        }
        return sat_skip;
    }
    if (QUANTA && store) {
        qstate_store<R>(qs, Hq, Hq2, E, E2, Hup_prev, M, ring, racc, out_a, out_b, lane);
    } else if (DIR == 0) {
        // the short reverse sweep ends on its one boundary, R[0]: A = best alignment inside R (doubled)
        // = the maximum over every cell of the pair's sweep
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) M = pmaxi(M, __shfl_xor(M, off, 64));
        if (hl == 0 && half_on) {
            read_a[ra] = half_lo(M) - BIAS;
            if (has_b) read_a[rb] = half_hi(M) - BIAS;
        }
    } else if (COMB && n_out > 0) {
        flush(n_out);
    }
    return 0;
}

// relax_c, redo: TAINT -- the margin c of the relaxed steps, and the per-task flags the sweep sets where a relaxed cell
// may have reached an output; otherwise, redo non-null: the exact re-sweep of the flagged tasks only (the others leave)
template <int R, bool HAS_N, int DIR, bool TAINT>
__global__ __launch_bounds__(WAVE * SWEEP_RING_WPB) void k_sweep_ring(int n_tasks, const NraSweepTask* __restrict__ tasks,
                                                     const NraDevRead* __restrict__ reads,
                                                     const NraDevRegion* __restrict__ regions,
                                                     const uint8_t* __restrict__ pool,
                                                     const uint32_t* __restrict__ q2bit,
                                                     const uint32_t* __restrict__ qnmask,
                                                     NraScoreParams sp,
                                                     const int32_t* __restrict__ kmin_arr,
                                                     const int32_t* __restrict__ kmax_arr,
                                                     const uint32_t* __restrict__ coff,
                                                     int32_t* __restrict__ snap,
                                                     int32_t* __restrict__ read_a,
                                                     int32_t* __restrict__ cand_score,
                                                     uint8_t* __restrict__ cand_flag, int relax_c, int32_t* __restrict__ redo)
{
    __shared__ int4 ring_all[SWEEP_RING_WPB * SWEEP_RING_D * 64];
    __shared__ int2 racc_all[SWEEP_RING_WPB * 64];
    // (with one wave per block everything below is a constant: LDS addresses stay immediates)
    const int wave_in_block = SWEEP_RING_WPB > 1 ? (int)(threadIdx.x >> 6) : 0;
    int4* ring = ring_all + wave_in_block * SWEEP_RING_D * 64;
    int2* racc = racc_all + wave_in_block * 64;
    const int task = blockIdx.x * SWEEP_RING_WPB + wave_in_block;
    if (task >= n_tasks) return;
    if (!TAINT && redo && redo[task] == 0) return;
    const int lane = SWEEP_RING_WPB > 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    sweep_ring_body<R, HAS_N, false, DIR, DIR == 1, false, TAINT>(task, lane, ring, racc, tasks, reads, regions, pool, q2bit, qnmask, sp,
                                                                  kmin_arr, kmax_arr, coff, snap, read_a, cand_score, cand_flag, nullptr, 0,
                                                                  0, false, false, relax_c, redo);
}

// ------------------------------------------------------------------------------------
// k_sweep_ring32: the LDS-ring sweep with TWO read pairs of one region per wave, 32 lanes each.
//
// Most real cores are a few hundred bases: k_sweep_ring then has 3 to 8 rows per lane, and what does not
// depend on the rows -- the ~12 instructions of per-step overhead, the 63*skew columns of pipeline fill --
// is a quarter of the work.  Here a pair occupies half a wave (rows = 32 * R): the two halves run the same
// template (same region, the union of the four reads' windows) in lock step, each with its own ring
// (lane 31 hands out what enters lane 0, lane 63 what enters lane 32), so the overhead is paid once for four
// reads and the pipeline is 32*skew columns deep.
template <int R, bool HAS_N, int DIR, bool TAINT>                     // relax_c, redo as in k_sweep_ring
__global__ __launch_bounds__(WAVE) void k_sweep_ring32(int n_tasks, const NraSweepTask* __restrict__ tasks,
                                                       const NraDevRead* __restrict__ reads,
                                                       const NraDevRegion* __restrict__ regions,
                                                       const uint8_t* __restrict__ pool,
                                                       const uint32_t* __restrict__ q2bit,
                                                       const uint32_t* __restrict__ qnmask,
                                                       NraScoreParams sp,
                                                       const int32_t* __restrict__ kmin_arr,
                                                       const int32_t* __restrict__ kmax_arr,
                                                       const uint32_t* __restrict__ coff,
                                                       int32_t* __restrict__ snap,
                                                       int32_t* __restrict__ read_a,
                                                       int32_t* __restrict__ cand_score,
                                                       uint8_t* __restrict__ cand_flag, int relax_c, int32_t* __restrict__ redo)
{
    __shared__ int4 ring[SWEEP_RING_D * 64];
    __shared__ int2 racc[64];
    const int task = blockIdx.x;
    if (task >= n_tasks) return;
    if (!TAINT && redo && redo[task] == 0) return;
    sweep_ring_body<R, HAS_N, true, DIR, DIR == 1, false, TAINT>(task, (int)threadIdx.x, ring, racc, tasks, reads, regions, pool, q2bit,
                                                                 qnmask, sp, kmin_arr, kmax_arr, coff, snap, read_a, cand_score, cand_flag,
                                                                 nullptr, 0, 0, false, false, relax_c, redo);
}

// ------------------------------------------------------------------------------------
// k_sweep_ringq: a bucket's reverse and forward sweeps as ONE launch of quanta taken by ticket.
//
// Two launches per bucket (all reverse sweeps, then all forward sweeps) made kernel-length tasks: 3750 waves of 1000 - 2300
// steps on 1024 SIMDs ended with a tail of SIMDs holding 3 or 4 of them (12 - 14 % of a config-2 step), and no forward
// sweep could start before the last reverse sweep of its bucket was over.  Here a sweep is cut every `qsteps` steps (a
// multiple of 64; the host picks it; a forward sweep also at the last multiple of 64 at or before its first boundary
// step) into parts -- quanta of a few hundred steps -- and a wave takes ONE by ticket (an
// atomic add when it starts) from a list the host orders [reverse parts 0 of every task | reverse parts 1 | ... | forward
// parts 0 | forward parts 1 | ...]:
//   * part p of a sweep waits for part p - 1 (it resumes from the state that one left), and a forward part that reaches
//     the first boundary step also for the task's whole reverse sweep (the junction rows, A): two counters per task count
//     the finished parts of either direction; bounded spin with s_sleep, a launch-wide give-up word like k_sweep_ringmt's.
//     Every producer holds a smaller ticket, so it was taken by a wave that has started: running or done, whatever order
//     the workgroups are dispatched in -- no deadlock as long as started waves stay resident;
//   * producers publish with an agent-scope release fence before the arrival, the consumer acquires after the poll
//     (cdna_hip_programming.md Guideline 16: plain payload, atomic flag, fences on both sides);
//   * a cut costs no step: the dumped state is the skewed wave state, the pipeline is not drained.
// A forward part that ends before the first boundary step (the columns of L) runs the plain body: no junction input, no combine.
// (the body inlined: as a real function call -- noinline -- it costs the calling convention's register reserve: 248 at R = 15)

// (waves per SIMD as the forward sweep alone: without the hint the merged body takes 226 registers at R = 15 where
// k_sweep_ring's forward sweep takes 156; with it 168 and a few spilled values in the prologues -- the R side's
// constants while the state is loaded --, none in a step loop)
// (A hint the kernel cannot meet is no target at all: the half-wave body at R = 5, asked for 6 waves, sits at 126
// registers, two below the fourth wave's limit, and drifted to 130 - 132 with the saturation events around its step loop;
// asked for the 4 it can have it takes 124.  tools/ringq_registers.py compares every instantiation with the body without
// the events.)
constexpr int ringq_waves(int R, bool half)
{
    if (half && R == 5) return 4;
    const int w = 512 / (9 * R + 30);
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}

template <int R, bool HAS_N, bool HALF, bool TAINT>                  // relax_c, redo: TAINT as in k_sweep_ring
__global__ __launch_bounds__(WAVE, ringq_waves(R, HALF)) void k_sweep_ringq(int n_quanta, const uint32_t* __restrict__ qlist, int qsteps, int n_tasks,
                                                      int32_t* ticket, int32_t* arrivals, int32_t* giveup,
                                                      int32_t* __restrict__ qstate,
                                                      const NraSweepTask* __restrict__ tasks,
                                                      const NraDevRead* __restrict__ reads,
                                                      const NraDevRegion* __restrict__ regions,
                                                      const uint8_t* __restrict__ pool,
                                                      const uint32_t* __restrict__ q2bit,
                                                      const uint32_t* __restrict__ qnmask,
                                                      NraScoreParams sp,
                                                      const int32_t* __restrict__ kmin_arr,
                                                      const int32_t* __restrict__ kmax_arr,
                                                      const uint32_t* __restrict__ coff,
                                                      int32_t* __restrict__ snap,
                                                      int32_t* __restrict__ read_a,
                                                      int32_t* __restrict__ cand_score,
                                                      uint8_t* __restrict__ cand_flag, int relax_c, int32_t* __restrict__ redo,
                                                      int sat_steps, int32_t* sat_count)
{
    __shared__ int4 ring[SWEEP_RING_D * 64];
    __shared__ int2 racc[64];
    const int lane = threadIdx.x;
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= n_quanta) return;
    // a quantum: direction << 31 | part << NRA_Q_PART_SHIFT | task (NRA_Q_* in nra_internal.h, with the step counts the host
    // lists the parts by)
    const uint32_t q = qlist[t];
    const int dir = (int)(q >> 31), part = (int)((q >> NRA_Q_PART_SHIFT) & NRA_Q_PART_MASK), task = (int)(q & NRA_Q_TASK_MASK);
    const NraSweepTask tk = tasks[task];
    const NraDevRegion rg = regions[reads[tk.read_a].region];
    const int nsteps_rev = NRA_Q_STEPS_REV(rg.l3, HALF), nsteps_fwd = NRA_Q_STEPS_FWD(rg.l1, rg.m1, tk.kmax, HALF);
    const int jfirst = rg.l1 + rg.m1 * tk.kmin - 1;                 // the first boundary step of the forward sweep
    // a forward sweep is cut at NRA_Q_CUT(jfirst) first -- the last multiple of 64 steps at or before the first boundary
    // step: the parts before it are plain -- and every `qsteps` steps on either side of that cut; a reverse sweep every `qsteps`
    const int s_cut = dir ? NRA_Q_CUT(jfirst) : 0;
    const int n_plain = (s_cut + qsteps - 1) / qsteps;
    const bool comb = dir && part >= n_plain;
    const int s_begin = comb ? s_cut + (part - n_plain) * qsteps : part * qsteps;
    const int s_end = (!comb && dir && s_begin + qsteps > s_cut) ? s_cut : s_begin + qsteps;
    const bool load = part > 0, store = s_end < (dir ? nsteps_fwd : nsteps_rev);
    const int need_rev = comb ? (nsteps_rev + qsteps - 1) / qsteps : 0;
    int32_t* mine = arrivals + 2 * (size_t)task + dir;
    const int32_t* rev = arrivals + 2 * (size_t)task;
    if (load || comb) {
        bool finished = false;
        for (unsigned spins = 0;; ++spins) {
            int ok = 0;                                     // 2: the sweep is over (NRA_Q_FINISHED)
            if (lane == 0) {
                const int before = load ? __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                ok = before >= NRA_Q_FINISHED ? 2
                   : before >= part && (!comb || __hip_atomic_load(rev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need_rev);
            }
            ok = __builtin_amdgcn_readfirstlane(ok);
            if (ok) { finished = ok == 2; break; }
            __builtin_amdgcn_s_sleep(64);
            if ((spins & 15) == 15) {
                int failed = 0;
                if (lane == 0) failed = __hip_atomic_load(giveup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane(failed) != 0) return;
                if (spins >= NRA_Q_SPIN_LIMIT) {
                    if (lane == 0) __hip_atomic_store(giveup, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return;
                }
            }
        }
        // the sweep left through the saturation exit in an earlier part: nothing to load, no arrival to add
        if (finished) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    // a slot per forward sweep, then -- where a reverse sweep has more than one part -- one per reverse sweep
    int32_t* __restrict__ qs = qstate + ((size_t)(dir ? 0 : n_tasks) + (size_t)task) * (NRA_QSTATE_INTS(R) * 64);
#define NRA_Q_ARGS task, lane, ring, racc, tasks, reads, regions, pool, q2bit, qnmask, sp, kmin_arr, kmax_arr, coff, snap, read_a, cand_score, cand_flag, qs, s_begin, s_end, load, store, relax_c, redo
    int skipped = 0;                                        // wave-uniform: steps the saturation exit left out
    if (!dir) sweep_ring_body<R, HAS_N, HALF, 0, false, true, TAINT>(NRA_Q_ARGS);
    else if (!comb) sweep_ring_body<R, HAS_N, HALF, 1, false, true, TAINT>(NRA_Q_ARGS);
    else skipped = sweep_ring_body<R, HAS_N, HALF, 1, true, true, TAINT>(NRA_Q_ARGS, sat_steps);
#undef NRA_Q_ARGS
    // everything this wave stored -- the wave state at the cut, or the R side's snapshot and A -- before the arrival
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
        if (skipped > 0) {
            // the sweep is over: a value no count of parts reaches tells its later parts to leave (the poll above)
            __hip_atomic_store(mine, NRA_Q_FINISHED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(sat_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // (the steps in 64 bits: 8192 sweeps of a few hundred thousand steps each would pass 2^31)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(sat_count + 2), (unsigned long long)skipped, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        } else {
            __hip_atomic_fetch_add(mine, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ------------------------------------------------------------------------------------
// The chained LDS-ring sweeps: reads of more than NRA_RING_CHAIN_MIN_ROWS rows as row blocks of 64*R rows.
//
// k_sweep_ring keeps all rows of a read pair in the registers of one wave: from 28 rows per lane on that is one
// wave per SIMD.  Here the rows are swept as consecutive blocks of 64*R rows, which fit three waves to a SIMD: what
// lane 63 leaves per column -- H of the block's last row, the two vertical-gap states and, on boundary columns, the
// S and B accumulators -- goes to a strip that the next block's lane 0 picks up (lane 63 feeds lane 0's ring slot
// anyway: it hands out the strip's values together with the template column).  W = false: two reads per wave in
// packed int16 (doubled scores up to 27000); W = true: one read per wave in int32 cells, any length.
//
// sweep_rowblock_body is the sweep of ONE row block.  Two kernels run it: k_sweep_ringchain, the blocks of a task one
// after the other in one wave, and k_sweep_ringmt, every block a wave of its own.  They differ in the hand-off between
// two blocks only, the body's `Link`:
//   bool fetch(col, at_boundary, h, f, f2, s, b)   what the block above left at column `col` (each lane its own; col < 0:
//                                                  nothing, the arguments stay as they are; s and b only at_boundary);
//                                                  wave-uniform control flow, false when the launch has failed
//   void publish(plane, col, v)                    plane 0..4 (H, F, F2, S, B) of column `col` for the block below
// ------------------------------------------------------------------------------------
typedef unsigned long long nra_u64;
typedef __attribute__((address_space(1))) nra_u64 nra_gu64;
typedef __attribute__((address_space(1))) int nra_gi32;

// The serial hand-off: five planes of plain int32 per strip, two strips per wave used in turn (a block reads the one
// the block before wrote).  Writer and reader are the same wave, so every value is there when it is asked for.
struct SweepStripLink {
    volatile int32_t* cin;
    volatile int32_t* cout;
    int chain_cap;
    __device__ __forceinline__ bool fetch(int col, bool at_boundary, int& h, int& f, int& f2, int& s, int& b) const
    {
        if (col >= 0) {
            h = cin[col]; f = cin[chain_cap + col]; f2 = cin[2 * chain_cap + col];
            if (at_boundary) { s = cin[3 * chain_cap + col]; b = cin[4 * chain_cap + col]; }
        }
        return true;
    }
    __device__ __forceinline__ void publish(int plane, int col, int v) const { cout[plane * chain_cap + col] = v; }
};

// The concurrent hand-off (cdna_hip_programming.md Guideline 16, R2: the data is the flag): what lane 63 of block b
// leaves per column is stored as 8-byte granules {epoch, value}, ONE agent-scope (sc1, write-through) store each, into
// the strip between the two blocks; block b+1 loads the granules of the 64 columns it is about to hand to its
// lane 0 with agent-scope (sc1) loads and polls until every tag carries this launch's epoch.  No fence, no flag;
// the strips are zeroed once when the batch is created and every launch has an epoch of its own (never 0), so a
// granule of an earlier launch or run never passes.  Spins sleep (s_sleep), are bounded, and watch a launch-wide
// error word: a wave that gives up sets it, the others leave, the host reports NRA_E_DEVICE.
//
// Polls (2 - 3 us each: an s_sleep and 3 - 5 agent-scope loads) before a waiting wave gives up: ~2.5 s, three orders above
// the longest legitimate wait (64 * (skew + 1) steps of the block above, a millisecond or two).  A hang guard, not a
// path: the argument that no wave waits for ever (tickets, at k_sweep_ringmt: a producer holds a smaller ticket than its
// consumer, so it is running or done) assumes that a wave, once started, stays resident until it ends -- true as long as
// nothing preempts the queue (no CWSR / time-slicing against another process on the device); if that ever fails the guard
// turns a hang into NRA_E_DEVICE from nra_batch_sync / nra_batch1d_fetch.
#define NRA_MT_SPIN_LIMIT (1u << 20)
struct SweepGranuleLink {
    const nra_gu64* cin;
    nra_gu64* cout;
    int chain_cap;
    uint32_t epoch;
    nra_u64 tag;                          // epoch << 32
    nra_gi32* err;
    __device__ __forceinline__ bool fetch(int col, bool at_boundary, int& h, int& f, int& f2, int& s, int& b) const
    {
        const bool mine = col >= 0;
        const nra_gu64* g = cin + (mine ? col : 0);
        for (unsigned spins = 0;; ++spins) {
            bool ok = true;
            if (mine) {
                const nra_u64 x0 = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const nra_u64 x1 = __hip_atomic_load(g + chain_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const nra_u64 x2 = __hip_atomic_load(g + 2 * (size_t)chain_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (x0 >> 32) == epoch && (x1 >> 32) == epoch && (x2 >> 32) == epoch;
                h = (int)(unsigned)x0; f = (int)(unsigned)x1; f2 = (int)(unsigned)x2;
                if (at_boundary) {
                    const nra_u64 x3 = __hip_atomic_load(g + 3 * (size_t)chain_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const nra_u64 x4 = __hip_atomic_load(g + 4 * (size_t)chain_cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = ok && (x3 >> 32) == epoch && (x4 >> 32) == epoch;
                    s = (int)(unsigned)x3; b = (int)(unsigned)x4;
                }
            }
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) return true;
            __builtin_amdgcn_s_sleep(32);
            if ((spins & 15) == 15) {
                int failed = 0;
                if (threadIdx.x == 0) failed = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__builtin_amdgcn_readfirstlane(failed) != 0) return false;
                if (spins >= NRA_MT_SPIN_LIMIT) {
                    if (threadIdx.x == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return false;
                }
            }
        }
    }
    __device__ __forceinline__ void publish(int plane, int col, int v) const
    {
        __hip_atomic_store(cout + (size_t)plane * chain_cap + col, tag | (nra_u64)(unsigned)v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the maximum over the wave of a packed running maximum
template <bool W>
__device__ __forceinline__ int sweep_wave_max(int M)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) M = mx2<W>(M, __shfl_xor(M, off, 64));
    return M;
}

// Row block `blk` of `n_blk` of task tk.  Returns whether the launch is still good (false: a fetch gave up); a reverse
// sweep leaves the packed maximum over the block's cells in M_out, each lane its own.
template <int R, bool HAS_N, int DIR, bool W, class Link>
__device__ __forceinline__ bool sweep_rowblock_body(const NraSweepTask& tk, const int blk, const int n_blk, int4* ring, int2* racc,
                                                    const NraDevRead* __restrict__ reads,
                                                    const NraDevRegion* __restrict__ regions,
                                                    const uint8_t* __restrict__ pool,
                                                    const uint32_t* __restrict__ q2bit,
                                                    const uint32_t* __restrict__ qnmask,
                                                    const NraScoreParams& sp,
                                                    const int32_t* __restrict__ kmin_arr,
                                                    const int32_t* __restrict__ kmax_arr,
                                                    const uint32_t* __restrict__ coff,
                                                    int32_t* __restrict__ snap,
                                                    const int32_t* read_a,
                                                    int32_t* __restrict__ cand_score,
                                                    uint8_t* __restrict__ cand_flag, Link& link, int& M_out)
{
    constexpr int SC = 2;
    constexpr int BIASW = W ? 0 : BIAS;
    constexpr int P1 = SweepScores<SC, W>::P1;
    const int lane = threadIdx.x;
    const int wr = (lane + 1) & 63;
    const bool first_blk = blk == 0, last_blk = blk == n_blk - 1;
    const bool has_b = !W && tk.read_b >= 0;
    const int ra = tk.read_a, rb = has_b ? tk.read_b : tk.read_a;
    const NraDevRead rda = reads[ra], rdb = reads[rb];
    const NraDevRegion rg = regions[rda.region];
    const int m = rg.m1;
    const int flank = DIR ? rg.l1 : rg.l3;
    const uint8_t* __restrict__ piece = pool + (DIR ? rg.p1_off : rg.pr_off);
    const int ncols = DIR ? flank + m * tk.kmax : flank;
    const int jfirst = DIR ? flank + m * tk.kmin - 1 : flank - 1;
    const int skew = DIR ? m : 1;
    const SweepCands cands(ra, rb, has_b, kmin_arr, kmax_arr, coff);
    int32_t* __restrict__ snap_task = snap + tk.snap_off;
    const SweepScores<SC, W> sc(sp);
    const int v_floor = sc.v_floor, NEG1 = sc.NEG1, NEG2 = sc.NEG2;

    // What enters row 0 of this block at template column `col` (each lane its own column): constants for the first
    // block and outside the template, else what the block above has left in the link.
    auto fetch = [&](int col, int& h, int& f, int& f2, int& s, int& b) -> bool {
        h = v_floor; f = NEG1; f2 = NEG1; s = NEG2; b = NEG1;
        if (first_blk) return true;
        const bool mine = col >= 0 && col < ncols;
        const bool at_boundary = DIR == 1 && mine && col >= jfirst && (col - jfirst) % m == 0;
        return link.fetch(mine ? col : -1, at_boundary, h, f, f2, s, b);
    };

    auto column_table = [&](int col) { return sweep_column_table<DIR>(sc, piece, ncols, flank, col); };

    int out_a = 0, out_b = 0;
    int n_out = 0, kcur = tk.kmin;                          // wave-uniform
    auto flush = [&](int n_valid) { sweep_flush(cands, n_valid, kcur, lane, out_a, out_b, cand_score, cand_flag); };
    // A (best alignment inside R, doubled) of the two reads: wave-uniform, kept in scalar registers
    const int a_of_a = DIR ? __builtin_amdgcn_readfirstlane(read_a[ra]) : 0, a_of_b = DIR ? __builtin_amdgcn_readfirstlane(read_a[rb]) : 0;

    const int nsteps = ncols + 63 * skew;
    const int row_base = blk * 64 * R;

    int qc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int gi = row_base + lane * R + i;
        const int ca = sweep_query_sel<HAS_N>(rda, q2bit, qnmask, gi, DIR == 0);
        const int cb = W ? 0x0c : sweep_query_sel<HAS_N>(rdb, q2bit, qnmask, gi, DIR == 0);
        qc[i] = ca | (0x0c << 8) | (cb << 16) | (0x0c << 24);
    }
    int Hbo[DIR ? R : 1], Ebo[DIR ? R : 1], E2bo[DIR ? R : 1];
    if (DIR) {
        const int q1 = SC * (sp.open1 - sp.ext1), q2 = SC * (sp.open2 - sp.ext2);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int r = row_base + lane * R + i;
            int h[2], e[2], e2[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int a = (s ? rdb.qlen : rda.qlen) - 2 - r;
                if (a >= 0) {
                    const int ablk = a / (64 * R);
                    const int w = a - ablk * 64 * R;
                    const int al = w / R, ai = w - al * R;
                    const int32_t* __restrict__ p = snap_task + ((size_t)ablk * 3 * R + ai) * 64 + al;
                    const int vh = p[0], ve = p[R * 64], ve2 = p[2 * R * 64];
                    h[s] = (W ? vh : (s ? half_hi(vh) : half_lo(vh))) + 2 * sc.o1;
                    e[s] = (W ? ve : (s ? half_hi(ve) : half_lo(ve))) + q1;
                    e2[s] = (W ? ve2 : (s ? half_hi(ve2) : half_lo(ve2))) + q2;
                } else { h[s] = BIASW + sc.o1 - SC; e[s] = BIASW - SC; e2[s] = BIASW - SC; }
            }
            Hbo[i] = W ? h[0] : pack2(h[0], h[1]);
            Ebo[i] = W ? e[0] : pack2(e[0], e[1]);
            E2bo[i] = W ? e2[0] : pack2(e2[0], e2[1]);
        }
    }
    int Hq[R], Hq2[R], E[R], E2[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { Hq[i] = v_floor; Hq2[i] = NEG1; E[i] = NEG1; E2[i] = NEG1; }

    // ring: padding columns everywhere, then lane 0's first `skew` columns (and, when the first boundary is one
    // of them, its accumulators; a later first boundary gets them from lane 63 one boundary phase ahead, below)
#pragma unroll
    for (int s = 0; s < SWEEP_RING_D; ++s) ring[s * 64 + lane] = make_int4(v_floor, NEG1, NEG1, sc.tbl_mis4);
    racc[lane] = make_int2(NEG2, NEG1);
    int feed = sc.tbl_mis4, sH, sF, sF2, sS, sB;   // what lane 63 hands to lane 0
    if (!fetch(lane < skew ? lane : -1, sH, sF, sF2, sS, sB)) return false;
    if (lane < skew) ring[lane * 64] = make_int4(sH, sF, sF2, column_table(lane));
    if (DIR == 1 && lane == jfirst && jfirst < skew) racc[0] = make_int2(sS, sB);
    ring_order();

    int Hup_prev = v_floor, M = BIASW * P1;
    int slot = 0;
    int phase = jfirst % m, pcnt = 0, bidx = 0;
#pragma unroll 1
    for (int step = 0; step < nsteps; ++step) {
        if ((step & 63) == 0) {                                            // columns step + skew + (0..63)
            const int col = step + skew + wr;
            feed = column_table(col);
            if (!fetch(col, sH, sF, sF2, sS, sB)) return false;
        }
        const int4 in = ring[slot * 64 + lane];
        const int tt = in.w;
        const int fl = DIR == 1 ? (int)((((unsigned)tt >> 15) & (unsigned)P1) | (unsigned)(BIASW * P1)) : BIASW * P1;   // as in k_sweep_ring
        int F = mx2<W>(in.y, fl), F2 = in.z;
        sweep_cell<0, R, R, W, true>(Hq, Hq2, E, E2, qc, Hup_prev, F, F2, M, tt & 0x7f7f7f7f, sc.tbl_hi, fl, sc.v_e1, sc.v_e2, sc.v_o1, sc.v_o2);
        Hup_prev = mx2<W>(in.x, fl - sc.v_o1);
        ring[slot * 64 + wr] = make_int4(Hq[R - 1], F, F2, tt);
        if (lane == 63) ring[slot * 64] = make_int4(sH, sF, sF2, feed);
        ring_order();                                       // the next steps' loads stay behind these stores
        const int c63 = step - 63 * skew;                                  // the column lane 63 has just finished
        if (lane == 63 && !last_blk && c63 >= 0) { link.publish(0, c63, Hq[R - 1]); link.publish(1, c63, F); link.publish(2, c63, F2); }
        feed = dpp_rol1(feed); sH = dpp_rol1(sH); sF = dpp_rol1(sF); sF2 = dpp_rol1(sF2);
        if (++slot == skew) slot = 0;

        if constexpr (DIR == 0) {
            if (tt & FLAG_SNAPSHOT) sweep_snapshot<0, R, R>(Hq, E, E2, snap_task + (size_t)blk * 3 * R * 64, lane);
        } else {
            if (pcnt == phase) {                                           // wave-uniform
                if (step >= jfirst) {                                      // every lane on a unit boundary
                    const int tS = sweep_combine<0, R, R, W>(Hq, E, E2, Hbo, Ebo, E2bo, NEG2);
                    const int2 acc = racc[lane];
                    const int accS = mx2<W>(acc.x, tS), accB = mx2<W>(acc.y, M);
                    racc[wr] = make_int2(accS, accB);
                    if (lane == 63) {
                        racc[0] = make_int2(sS, sB);                       // of column step + skew: lane 0's next boundary
                        if (!last_blk && c63 >= 0) { link.publish(3, c63, accS); link.publish(4, c63, accB); }
                    }
                    ring_order();
                    if (last_blk && bidx >= 63 && kcur <= tk.kmax) {       // lane 63 is on the boundary of k = kcur
                        int va = 0, vb = 0;
                        if (lane == 63) {
                            va = sweep_emit<W>(accS, accB, 0, a_of_a + 1, sp.min_score);
                            if (!W) vb = sweep_emit<W>(accS, accB, 1, a_of_b + 1, sp.min_score);
                        }
                        out_a = dpp_rol1(out_a); out_b = dpp_rol1(out_b);
                        if (lane == 63) { out_a = va; out_b = vb; }
                        ++kcur; ++n_out;
                        if (n_out == 64) { flush(64); n_out = 0; }
                    }
                    ++bidx;
                } else if (step + m >= jfirst) {                           // one boundary phase before lane 0's first boundary
                    if (lane == 63) racc[0] = make_int2(sS, sB);           // of column step + skew = jfirst
                    ring_order();
                }
            }
            sS = dpp_rol1(sS); sB = dpp_rol1(sB);
            if (++pcnt == m) pcnt = 0;
        }
    }
    if (DIR == 0) M_out = M;
    else if (last_blk && n_out > 0) flush(n_out);
    return true;
}

// k_sweep_ringchain: the row blocks of a task one after the other in ONE wave, under NRA_F_SERIAL_CHAIN and when a
// read alone would need more strips than the concurrent form has.  A launch has one wave per strip pair and walks its
// tasks with a wave-uniform grid stride.
template <int R, bool HAS_N, int DIR, bool W>
__global__ __launch_bounds__(WAVE) void k_sweep_ringchain(int n_tasks, const NraSweepTask* __restrict__ tasks,
                                                          const NraDevRead* __restrict__ reads,
                                                          const NraDevRegion* __restrict__ regions,
                                                          const uint8_t* __restrict__ pool,
                                                          const uint32_t* __restrict__ q2bit,
                                                          const uint32_t* __restrict__ qnmask,
                                                          NraScoreParams sp,
                                                          const int32_t* __restrict__ kmin_arr,
                                                          const int32_t* __restrict__ kmax_arr,
                                                          const uint32_t* __restrict__ coff,
                                                          int32_t* __restrict__ snap,
                                                          int32_t* __restrict__ read_a,
                                                          int32_t* __restrict__ cand_score,
                                                          uint8_t* __restrict__ cand_flag,
                                                          int32_t* chain_buf, int chain_cap)
{
    constexpr int BIASW = W ? 0 : BIAS;
    __shared__ int4 ring[SWEEP_RING_D * 64];
    __shared__ int2 racc[64];
    volatile int32_t* strip = chain_buf + (size_t)blockIdx.x * 10 * chain_cap;
    for (int task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const NraSweepTask tk = tasks[task];
        const bool has_b = !W && tk.read_b >= 0;
        const int ra = tk.read_a, rb = has_b ? tk.read_b : tk.read_a;
        const int n_blk = (imax(reads[ra].qlen, reads[rb].qlen) + 64 * R - 1) / (64 * R);
        int a_all = BIASW * (W ? 1 : 0x00010001);           // reverse sweep: maximum over the cells of every block
        for (int blk = 0; blk < n_blk; ++blk) {
            SweepStripLink link{strip + ((blk + 1) & 1) * 5 * chain_cap, strip + (blk & 1) * 5 * chain_cap, chain_cap};
            int M = 0;
            sweep_rowblock_body<R, HAS_N, DIR, W>(tk, blk, n_blk, ring, racc, reads, regions, pool, q2bit, qnmask, sp, kmin_arr,
                                                  kmax_arr, coff, snap, read_a, cand_score, cand_flag, link, M);
            if (DIR == 0) a_all = mx2<W>(a_all, M);
        }
        if (DIR == 0) {
            // A = best alignment inside R (doubled) = the maximum over every cell of the sweep
            a_all = sweep_wave_max<W>(a_all);
            if (threadIdx.x == 0) {
                read_a[ra] = (W ? a_all : half_lo(a_all)) - BIASW;
                if (has_b) read_a[rb] = half_hi(a_all) - BIASW;
            }
        }
    }
}

// k_sweep_ringmt: the row blocks of a read as CONCURRENT waves.
//
// k_sweep_ringchain runs the blocks of a task one after the other in one wave: a batch of few long reads (2000
// cores of 3.7 kb = 1000 tasks of three blocks) then has one wave per SIMD.  Here a wave is one (task, row block):
// block b+1 starts as soon as block b has published the columns it needs and follows 64 * (skew + 1) steps behind,
// so the blocks of a read overlap and the launch has (blocks per read) times the waves.
//
// No deadlock, whatever the dispatch order: a wave takes its (task, block) by TICKET -- one atomic add when it
// starts -- and the block list is ordered so that a producer precedes its consumer (all blocks 0, then all blocks 1,
// ...).  Whoever holds a ticket runs; every smaller ticket was taken by a wave that has started, so the producer a
// wave waits for is running or done and never waits for a larger ticket.  (The waits themselves: SweepGranuleLink.)
template <int R, bool HAS_N, int DIR, bool W>
__global__ __launch_bounds__(WAVE, 3) void k_sweep_ringmt(int n_blocks, const NraChainBlock* __restrict__ blocks,
                                                       int32_t* ticket, const NraSweepTask* __restrict__ tasks,
                                                       const NraDevRead* __restrict__ reads,
                                                       const NraDevRegion* __restrict__ regions,
                                                       const uint8_t* __restrict__ pool,
                                                       const uint32_t* __restrict__ q2bit,
                                                       const uint32_t* __restrict__ qnmask,
                                                       NraScoreParams sp,
                                                       const int32_t* __restrict__ kmin_arr,
                                                       const int32_t* __restrict__ kmax_arr,
                                                       const uint32_t* __restrict__ coff,
                                                       int32_t* __restrict__ snap,
                                                       int32_t* read_a,
                                                       int32_t* __restrict__ cand_score,
                                                       uint8_t* __restrict__ cand_flag,
                                                       nra_u64* strips, int chain_cap, uint32_t epoch, int32_t* error)
{
    constexpr int BIASW = W ? 0 : BIAS;
    __shared__ int4 ring[SWEEP_RING_D * 64];
    __shared__ int2 racc[64];
    const int lane = threadIdx.x;
    int my = 0;
    if (lane == 0) my = atomicAdd(ticket, 1);
    my = __builtin_amdgcn_readfirstlane(my);
    if (my >= n_blocks) return;
    const NraChainBlock cb = blocks[my];
    const NraSweepTask tk = tasks[cb.task];
    const bool first_blk = cb.blk == 0, last_blk = cb.blk == cb.nblk - 1;
    SweepGranuleLink link{(const nra_gu64*)(strips + (size_t)(first_blk ? 0 : cb.strip_in) * 5 * (size_t)chain_cap),
                          (nra_gu64*)(strips + (size_t)(last_blk ? 0 : cb.strip_out) * 5 * (size_t)chain_cap), chain_cap, epoch,
                          (nra_u64)epoch << 32, (nra_gi32*)error};
    int M = 0;
    if (!sweep_rowblock_body<R, HAS_N, DIR, W>(tk, cb.blk, cb.nblk, ring, racc, reads, regions, pool, q2bit, qnmask, sp, kmin_arr,
                                               kmax_arr, coff, snap, read_a, cand_score, cand_flag, link, M))
        return;
    if (DIR == 0) {
        // A = best alignment inside R (doubled) = the maximum over every cell of every block: the blocks are waves
        // of their own, so each adds its maximum to the read's word (zeroed before the launch; A >= 0)
        const bool has_b = !W && tk.read_b >= 0;
        const int a_all = sweep_wave_max<W>(M);
        if (lane == 0) {
            atomicMax(&read_a[tk.read_a], (W ? a_all : half_lo(a_all)) - BIASW);
            if (has_b) atomicMax(&read_a[tk.read_b], half_hi(a_all) - BIASW);
        }
    }
}

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
template <int DIR>
static int launch_sweep(int R, int has_n, int chain, hipStream_t st, int n_tasks, const NraSweepTask* tasks, NraSweepArgs a,
                        int32_t* chain_buf, int chain_cap, int n_strips)
{
    if (n_tasks <= 0) return 0;
    if (DIR == 0) { a.cand_score = nullptr; a.cand_flag = nullptr; }      // a reverse sweep has no candidate outputs
#define ARGS n_tasks, tasks, SWEEP_FIELDS(a), chain_buf, chain_cap
    if (chain) {      // row-block chaining: only the instantiations long reads (and the tests) use
        if (n_strips <= 0) return (int)hipErrorInvalidValue;
        const int n_waves = n_tasks < n_strips ? n_tasks : n_strips;
        if (R == NRA_CHAIN_R) {
            if (has_n) k_sweep_pk16<NRA_CHAIN_R, true, DIR, true><<<n_waves, WAVE, 0, st>>>(ARGS);
            else k_sweep_pk16<NRA_CHAIN_R, false, DIR, true><<<n_waves, WAVE, 0, st>>>(ARGS);
        } else if (R == NRA_CHAIN_R_TEST) {
            if (has_n) k_sweep_pk16<NRA_CHAIN_R_TEST, true, DIR, true><<<n_waves, WAVE, 0, st>>>(ARGS);
            else k_sweep_pk16<NRA_CHAIN_R_TEST, false, DIR, true><<<n_waves, WAVE, 0, st>>>(ARGS);
        } else return (int)hipErrorInvalidValue;
        return (int)hipGetLastError();
    }
#define CASE(r)                                                                                     \
    case r:                                                                                         \
        if (has_n) k_sweep_pk16<r, true, DIR, false><<<n_tasks, WAVE, 0, st>>>(ARGS); \
        else k_sweep_pk16<r, false, DIR, false><<<n_tasks, WAVE, 0, st>>>(ARGS);       \
        break;
    switch (R) {
        NRA_R_LIST(CASE)
    default: return (int)hipErrorInvalidValue;
    }
#undef CASE
#undef ARGS
    return (int)hipGetLastError();
}

// the LDS-ring sweeps; HALF: the half-wave kernels, two read pairs per wave (R <= NRA_RING32_MAX_R)
template <int DIR, bool HALF>
int launch_sweep_ring(int R, int has_n, hipStream_t st, int n_tasks, const NraSweepTask* tasks, NraSweepArgs a, int relax_c,
                      int32_t* redo)
{
    if (n_tasks <= 0) return 0;
    if (DIR == 0) { a.cand_score = nullptr; a.cand_flag = nullptr; }
    const int grid = HALF ? n_tasks : (n_tasks + SWEEP_RING_WPB - 1) / SWEEP_RING_WPB;
#define ARGS n_tasks, tasks, SWEEP_FIELDS(a), relax_c, redo
#define LAUNCH(r, n, t)                                                                         \
    {                                                                                           \
        if constexpr (HALF) k_sweep_ring32<r, n, DIR, t><<<grid, WAVE, 0, st>>>(ARGS);         \
        else k_sweep_ring<r, n, DIR, t><<<grid, WAVE * SWEEP_RING_WPB, 0, st>>>(ARGS);         \
    }
#define CASE(r)                                                                                 \
    case r:                                                                                     \
        if constexpr (HALF && r > NRA_RING32_MAX_R) return (int)hipErrorInvalidValue;           \
        else if (relax_c > 0) { if (has_n) LAUNCH(r, true, true) else LAUNCH(r, false, true) }  \
        else { if (has_n) LAUNCH(r, true, false) else LAUNCH(r, false, false) }                 \
        break;
    switch (R) {
        NRA_R_LIST(CASE)
    default: return (int)hipErrorInvalidValue;
    }
#undef CASE
#undef LAUNCH
#undef ARGS
    return (int)hipGetLastError();
}

template <bool HALF>
int launch_sweep_ringq(int R, int has_n, hipStream_t st, int n_quanta, const uint32_t* qlist, int qsteps, int n_tasks, int32_t* ticket,
                       int32_t* arrivals, int32_t* giveup, int32_t* qstate, const NraSweepTask* tasks, NraSweepArgs a,
                       int relax_c, int32_t* redo, int sat_steps, int32_t* sat_count)
{
    if (n_quanta <= 0) return 0;
#define ARGS n_quanta, qlist, qsteps, n_tasks, ticket, arrivals, giveup, qstate, tasks, SWEEP_FIELDS(a), relax_c, redo, sat_steps, sat_count
#define CASE(r)                                                                                                          \
    case r:                                                                                                              \
        if constexpr (HALF && r > NRA_RING32_MAX_R) return (int)hipErrorInvalidValue;                                   \
        else if (relax_c > 0) { if (has_n) k_sweep_ringq<r, true, HALF, true><<<n_quanta, WAVE, 0, st>>>(ARGS);          \
                                else k_sweep_ringq<r, false, HALF, true><<<n_quanta, WAVE, 0, st>>>(ARGS); }             \
        else { if (has_n) k_sweep_ringq<r, true, HALF, false><<<n_quanta, WAVE, 0, st>>>(ARGS);                          \
               else k_sweep_ringq<r, false, HALF, false><<<n_quanta, WAVE, 0, st>>>(ARGS); }                             \
        break;
    switch (R) {
        NRA_R_LIST(CASE)
    default: return (int)hipErrorInvalidValue;
    }
#undef CASE
#undef ARGS
    return (int)hipGetLastError();
}

// The half-wave kernels compile in parts of their own (build.py): each of those parts instantiates its launcher, and the
// extern "C" launchers of parts 11, 12 and 25 call it.
#define NRA_SPEC(...) decltype(__VA_ARGS__) __VA_ARGS__
#if NRA_HAS_PART(15)
template NRA_SPEC(launch_sweep_ring<0, true>);
#else
extern template NRA_SPEC(launch_sweep_ring<0, true>);
#endif
#if NRA_HAS_PART(16)
template NRA_SPEC(launch_sweep_ring<1, true>);
#else
extern template NRA_SPEC(launch_sweep_ring<1, true>);
#endif
#if NRA_HAS_PART(26)
template NRA_SPEC(launch_sweep_ringq<true>);
#else
extern template NRA_SPEC(launch_sweep_ringq<true>);
#endif
#undef NRA_SPEC

#if NRA_HAS_PART(11)
extern "C" int nra_launch_sweep_ring_bwd(int R, int has_n, int half, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                                         NraSweepArgs a, int relax_c, int32_t* redo)
{
    return (half ? launch_sweep_ring<0, true> : launch_sweep_ring<0, false>)(R, has_n, st, n_tasks, tasks, a, relax_c, redo);
}
#endif
#if NRA_HAS_PART(12)
extern "C" int nra_launch_sweep_ring_fwd(int R, int has_n, int half, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                                         NraSweepArgs a, int relax_c, int32_t* redo)
{
    return (half ? launch_sweep_ring<1, true> : launch_sweep_ring<1, false>)(R, has_n, st, n_tasks, tasks, a, relax_c, redo);
}
#endif
#if NRA_HAS_PART(25)
extern "C" int nra_launch_sweep_ringq(int R, int has_n, int half, hipStream_t st, int n_quanta, const uint32_t* qlist, int qsteps,
                                      int n_tasks, int32_t* ticket, int32_t* arrivals, int32_t* giveup, int32_t* qstate,
                                      const NraSweepTask* tasks, NraSweepArgs a, int relax_c, int32_t* redo, int sat_steps,
                                      int32_t* sat_count)
{
    return (half ? launch_sweep_ringq<true> : launch_sweep_ringq<false>)(R, has_n, st, n_quanta, qlist, qsteps, n_tasks, ticket, arrivals,
                                                                          giveup, qstate, tasks, a, relax_c, redo, sat_steps, sat_count);
}
#endif

template <int DIR>
static int launch_sweep_ringchain(int R, int has_n, int wide, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                                  NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips)
{
    if (n_tasks <= 0) return 0;
    if (DIR == 0) { a.cand_score = nullptr; a.cand_flag = nullptr; }
    const int grid = n_tasks < n_strips ? n_tasks : n_strips;
#define ARGS n_tasks, tasks, SWEEP_FIELDS(a), chain_buf, chain_cap
#define LAUNCH(r)                                                                                        \
    do {                                                                                                 \
        if (wide) { if (has_n) k_sweep_ringchain<r, true, DIR, true><<<grid, WAVE, 0, st>>>(ARGS);      \
                    else k_sweep_ringchain<r, false, DIR, true><<<grid, WAVE, 0, st>>>(ARGS); }         \
        else { if (has_n) k_sweep_ringchain<r, true, DIR, false><<<grid, WAVE, 0, st>>>(ARGS);          \
               else k_sweep_ringchain<r, false, DIR, false><<<grid, WAVE, 0, st>>>(ARGS); }             \
    } while (0)
    if (R == NRA_RING_CHAIN_R) LAUNCH(NRA_RING_CHAIN_R);
    else if (R == NRA_CHAIN_R_TEST) LAUNCH(NRA_CHAIN_R_TEST);
    else return (int)hipErrorInvalidValue;
#undef LAUNCH
#undef ARGS
    return (int)hipGetLastError();
}

#if NRA_HAS_PART(13)
extern "C" int nra_launch_sweep_ringchain_bwd(int R, int has_n, int wide, hipStream_t st, int n_tasks,
                                              const NraSweepTask* tasks, NraSweepArgs a, int32_t* chain_buf, int chain_cap,
                                              int n_strips)
{
    return launch_sweep_ringchain<0>(R, has_n, wide, st, n_tasks, tasks, a, chain_buf, chain_cap, n_strips);
}
#endif
#if NRA_HAS_PART(14)
extern "C" int nra_launch_sweep_ringchain_fwd(int R, int has_n, int wide, hipStream_t st, int n_tasks,
                                              const NraSweepTask* tasks, NraSweepArgs a, int32_t* chain_buf, int chain_cap,
                                              int n_strips)
{
    return launch_sweep_ringchain<1>(R, has_n, wide, st, n_tasks, tasks, a, chain_buf, chain_cap, n_strips);
}
#endif

template <int DIR>
static int launch_sweep_ringmt(int R, int has_n, int wide, hipStream_t st, int n_blocks, const NraChainBlock* blocks,
                               int32_t* ticket, const NraSweepTask* tasks, NraSweepArgs a, uint64_t* strips, int chain_cap,
                               uint32_t epoch, int32_t* error)
{
    if (n_blocks <= 0) return 0;
    if (epoch == 0) return (int)hipErrorInvalidValue;
    if (DIR == 0) { a.cand_score = nullptr; a.cand_flag = nullptr; }
    hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
#define ARGS n_blocks, blocks, ticket, tasks, SWEEP_FIELDS(a), (nra_u64*)strips, chain_cap, epoch, error
#define LAUNCH(r)                                                                                        \
    do {                                                                                                 \
        if (wide) { if (has_n) k_sweep_ringmt<r, true, DIR, true><<<n_blocks, WAVE, 0, st>>>(ARGS);      \
                    else k_sweep_ringmt<r, false, DIR, true><<<n_blocks, WAVE, 0, st>>>(ARGS); }         \
        else { if (has_n) k_sweep_ringmt<r, true, DIR, false><<<n_blocks, WAVE, 0, st>>>(ARGS);          \
               else k_sweep_ringmt<r, false, DIR, false><<<n_blocks, WAVE, 0, st>>>(ARGS); }             \
    } while (0)
    // (the host picks the block height that pads a bucket's reads least: NRA_RING_MT_R_MIN .. NRA_RING_MT_R rows per lane)
    switch (R) {
    case 15: LAUNCH(15); break;
    case 14: LAUNCH(14); break;
    case 13: LAUNCH(13); break;
    case 12: LAUNCH(12); break;
    case NRA_CHAIN_R_TEST: LAUNCH(NRA_CHAIN_R_TEST); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef LAUNCH
#undef ARGS
    return (int)hipGetLastError();
}

#if NRA_HAS_PART(18)
extern "C" int nra_launch_sweep_ringmt_bwd(int R, int has_n, int wide, hipStream_t st, int n_blocks,
                                           const NraChainBlock* blocks, int32_t* ticket, const NraSweepTask* tasks,
                                           NraSweepArgs a, uint64_t* strips, int chain_cap, uint32_t epoch, int32_t* error)
{
    return launch_sweep_ringmt<0>(R, has_n, wide, st, n_blocks, blocks, ticket, tasks, a, strips, chain_cap, epoch, error);
}
#endif
#if NRA_HAS_PART(19)
extern "C" int nra_launch_sweep_ringmt_fwd(int R, int has_n, int wide, hipStream_t st, int n_blocks,
                                           const NraChainBlock* blocks, int32_t* ticket, const NraSweepTask* tasks,
                                           NraSweepArgs a, uint64_t* strips, int chain_cap, uint32_t epoch, int32_t* error)
{
    return launch_sweep_ringmt<1>(R, has_n, wide, st, n_blocks, blocks, ticket, tasks, a, strips, chain_cap, epoch, error);
}
#endif

#if NRA_HAS_PART(5)
extern "C" int nra_launch_sweep_bwd(int R, int has_n, int chain, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                                    NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips)
{
    return launch_sweep<0>(R, has_n, chain, st, n_tasks, tasks, a, chain_buf, chain_cap, n_strips);
}
#endif
#if NRA_HAS_PART(6)
extern "C" int nra_launch_sweep_fwd(int R, int has_n, int chain, hipStream_t st, int n_tasks, const NraSweepTask* tasks,
                                    NraSweepArgs a, int32_t* chain_buf, int chain_cap, int n_strips)
{
    return launch_sweep<1>(R, has_n, chain, st, n_tasks, tasks, a, chain_buf, chain_cap, n_strips);
}
#endif
