// nra_flank.hip -- flank haplotypes: the pileup of the reads' flank segments on the two reference flanks of a region and
// the columns where the reads disagree systematically (gfx950).  The two haplotypes behind those columns are
// k_split_phase's (nra_split.hip), launched as it is on the rows and column calls written here.
//
//   k_flank_align<C>  one wave per (row, side): the banded DP of nra_cons_dp.h with the start pinned and the end free
//                     (cons_band_align<C, true>: the band centred on diagonal 0, then a wave reduction of (value,
//                     column) over row n, the smallest column winning).  When the banded distance proves exact and is
//                     at most max_dist, lane 0 walks back from (n, j*) and writes the codes of the columns below j* as
//                     k_split_align does, one 16-byte store per 16 columns; the piece that holds j* leaves with "not
//                     covered" in its bytes from j* on, and the pieces above it keep what the host set.  No atomics.
//   k_flank_count     k_split_count with the coverage of the column (rows whose code is <= 5) in place of m_v and no
//                     site at a side offset below `skip`.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 25 and tests/flank_ref.py.  No floating point; nothing
// depends on the order of the rows or on timing.
#include "nra_cons_dp.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(38)

#define FLANK_NONE4 (0x01010101u * NRA_FLANK_SYM_NONE)

template <int C>
__global__ __launch_bounds__(WAVE) void k_flank_align(int n_items, const NraFlankItem* __restrict__ items,
                                                      const uint8_t* __restrict__ seqs,
                                                      const uint8_t* __restrict__ backbones, uint4* __restrict__ ptrs,
                                                      uint8_t* __restrict__ rows, int32_t* __restrict__ status,
                                                      int max_dist)
{
    const int it = blockIdx.x;
    if (it >= n_items) return;
    const int lane = threadIdx.x;
    const NraFlankItem item = items[it];
    const int n = item.n;
    const uint8_t* s = seqs + item.seq;
    uint4* pblk = ptrs + item.ptr;
    int kend = 0;
    const int dist = cons_band_align<C, true>(n, item.t, s, backbones + item.bb, pblk, lane, max_dist, kend);
    if (dist < 0) {                           // NRA_CONS_WIDEN or NRA_CONS_LEFT_OUT
        if (lane == 0) status[2 * it] = dist;
        return;
    }
    __threadfence();                          // the other lanes' pointer stores, before lane 0 loads them
    __syncthreads();
    if (lane != 0) return;

    // ---- the walk back on one lane, from (n, j*): column j - 1 gets the base aligned to it or "deleted"
    uint8_t* row = rows + item.row;           // round_up(t, 16) bytes, 16-byte aligned, all NRA_FLANK_SYM_NONE
    const int jend = n + kend - (32 * C - 1);
    int i = n, j = jend, k = kend;
    long long have = -1, have_s = -1;
    uint4 pw = make_uint4(0, 0, 0, 0), sw = make_uint4(0, 0, 0, 0);
    uint4 piece = make_uint4(FLANK_NONE4, FLANK_NONE4, FLANK_NONE4, FLANK_NONE4);   // the 16 columns around j
    uint32_t word = (j & 3) ? FLANK_NONE4 << (8 * (j & 3)) : 0u;                    // the 4 columns around j
    while (j > 0) {                           // what is left at j = 0 are insertions
        const uint32_t op = cons_walk_op<C>(pblk, n, i, j, k, have, pw);
        if (op == 1u) {
            --i;
            ++k;
            continue;
        }
        uint32_t code = NRA_SPLIT_SYM_DELETED;
        if (op == 0u) {
            code = (uint32_t)cons_walk_base(s, i, have_s, sw);
            --i;
        } else {
            --k;
        }
        --j;
        word |= code << (8 * (j & 3));
        if ((j & 3) == 0) {
            const int q = (j >> 2) & 3;
            if (q == 0) piece.x = word; else if (q == 1) piece.y = word; else if (q == 2) piece.z = word; else piece.w = word;
            word = 0;
            if (q == 0) *reinterpret_cast<uint4*>(row + j) = piece;
        }
    }
    status[2 * it] = dist;
    status[2 * it + 1] = jend;
}

// the most voted of four counts and the second (ties go to the smaller code), and their counts: split_top2 of nra_split.hip
__device__ __forceinline__ void flank_top2(const int (&n)[4], int& a, int& b, int& na, int& nb)
{
    a = 0;
    int best = n[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        a = n[c] > best ? c : a;
        best = imax(best, n[c]);
    }
    b = -1;
    int second = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool take = c != a && n[c] > second;
        b = take ? c : b;
        second = take ? n[c] : second;
    }
    na = best;
    nb = second;
}

__global__ __launch_bounds__(NRA_SPLIT_THREADS) void k_flank_count(int n_blocks, const NraSplitBlock* __restrict__ blocks,
                                                                   const NraSplitGroup* __restrict__ groups,
                                                                   const int32_t* __restrict__ lpad,
                                                                   const int64_t* __restrict__ rowtab,
                                                                   const uint8_t* __restrict__ rows, NraSplitParams prm,
                                                                   int skip, int32_t* __restrict__ col_nb,
                                                                   uint8_t* __restrict__ col_ab)
{
    if ((int)blockIdx.x >= n_blocks) return;
    const NraSplitBlock blk = blocks[blockIdx.x];
    const NraSplitGroup grp = groups[blk.group];
    const int j = blk.col0 + (int)threadIdx.x;
    if (j >= grp.t) return;
    const int64_t* rt = rowtab + grp.rows;
    const int right = lpad[blk.group];
    const int o = j >= right ? j - right : j; // the offset from the repeat (a padding column has no row that covers it)
    int n[4] = {0, 0, 0, 0};
    int cov = 0;
    for (int r = 0; r < grp.m; ++r) {
        const int64_t off = rt[r];            // the same for every lane
        if (off < 0) continue;
        const int c = rows[off + j];
#pragma unroll
        for (int x = 0; x < 4; ++x) n[x] += (int)(c == x);
        cov += (int)(c <= NRA_SPLIT_SYM_DELETED);
    }
    int a, b, va, vb;
    flank_top2(n, a, b, va, vb);
    const long long na = va, nb = vb;
    const bool site = o >= skip && nb >= prm.min_count && 100 * nb >= (long long)prm.min_share_pct * (na + nb) &&
                      2 * (na + nb) >= (long long)cov;
    col_nb[grp.col + j] = site ? (int)nb : 0;
    col_ab[grp.col + j] = (uint8_t)(a << 2 | b);
}

template <int C>
static int launch_flank_align(hipStream_t st, int n_items, const NraFlankItem* items, const uint8_t* seqs,
                              const uint8_t* backbones, uint4* ptrs, uint8_t* rows, int32_t* status, int max_dist)
{
    k_flank_align<C><<<dim3((unsigned)n_items), WAVE, 0, st>>>(n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_flank_align(hipStream_t st, int c, int n_items, const NraFlankItem* items, const uint8_t* seqs,
                                      const uint8_t* backbones, uint4* ptrs, uint8_t* rows, int32_t* status, int max_dist)
{
    if (n_items <= 0) return (int)hipSuccess;
    switch (c) {
    case 1: return launch_flank_align<1>(st, n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    case 2: return launch_flank_align<2>(st, n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    case 4: return launch_flank_align<4>(st, n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    case 8: return launch_flank_align<8>(st, n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    case 16: return launch_flank_align<16>(st, n_items, items, seqs, backbones, ptrs, rows, status, max_dist);
    default: return (int)hipErrorInvalidValue;
    }
}

extern "C" int nra_launch_flank_count(hipStream_t st, int n_blocks, const NraSplitBlock* blocks,
                                      const NraSplitGroup* groups, const int32_t* lpad, const int64_t* rowtab,
                                      const uint8_t* rows, NraSplitParams prm, int skip, int32_t* col_nb, uint8_t* col_ab)
{
    if (n_blocks <= 0) return (int)hipSuccess;
    k_flank_count<<<dim3((unsigned)n_blocks), NRA_SPLIT_THREADS, 0, st>>>(n_blocks, blocks, groups, lpad, rowtab, rows, prm,
                                                                         skip, col_nb, col_ab);
    return (int)hipGetLastError();
}

#endif  // part 38
