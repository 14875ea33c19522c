// nra_split.hip -- allele split: the pileup of a group's tracts on its backbone, the columns where the reads disagree
// systematically, and the two read sets behind them (gfx950).
//
//   k_split_align<C>  one wave per tract: the banded DP of nra_cons_dp.h (cons_band_align<C>, shared with k_cons_align).
//                     When the banded distance proves exact and is at most max_dist, lane 0 walks back from (n, t) and
//                     writes the tract's row, one code byte per backbone column (0..3 base, 4 a code-4 base, 5 deleted).
//                     The walk meets the columns from right to left: their bytes are packed into a 16-byte piece in
//                     registers and leave as one store per 16 columns.  No atomics.
//   k_split_count     256 columns of a group per workgroup: a lane owns a column and loops over the group's rows (a wave
//                     reads 64 consecutive bytes of a row), the four base counts stay in registers, and the lane calls
//                     its column: n[b] for a site, 0 for any other.
//   k_split_phase     one workgroup per group: lists the sites in column order (ballot and prefix count per 64 columns,
//                     running base per 256), cuts them to max_sites by a threshold on n[b] found by bisection, gathers
//                     their symbols into a [site][tract] byte matrix in global memory, and iterates: a wave owns a
//                     site and counts its eight (haplotype, base) cells by ballots over 64 reads at a time, the
//                     haplotype symbols live in LDS, a thread owns a read and relabels it, and one barrier-or tells
//                     whether a label changed.  Then the verdict and the outputs.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 19 and tests/split_ref.py.  No floating point; nothing
// depends on the order of the tracts or on timing.
#include "nra_cons_dp.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(33)

#define SPLIT_MAX_SITES 4096                  // NRA_SPLIT_MAX_SITES of the public header
#define SPLIT_WAVES (NRA_SPLIT_THREADS / WAVE)

template <int C>
__global__ __launch_bounds__(WAVE) void k_split_align(int n_items, const NraSplitItem* __restrict__ items,
                                                      const NraSplitGroup* __restrict__ groups,
                                                      const uint8_t* __restrict__ seqs,
                                                      const uint8_t* __restrict__ backbones, uint4* __restrict__ ptrs,
                                                      uint8_t* __restrict__ rows, int32_t* __restrict__ status,
                                                      int max_dist)
{
    const int it = blockIdx.x;
    if (it >= n_items) return;
    const int lane = threadIdx.x;
    const NraSplitItem item = items[it];
    const int n = item.n, t = groups[item.group].t;
    const uint8_t* s = seqs + item.seq;
    uint4* pblk = ptrs + item.ptr;
    int kend = 0;
    const int dist = cons_band_align<C>(n, t, s, backbones + groups[item.group].bb, pblk, lane, max_dist, kend);
    if (dist < 0) {                           // NRA_CONS_WIDEN or NRA_CONS_LEFT_OUT
        if (lane == 0) status[it] = dist;
        return;
    }
    __threadfence();                          // the other lanes' pointer stores, before lane 0 loads them
    __syncthreads();
    if (lane != 0) return;

    // ---- the walk back on one lane: column j - 1 gets the base aligned to it or "deleted"; insertions leave no mark
    uint8_t* row = rows + item.row;           // round_up(t, 16) bytes, 16-byte aligned
    int i = n, j = t, k = kend;
    long long have = -1, have_s = -1;
    uint4 pw = make_uint4(0, 0, 0, 0), sw = make_uint4(0, 0, 0, 0);
    uint4 piece = make_uint4(0, 0, 0, 0);     // the 16 columns around j
    uint32_t word = 0;                        // the 4 columns around j
    while (i > 0 || j > 0) {
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
            if (q == 0) {
                *reinterpret_cast<uint4*>(row + j) = piece;
                piece = make_uint4(0, 0, 0, 0);
            }
        }
    }
    status[it] = dist;
}

// the most voted of four counts and the second (ties go to the smaller code), and their counts
__device__ __forceinline__ void split_top2(const int (&n)[4], int& a, int& b, int& na, int& nb)
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

__global__ __launch_bounds__(NRA_SPLIT_THREADS) void k_split_count(int n_blocks, const NraSplitBlock* __restrict__ blocks,
                                                                   const NraSplitGroup* __restrict__ groups,
                                                                   const int64_t* __restrict__ rowtab,
                                                                   const uint8_t* __restrict__ rows, NraSplitParams prm,
                                                                   int32_t* __restrict__ col_nb,
                                                                   uint8_t* __restrict__ col_ab)
{
    if ((int)blockIdx.x >= n_blocks) return;
    const NraSplitBlock blk = blocks[blockIdx.x];
    const NraSplitGroup grp = groups[blk.group];
    const int j = blk.col0 + (int)threadIdx.x;
    if (j >= grp.t) return;
    const int64_t* rt = rowtab + grp.rows;
    int n[4] = {0, 0, 0, 0};
    for (int r = 0; r < grp.m; ++r) {
        const int64_t off = rt[r];            // the same for every lane
        if (off < 0) continue;
        const int c = rows[off + j];
#pragma unroll
        for (int x = 0; x < 4; ++x) n[x] += (int)(c == x);
    }
    int a, b, va, vb;
    split_top2(n, a, b, va, vb);
    const long long na = va, nb = vb;
    const bool site = nb >= prm.min_count && 100 * nb >= (long long)prm.min_share_pct * (na + nb) &&
                      2 * (na + nb) >= (long long)grp.mv;
    col_nb[grp.col + j] = site ? (int)nb : 0;
    col_ab[grp.col + j] = (uint8_t)(a << 2 | b);
}

// position of a thread's element among those of the workgroup with `pred`, in thread order; total = how many
__device__ __forceinline__ int split_block_rank(bool pred, int* wcnt, int& total)
{
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const unsigned long long mask = __ballot(pred);
    if (lane == 0) wcnt[wv] = __popcll(mask);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SPLIT_WAVES; ++w) {
        const int c = wcnt[w];
        before += w < wv ? c : 0;
        total += c;
    }
    __syncthreads();
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ int split_block_sum(int v, int* wcnt)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & (WAVE - 1)) == 0) wcnt[threadIdx.x / WAVE] = v;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < SPLIT_WAVES; ++w) total += wcnt[w];
    __syncthreads();
    return total;
}

// The haplotype symbols of every site from the labels as they stand: wave w takes the sites w, w + 4, ...; with `out`
// it also writes the site records (haplotypes swapped if `swap`) and counts the supported sites in *n_sup.
__device__ __forceinline__ void split_hap_symbols(int S, int m, const uint8_t* __restrict__ mat,
                                                  const int32_t* __restrict__ lab, const uint8_t* sab,
                                                  uint8_t (*hs)[SPLIT_MAX_SITES], const int32_t* __restrict__ pos,
                                                  int32_t* __restrict__ out, bool swap, int purity, int* n_sup)
{
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int q = wv; q < S; q += SPLIT_WAVES) {
        const uint8_t* line = mat + (size_t)q * m;
        int cnt[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        for (int r0 = 0; r0 < m; r0 += WAVE) {
            const int r = r0 + lane;
            const int l = r < m ? lab[r] : -1;
            const int sym = r < m ? line[r] : NRA_SPLIT_SYM_NONE;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 4; ++c) cnt[h][c] += __popcll(__ballot(l == h && sym == c));
        }
        int sym[2], tot[2], own[2];                  // own: the rows that show the most voted base
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int a = 0, best = cnt[h][0];
#pragma unroll
            for (int c = 1; c < 4; ++c) {
                a = cnt[h][c] > best ? c : a;
                best = imax(best, cnt[h][c]);
            }
            own[h] = best;
            tot[h] = cnt[h][0] + cnt[h][1] + cnt[h][2] + cnt[h][3];
            const int ab = sab[q];
            sym[h] = tot[h] > 0 ? a : (h == 0 ? ab >> 2 : ab & 3);    // nobody shows a base: a for 0, b for 1
        }
        if (lane == 0) {
            hs[0][q] = (uint8_t)sym[0];
            hs[1][q] = (uint8_t)sym[1];
            if (out) {
                bool ok = sym[0] != sym[1];
#pragma unroll
                for (int h = 0; h < 2; ++h)       // own = 0 where the symbol is the site's a or b for want of a base
                    ok = ok && own[h] > 0 && 100ll * own[h] >= (long long)purity * tot[h];
                int32_t* rec = out + (size_t)q * NRA_SPLIT_SITE_INTS;
                const int h0 = swap ? 1 : 0;
                rec[0] = pos[q];
                rec[1] = sym[h0];
                rec[2] = sym[1 - h0];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    rec[3 + c] = swap ? cnt[1][c] : cnt[0][c];
                    rec[7 + c] = swap ? cnt[0][c] : cnt[1][c];
                }
                rec[11] = ok ? 1 : 0;
                if (ok) atomicAdd(n_sup, 1);
            }
        }
    }
}

__global__ __launch_bounds__(NRA_SPLIT_THREADS) void k_split_phase(int n_groups, const NraSplitGroup* __restrict__ groups,
                                                                   const int64_t* __restrict__ rowtab,
                                                                   const uint8_t* __restrict__ rows, NraSplitParams prm,
                                                                   const int32_t* __restrict__ col_nb,
                                                                   const uint8_t* __restrict__ col_ab,
                                                                   int32_t* __restrict__ col_pos,
                                                                   int32_t* __restrict__ col_key,
                                                                   uint8_t* __restrict__ mats, int32_t* __restrict__ labels,
                                                                   int32_t* __restrict__ sites, int32_t* __restrict__ res)
{
    __shared__ uint8_t hs[2][SPLIT_MAX_SITES];    // the haplotype symbols
    __shared__ uint8_t sab[SPLIT_MAX_SITES];      // a << 2 | b of the kept sites
    __shared__ int wcnt[SPLIT_WAVES];
    __shared__ int sh_anchor, sh_sup;
    const int g = blockIdx.x;
    if (g >= n_groups) return;
    const int tid = threadIdx.x;
    const NraSplitGroup grp = groups[g];
    const int t = grp.t, m = grp.m, K = prm.max_sites;
    const int32_t* nbv = col_nb + grp.col;
    const uint8_t* abv = col_ab + grp.col;
    int32_t* pos = col_pos + grp.col;
    int32_t* key = col_key + grp.col;
    const int64_t* rt = rowtab + grp.rows;
    uint8_t* mat = mats + grp.mat;
    int32_t* lab = labels + grp.first;
    int32_t* out = res + (size_t)g * NRA_SPLIT_RES_INTS;

    // ---- the sites in column order
    int S = 0;
    if (grp.mv > 0)
        for (int j0 = 0; j0 < t; j0 += NRA_SPLIT_THREADS) {
            const int j = j0 + tid;
            const int nb = j < t ? nbv[j] : 0;
            int total;
            const int at = S + split_block_rank(nb > 0, wcnt, total);
            if (nb > 0) {
                pos[at] = j;
                key[at] = nb;
            }
            S += total;
        }
    __syncthreads();
    if (S > K) {
        // the smallest v with at most K sites of n[b] >= v: those stay, and the first sites of n[b] = v - 1 fill up
        int lo = 1, hi = grp.mv + 1;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            int c = 0;
            for (int q = tid; q < S; q += NRA_SPLIT_THREADS) c += (int)(key[q] >= mid);
            if (split_block_sum(c, wcnt) <= K) hi = mid; else lo = mid;
        }
        int c = 0;
        for (int q = tid; q < S; q += NRA_SPLIT_THREADS) c += (int)(key[q] >= hi);
        const int fill = K - split_block_sum(c, wcnt);
        int kept = 0, seen_eq = 0;
        for (int q0 = 0; q0 < S; q0 += NRA_SPLIT_THREADS) {
            const int q = q0 + tid;
            const int kq = q < S ? key[q] : 0, pq = q < S ? pos[q] : 0;
            int total_eq, total;
            const int eq_at = seen_eq + split_block_rank(kq == hi - 1, wcnt, total_eq);
            const bool keep = kq >= hi || (kq == hi - 1 && eq_at < fill);
            const int at = kept + split_block_rank(keep, wcnt, total);   // at <= q: written after the chunk was read
            if (keep) {
                pos[at] = pq;
                key[at] = kq;
            }
            seen_eq += total_eq;
            kept += total;
        }
        S = kept;
        __syncthreads();
    }

    // ---- the matrix, the anchor, the start labels
    for (int q = tid; q < S; q += NRA_SPLIT_THREADS) sab[q] = abv[pos[q]];
    if (tid == 0) {
        int best = 0;
        for (int q = 1; q < S; ++q) best = key[q] > key[best] ? q : best;     // a tie keeps the smaller column
        sh_anchor = best;
        sh_sup = 0;
    }
    __syncthreads();
    const int anchor = sh_anchor;
    for (int r = tid; r < m; r += NRA_SPLIT_THREADS) {
        const int64_t off = rt[r];
        for (int q = 0; q < S; ++q) mat[(size_t)q * m + r] = off >= 0 ? rows[off + pos[q]] : (uint8_t)NRA_SPLIT_SYM_NONE;
        int l = -1;
        if (off >= 0) {
            l = 0;
            if (S > 0) {
                const int sym = rows[off + pos[anchor]], ab = sab[anchor];
                l = sym == (ab >> 2) ? 0 : sym == (ab & 3) ? 1 : NRA_SPLIT_UNDECIDED;
            }
        }
        lab[r] = l;
    }

    // ---- up to max_iter rounds of haplotype symbols and labels
    int iters = 0;
    if (S > 0)
        for (int round = 0; round < prm.max_iter; ++round) {
            ++iters;
            __syncthreads();
            split_hap_symbols(S, m, mat, lab, sab, hs, pos, nullptr, false, 0, nullptr);
            __syncthreads();
            int changed = 0;
            for (int r = tid; r < m; r += NRA_SPLIT_THREADS) {
                const int l = lab[r];
                if (l < 0) continue;
                int m0 = 0, m1 = 0;
                for (int q = 0; q < S; ++q) {
                    const int sym = mat[(size_t)q * m + r];
                    m0 += (int)(sym < 4 && sym != hs[0][q]);
                    m1 += (int)(sym < 4 && sym != hs[1][q]);
                }
                const int nl = m0 < m1 ? 0 : m1 < m0 ? 1 : l;
                if (nl != l) {
                    lab[r] = nl;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    __syncthreads();

    // ---- the verdict
    int c0 = 0, c1 = 0, cu = 0;
    for (int r = tid; r < m; r += NRA_SPLIT_THREADS) {
        const int l = lab[r];
        c0 += (int)(l == 0);
        c1 += (int)(l == 1);
        cu += (int)(l == NRA_SPLIT_UNDECIDED);
    }
    const int n0 = split_block_sum(c0, wcnt), n1 = split_block_sum(c1, wcnt), und = split_block_sum(cu, wcnt);
    const bool swap = n1 > n0;                 // haplotype 0 is the larger one; a tie keeps the start
    split_hap_symbols(S, m, mat, lab, sab, hs, pos, sites + grp.site * NRA_SPLIT_SITE_INTS, swap, prm.min_purity_pct,
                      &sh_sup);
    __syncthreads();
    if (swap)
        for (int r = tid; r < m; r += NRA_SPLIT_THREADS) {
            const int l = lab[r];
            if (l == 0 || l == 1) lab[r] = 1 - l;
        }
    if (tid == 0) {
        const int big = swap ? n1 : n0, small = swap ? n0 : n1, sup = sh_sup;
        out[0] = (big >= prm.min_count && small >= prm.min_count && sup >= prm.min_sites) ? 1 : 0;
        out[1] = big;
        out[2] = small;
        out[3] = und;
        out[4] = m - grp.mv;
        out[5] = S;
        out[6] = sup;
        out[7] = iters;
    }
}

template <int C>
static int launch_split_align(hipStream_t st, int n_items, const NraSplitItem* items, const NraSplitGroup* groups,
                              const uint8_t* seqs, const uint8_t* backbones, uint4* ptrs, uint8_t* rows, int32_t* status,
                              int max_dist)
{
    k_split_align<C><<<dim3((unsigned)n_items), WAVE, 0, st>>>(n_items, items, groups, seqs, backbones, ptrs, rows, status,
                                                              max_dist);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_split_align(hipStream_t st, int c, int n_items, const NraSplitItem* items,
                                      const NraSplitGroup* groups, const uint8_t* seqs, const uint8_t* backbones,
                                      uint4* ptrs, uint8_t* rows, int32_t* status, int max_dist)
{
    if (n_items <= 0) return (int)hipSuccess;
    switch (c) {
    case 1: return launch_split_align<1>(st, n_items, items, groups, seqs, backbones, ptrs, rows, status, max_dist);
    case 2: return launch_split_align<2>(st, n_items, items, groups, seqs, backbones, ptrs, rows, status, max_dist);
    case 4: return launch_split_align<4>(st, n_items, items, groups, seqs, backbones, ptrs, rows, status, max_dist);
    case 8: return launch_split_align<8>(st, n_items, items, groups, seqs, backbones, ptrs, rows, status, max_dist);
    case 16: return launch_split_align<16>(st, n_items, items, groups, seqs, backbones, ptrs, rows, status, max_dist);
    default: return (int)hipErrorInvalidValue;
    }
}

extern "C" int nra_launch_split_count(hipStream_t st, int n_blocks, const NraSplitBlock* blocks,
                                      const NraSplitGroup* groups, const int64_t* rowtab, const uint8_t* rows,
                                      NraSplitParams prm, int32_t* col_nb, uint8_t* col_ab)
{
    if (n_blocks <= 0) return (int)hipSuccess;
    k_split_count<<<dim3((unsigned)n_blocks), NRA_SPLIT_THREADS, 0, st>>>(n_blocks, blocks, groups, rowtab, rows, prm,
                                                                         col_nb, col_ab);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_split_phase(hipStream_t st, int n_groups, const NraSplitGroup* groups, const int64_t* rowtab,
                                      const uint8_t* rows, NraSplitParams prm, const int32_t* col_nb,
                                      const uint8_t* col_ab, int32_t* col_pos, int32_t* col_key, uint8_t* mats,
                                      int32_t* labels, int32_t* sites, int32_t* res)
{
    if (n_groups <= 0) return (int)hipSuccess;
    k_split_phase<<<dim3((unsigned)n_groups), NRA_SPLIT_THREADS, 0, st>>>(n_groups, groups, rowtab, rows, prm, col_nb,
                                                                         col_ab, col_pos, col_key, mats, labels, sites,
                                                                         res);
    return (int)hipGetLastError();
}

#endif  // part 33
