// nra_extend.hip -- anchored wraparound extension: how many motif bases a tract shows from its anchored end (gfx950).
//
//   k_extend<P>  one lane per read, 64 reads per wave (sorted by tract length, so the lanes of a wave run about as
//                long).  The lane keeps its row of p <= P phase cells -- a score H and a count M of motif bases consumed
//                per cell -- and its motif's match masks in registers: a row needs no cross-lane traffic.  The running
//                best (score, row, phase, count) stays in the lane; nothing is stored per row and nothing is traced
//                back.  One 16-byte store per read at the end.
// Cells j >= p of a capacity P > p are never read by a cell j < p (phase 0 takes cell p - 1 through ext_last).  Their
// match bits are 0, so every step into them adds -mismatch or -gap <= 0 to a cell of an earlier or the same row: they
// never exceed the running best of the cells j < p, and the strict comparison of the best keeps them out unmasked.
// The contract (recurrences, tie rules, outputs) is DESIGN.md section 16 and tests/extend_ref.py.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(30)

__device__ __forceinline__ uint64_t ext_eq(const uint64_t (&eq)[4], uint32_t c)
{
    return c == 0 ? eq[0] : c == 1 ? eq[1] : c == 2 ? eq[2] : c == 3 ? eq[3] : 0ull;
}

// cell pp - 1 of the row.  Capacities up to 6 are exact (pp == P); the others hold P / 2 < pp <= P (8: 6 < pp), so only
// the upper cells can be the last one.
template <int P>
__device__ __forceinline__ int ext_last(const int (&D)[P], int pp)
{
    if constexpr (P <= 6) {
        return D[P - 1];
    } else {
        // masked OR, not a select chain: the compiler turns a select chain into an indexed load from scratch
        constexpr int LO = P == 8 ? 6 : P / 2;
        int v = 0;
#pragma unroll
        for (int j = LO; j < P; ++j) v |= D[j] & -(int)(j == pp - 1);
        return v;
    }
}

// deletions along phases 1..P-1: H[j] = max(H[j], H[j-1] - g), strictly greater replaces, the count follows
template <int P>
__device__ __forceinline__ void ext_delete_pass(int (&H)[P], int (&M)[P], int g)
{
#pragma unroll
    for (int j = 1; j < P; ++j) {
        const int cand = H[j - 1] - g;
        const bool take = cand > H[j];
        H[j] = take ? cand : H[j];
        M[j] = take ? M[j - 1] + 1 : M[j];
    }
}

template <int P>
__global__ __launch_bounds__(WAVE) void k_extend(int n_reads, const NraStructRead* __restrict__ reads,
                                                 const NraStructMotif* __restrict__ motifs,
                                                 const uint8_t* __restrict__ codes, int a, int b, int g,
                                                 int32_t* __restrict__ res)
{
    const int idx = blockIdx.x * WAVE + threadIdx.x;
    if (idx >= n_reads) return;
    const NraStructRead rd = reads[idx];
    const NraStructMotif mo = motifs[rd.motif];
    const int pp = P <= 6 ? P : mo.p;      // exact capacities know p at compile time
    const uint64_t eq[4] = {mo.eq[0], mo.eq[1], mo.eq[2], mo.eq[3]};
    const int n = rd.n;
    const uint8_t* tract = codes + rd.tract;

    int H[P], M[P];
#pragma unroll
    for (int j = 0; j < P; ++j) H[j] = M[j] = 0;
    int best = 0, best_i = 0, best_j = 0, best_m = 0;
    for (int i0 = 0; i0 < n; i0 += NRA_STRUCT_BLOCK) {
        const uint4 blk = *reinterpret_cast<const uint4*>(tract + i0);
        const uint64_t lo = ((uint64_t)blk.y << 32) | blk.x, hi = ((uint64_t)blk.w << 32) | blk.z;
        const int nb = min(n - i0, NRA_STRUCT_BLOCK);
#pragma unroll 1
        for (int r = 0; r < nb; ++r) {
            const uint32_t c = (uint32_t)((r < 8 ? lo : hi) >> (8 * (r & 7))) & 0xffu;
            const uint64_t e = ext_eq(eq, c);
            // T[j] = max(diagonal from [i-1][j-1 mod p], insertion from [i-1][j]); a tie takes the diagonal
            const int last_h = ext_last<P>(H, pp), last_m = ext_last<P>(M, pp);
#pragma unroll
            for (int j = P - 1; j >= 0; --j) {
                const int src_h = j == 0 ? last_h : H[j - 1];
                const int src_m = j == 0 ? last_m : M[j - 1];
                const int diag = src_h + (((e >> j) & 1ull) ? a : -b);
                const int up = H[j] - g;
                const bool take = diag >= up;
                H[j] = take ? diag : up;
                M[j] = take ? src_m + 1 : M[j];
            }
            // deletions, cyclic: a pass without the wrap, the wrap into phase 0, a second pass
            if constexpr (P > 1) {
                ext_delete_pass<P>(H, M, g);
                const int cand = ext_last<P>(H, pp) - g;
                if (cand > H[0]) {                           // the second pass only carries on what the wrap changed
                    H[0] = cand;
                    M[0] = ext_last<P>(M, pp) + 1;
                    ext_delete_pass<P>(H, M, g);
                }
            }
            // running best: strictly greater replaces, so the smallest row and then the smallest phase keep a tie
            const int before = best;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const bool t = H[j] > best;
                best = t ? H[j] : best;
                best_j = t ? j : best_j;
                best_m = t ? M[j] : best_m;
            }
            best_i = best > before ? i0 + r + 1 : best_i;
        }
    }
    *reinterpret_cast<int4*>(res + 4 * (size_t)idx) = make_int4(best, best_i, best_j, best_m);
}

template <int P>
static int launch_extend(hipStream_t st, int n_reads, const NraStructRead* reads, const NraStructMotif* motifs,
                         const uint8_t* codes, int a, int b, int g, int32_t* res)
{
    k_extend<P><<<dim3((unsigned)((n_reads + WAVE - 1) / WAVE)), WAVE, 0, st>>>(n_reads, reads, motifs, codes, a, b, g,
                                                                              res);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_extend(hipStream_t st, int P, int n_reads, const NraStructRead* reads,
                                 const NraStructMotif* motifs, const uint8_t* codes, int match, int mismatch, int gap,
                                 int32_t* res)
{
    if (n_reads <= 0) return (int)hipSuccess;
    switch (P) {
    case 1: return launch_extend<1>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 2: return launch_extend<2>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 3: return launch_extend<3>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 4: return launch_extend<4>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 5: return launch_extend<5>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 6: return launch_extend<6>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 8: return launch_extend<8>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 16: return launch_extend<16>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 32: return launch_extend<32>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    case 64: return launch_extend<64>(st, n_reads, reads, motifs, codes, match, mismatch, gap, res);
    default: return (int)hipErrorInvalidValue;
    }
}

#endif  // part 30
