// nra_structure.hip -- repeat structure: wraparound edit-distance alignment of read tracts against their motif (gfx950).
//
//   k_structure<P>  one lane per read, 64 reads per wave (sorted by tract length, so the lanes of a wave run about as
//                   long).  The lane keeps its row of p <= P phase cells and its motif's match masks in registers: a row
//                   needs no cross-lane traffic.  Per row it stores 2 bits per phase (insertion taken, deletion taken)
//                   at [row][lane] of its wave's pointer block, so that the 64 stores of a row are one contiguous piece.
//                   Then the lane traces back from (n, end phase), NRA_STRUCT_BLOCK rows at a time: the block's pointer
//                   rows and codes are loaded together (the row index only falls, by one per base), and its path
//                   bytes leave in one 16-byte store.
// The contract (recurrences, tie rules, path bytes) is DESIGN.md section 14 and tests/structure_ref.py.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(28)

template <int P>
__device__ __forceinline__ void struct_pack(uint32_t* dst, uint64_t ins, uint64_t del)
{
    if constexpr (P <= 16) {
        dst[0] = (uint32_t)ins | ((uint32_t)del << 16);
    } else if constexpr (P <= 32) {
        *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)ins, (uint32_t)del);
    } else {
        *reinterpret_cast<uint4*>(dst) =
            make_uint4((uint32_t)ins, (uint32_t)(ins >> 32), (uint32_t)del, (uint32_t)(del >> 32));
    }
}

template <int P>
__device__ __forceinline__ void struct_load(const uint32_t* src, uint32_t (&w)[NRA_STRUCT_WORDS(P)])
{
    if constexpr (P <= 16) {
        w[0] = src[0];
    } else if constexpr (P <= 32) {
        const uint2 v = *reinterpret_cast<const uint2*>(src);
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

// (ins bit, del bit) of phase j in a loaded row
template <int P>
__device__ __forceinline__ void struct_bits(const uint32_t (&w)[NRA_STRUCT_WORDS(P)], int j, uint32_t& ins, uint32_t& del)
{
    if constexpr (P <= 16) {
        ins = (w[0] >> j) & 1u;
        del = (w[0] >> (16 + j)) & 1u;
    } else if constexpr (P <= 32) {
        ins = (w[0] >> j) & 1u;
        del = (w[1] >> j) & 1u;
    } else {
        const uint64_t i64 = ((uint64_t)w[1] << 32) | w[0];
        const uint64_t d64 = ((uint64_t)w[3] << 32) | w[2];
        ins = (uint32_t)(i64 >> j) & 1u;
        del = (uint32_t)(d64 >> j) & 1u;
    }
}

__device__ __forceinline__ uint64_t struct_eq(const uint64_t (&eq)[4], uint32_t c)
{
    return c == 0 ? eq[0] : c == 1 ? eq[1] : c == 2 ? eq[2] : c == 3 ? eq[3] : 0ull;
}

// cell pp - 1 of the row (pp == P needs no select)
template <int P>
__device__ __forceinline__ int struct_last(const int (&D)[P], int pp)
{
    if constexpr (P <= 6) {
        return D[P - 1];
    } else {
        // masked OR, not a select chain: the compiler turns a select chain into an indexed load from scratch
        int v = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) v |= D[j] & -(int)(j == pp - 1);
        return v;
    }
}

template <int P>
__global__ __launch_bounds__(WAVE) void k_structure(int n_reads, const NraStructRead* __restrict__ reads,
                                                    const NraStructMotif* __restrict__ motifs,
                                                    const uint8_t* __restrict__ codes, uint32_t* __restrict__ ptrs,
                                                    uint8_t* __restrict__ path, int32_t* __restrict__ res)
{
    constexpr int W = NRA_STRUCT_WORDS(P);
    constexpr int G = P >= 32 ? 4 : NRA_STRUCT_BLOCK;         // pointer rows loaded together in the traceback
    const int idx = blockIdx.x * WAVE + threadIdx.x;
    if (idx >= n_reads) return;
    const int lane = threadIdx.x;
    const NraStructRead rd = reads[idx];
    const NraStructMotif mo = motifs[rd.motif];
    const int pp = P <= 6 ? P : mo.p;      // exact capacities know p at compile time
    const uint64_t eq[4] = {mo.eq[0], mo.eq[1], mo.eq[2], mo.eq[3]};
    const int n = rd.n;
    const uint8_t* tract = codes + rd.tract;
    uint32_t* wptr = ptrs + rd.ptr + (uint64_t)lane * W;       // row r (1-based) at + (r - 1) * 64 * W

    // ---- forward: D[i][j], i = 1..n, in place
    int D[P];
#pragma unroll
    for (int j = 0; j < P; ++j) D[j] = 0;
    for (int i0 = 0; i0 < n; i0 += NRA_STRUCT_BLOCK) {
        const uint4 blk = *reinterpret_cast<const uint4*>(tract + i0);
        const uint64_t lo = ((uint64_t)blk.y << 32) | blk.x, hi = ((uint64_t)blk.w << 32) | blk.z;
        const int nb = min(n - i0, NRA_STRUCT_BLOCK);
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            const uint32_t c = (uint32_t)((b < 8 ? lo : hi) >> (8 * (b & 7))) & 0xffu;
            const uint64_t e = struct_eq(eq, c);
            // T[j] = min(diag from D[i-1][j-1 mod p], insertion from D[i-1][j]); a tie takes the diagonal
            const int last = struct_last<P>(D, pp);
            uint64_t ins = 0, del = 0;
#pragma unroll
            for (int j = P - 1; j >= 0; --j) {
                const int src = j == 0 ? last : D[j - 1];
                const int diag = src + (int)(((e >> j) & 1ull) ^ 1ull);
                const int up = D[j] + 1;
                ins |= (uint64_t)(up < diag) << j;
                D[j] = min(diag, up);
            }
            // deletions D[i][j - 1 mod p] + 1, cyclic: a pass without the wrap, the wrap into phase 0, a second pass;
            // a tie keeps T
#pragma unroll
            for (int j = 1; j < P; ++j) {
                const bool take = D[j - 1] + 1 < D[j] && j < pp;
                D[j] = take ? D[j - 1] + 1 : D[j];
                del |= (uint64_t)take << j;
            }
            {
                const int cand = struct_last<P>(D, pp) + 1;
                const bool take = cand < D[0];
                D[0] = take ? cand : D[0];
                del |= (uint64_t)take;
            }
#pragma unroll
            for (int j = 1; j < P; ++j) {
                const bool take = D[j - 1] + 1 < D[j] && j < pp;
                D[j] = take ? D[j - 1] + 1 : D[j];
                del |= (uint64_t)take << j;
            }
            struct_pack<P>(wptr + (uint64_t)(i0 + b) * (WAVE * W), ins, del);
        }
    }
    int best = D[0], endj = 0;
#pragma unroll
    for (int j = 1; j < P; ++j) {
        const bool t = j < pp && D[j] < best;
        best = t ? D[j] : best;
        endj = t ? j : endj;
    }

    // ---- traceback from (n, end phase), one block of NRA_STRUCT_BLOCK rows at a time (the lane's own stores above are
    // visible to its loads)
    int j = endj;
    for (int q = (n - 1) / NRA_STRUCT_BLOCK; n > 0 && q >= 0; --q) {
        const int i0 = q * NRA_STRUCT_BLOCK;
        const int top = min(n - i0, NRA_STRUCT_BLOCK);          // rows i0 + 1 .. i0 + top of this block
        const uint4 blk = *reinterpret_cast<const uint4*>(tract + i0);
        const uint32_t wd[4] = {blk.x, blk.y, blk.z, blk.w};
        uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int h = NRA_STRUCT_BLOCK / G - 1; h >= 0; --h) {
            uint32_t rows[G][W];
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (h * G + g < top) struct_load<P>(wptr + (uint64_t)(i0 + h * G + g) * (WAVE * W), rows[g]);
#pragma unroll
            for (int g = G - 1; g >= 0; --g) {
                const int b = h * G + g;
                if (b >= top) continue;
                uint32_t ins, del, nd = 0;
                struct_bits<P>(rows[g], j, ins, del);
                while (del) {                                    // at most pp - 1 deletions in a row
                    j = j == 0 ? pp - 1 : j - 1;
                    ++nd;
                    struct_bits<P>(rows[g], j, ins, del);
                }
                uint32_t op = 2u;
                if (!ins) {
                    const uint32_t c = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu;
                    op = (uint32_t)((struct_eq(eq, c) >> j) & 1ull) ^ 1u;
                    j = j == 0 ? pp - 1 : j - 1;
                }
                out[b >> 2] |= (op | (nd << 2)) << (8 * (b & 3));
            }
        }
        *reinterpret_cast<uint4*>(path + rd.tract + i0) = make_uint4(out[0], out[1], out[2], out[3]);
    }
    res[2 * idx] = best;
    res[2 * idx + 1] = n > 0 ? j : 0;
}

template <int P>
static int launch_structure(hipStream_t st, int n_reads, const NraStructRead* reads, const NraStructMotif* motifs,
                            const uint8_t* codes, uint32_t* ptrs, uint8_t* path, int32_t* res)
{
    k_structure<P><<<dim3((unsigned)((n_reads + WAVE - 1) / WAVE)), WAVE, 0, st>>>(n_reads, reads, motifs, codes, ptrs,
                                                                                 path, res);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_structure(hipStream_t st, int P, int n_reads, const NraStructRead* reads,
                                    const NraStructMotif* motifs, const uint8_t* codes, uint32_t* ptrs, uint8_t* path,
                                    int32_t* res)
{
    if (n_reads <= 0) return (int)hipSuccess;
    switch (P) {
    case 1: return launch_structure<1>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 2: return launch_structure<2>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 3: return launch_structure<3>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 4: return launch_structure<4>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 5: return launch_structure<5>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 6: return launch_structure<6>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 8: return launch_structure<8>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 16: return launch_structure<16>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 32: return launch_structure<32>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    case 64: return launch_structure<64>(st, n_reads, reads, motifs, codes, ptrs, path, res);
    default: return (int)hipErrorInvalidValue;
    }
}

#endif  // part 28
