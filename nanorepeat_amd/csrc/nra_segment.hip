// nra_segment.hip -- motif runs: edit-distance alignment of tracts against a set of motifs, each repeated without end,
// with a price for changing motif (gfx950).
//
//   k_segment<SC>  one lane per tract, 64 tracts per wave (sorted by tract length, so the lanes of a wave run about as
//                  long).  The lane keeps its row of S <= SC state cells in registers.  A lane owns its motif set, so
//                  the layout of the states differs between the lanes of a wave: it is held as per-lane bit masks over
//                  the states (first state of a motif, last state of a motif, eq[c] as in k_structure), every loop over
//                  the states is unrolled at compile time and no register array is indexed by a lane's value.  The wrap
//                  of the diagonal and of the deletion pass is a downward scan that latches the cell at a last-state
//                  bit and applies it at the next first-state bit.  Per row the lane stores 3 bits per state
//                  (insertion, deletion, switch) and the states of b1 and b2 at [row][lane] of its wave's pointer
//                  block, then traces back from (n, end state), NRA_STRUCT_BLOCK rows at a time, and stores the path
//                  bytes and the motif bytes of a block in one 16-byte store each.
// The contract (recurrences, tie rules, outputs) is include/nanorepeat_amd.h, DESIGN.md section 20 and
// tests/segment_ref.py.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(34)

#define SEG_BIG (1 << 28)                     // above every cell: n <= 200 000 edits, + W <= 1000

struct SegRow {
    uint32_t ins, del, sw, s1, s2;
};

template <int SC>
__device__ __forceinline__ void seg_pack(uint32_t* dst, uint32_t ins, uint32_t del, uint32_t sw, uint32_t s1, uint32_t s2)
{
    if constexpr (SC <= 8) {
        dst[0] = ins | (del << 8) | (sw << 16) | (s1 << 24) | (s2 << 27);
    } else if constexpr (SC <= 16) {
        *reinterpret_cast<uint2*>(dst) = make_uint2(ins | (del << 16), sw | (s1 << 16) | (s2 << 20));
    } else {
        *reinterpret_cast<uint4*>(dst) = make_uint4(ins, del, sw, s1 | (s2 << 8));
    }
}

template <int SC>
__device__ __forceinline__ void seg_load(const uint32_t* src, uint32_t (&w)[NRA_SEG_WORDS(SC)])
{
    if constexpr (SC <= 8) {
        w[0] = src[0];
    } else if constexpr (SC <= 16) {
        const uint2 v = *reinterpret_cast<const uint2*>(src);
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

template <int SC>
__device__ __forceinline__ SegRow seg_unpack(const uint32_t (&w)[NRA_SEG_WORDS(SC)])
{
    SegRow r;
    if constexpr (SC <= 8) {
        r.ins = w[0] & 0xffu; r.del = (w[0] >> 8) & 0xffu; r.sw = (w[0] >> 16) & 0xffu;
        r.s1 = (w[0] >> 24) & 7u; r.s2 = (w[0] >> 27) & 7u;
    } else if constexpr (SC <= 16) {
        r.ins = w[0] & 0xffffu; r.del = w[0] >> 16; r.sw = w[1] & 0xffffu;
        r.s1 = (w[1] >> 16) & 15u; r.s2 = (w[1] >> 20) & 15u;
    } else {
        r.ins = w[0]; r.del = w[1]; r.sw = w[2];
        r.s1 = w[3] & 31u; r.s2 = (w[3] >> 8) & 31u;
    }
    return r;
}

__device__ __forceinline__ uint32_t seg_eq(const uint32_t (&eq)[4], uint32_t c)
{
    return c == 0 ? eq[0] : c == 1 ? eq[1] : c == 2 ? eq[2] : c == 3 ? eq[3] : 0u;
}

// bits 0..g (g <= 31)
__device__ __forceinline__ uint32_t seg_upto(int g) { return (2u << g) - 1u; }

// the states of the motif that holds state g, as a mask
__device__ __forceinline__ uint32_t seg_motif_mask(uint32_t first, int g)
{
    const uint32_t upto = seg_upto(g);
    const int start = 31 - __clz((int)(first & upto));          // bit 0 is always a first state
    const uint32_t above = first & ~upto;                        // the first states of the motifs after it
    const uint32_t next = above & (0u - above);                  // the lowest of them, 0 when it is the last motif
    return ~((1u << start) - 1u) & (next - 1u);
}

// the state a diagonal step or a deletion comes from: g - 1, cyclic inside the motif
__device__ __forceinline__ int seg_prev(uint32_t first, int S, int g)
{
    if (!((first >> g) & 1u)) return g - 1;
    const uint32_t above = first & ~seg_upto(g);
    return (above ? __ffs((int)above) - 1 : S) - 1;
}

// (value, state) of the smallest cell among the states of `mask`, at the smallest such state
template <int SC>
__device__ __forceinline__ void seg_min(const int (&D)[SC], uint32_t mask, int& v, int& s)
{
    v = SEG_BIG; s = 0;
#pragma unroll
    for (int g = 0; g < SC; ++g) {
        const int x = ((mask >> g) & 1u) ? D[g] : SEG_BIG;
        const bool t = x < v;
        v = t ? x : v;
        s = t ? g : s;
    }
}

template <int SC>
__global__ __launch_bounds__(WAVE) void k_segment(int n_tracts, const NraStructRead* __restrict__ tracts,
                                                  const NraSegSet* __restrict__ sets, const uint8_t* __restrict__ codes,
                                                  int switch_cost, uint32_t* __restrict__ ptrs,
                                                  uint8_t* __restrict__ path, uint8_t* __restrict__ which,
                                                  int32_t* __restrict__ res)
{
    constexpr int W = NRA_SEG_WORDS(SC);
    constexpr int G = SC >= 32 ? 4 : NRA_STRUCT_BLOCK;        // pointer rows loaded together in the traceback
    const int idx = blockIdx.x * WAVE + threadIdx.x;
    if (idx >= n_tracts) return;
    const int lane = threadIdx.x;
    const NraStructRead rd = tracts[idx];
    const NraSegSet st = sets[rd.motif];
    const uint32_t eq[4] = {st.eq[0], st.eq[1], st.eq[2], st.eq[3]};
    const uint32_t first = st.first, last = st.last;
    const int S = st.S;
    const uint32_t valid = seg_upto(S - 1);                   // cells S .. SC - 1 are computed and never looked at
    const int n = rd.n;
    const uint8_t* tract = codes + rd.tract;
    uint32_t* wptr = ptrs + rd.ptr + (uint64_t)lane * W;      // row r (1-based) at + (r - 1) * 64 * W

    // ---- forward: D[i][g], i = 1..n, in place
    int D[SC];
#pragma unroll
    for (int g = 0; g < SC; ++g) D[g] = 0;
    for (int i0 = 0; i0 < n; i0 += NRA_STRUCT_BLOCK) {
        const uint4 blk = *reinterpret_cast<const uint4*>(tract + i0);
        const uint64_t lo = ((uint64_t)blk.y << 32) | blk.x, hi = ((uint64_t)blk.w << 32) | blk.z;
        const int nb = min(n - i0, NRA_STRUCT_BLOCK);
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            const uint32_t c = (uint32_t)((b < 8 ? lo : hi) >> (8 * (b & 7))) & 0xffu;
            const uint32_t e = seg_eq(eq, c);
            uint32_t ins = 0, del = 0, sw = 0;
            // T[g] = min(diagonal from D[i-1][prev g], insertion from D[i-1][g]); a tie takes the diagonal.  Downward, so
            // that D[g - 1] is still row i-1; the last state of a motif is latched before it is overwritten
            int latch = 0;
#pragma unroll
            for (int g = SC - 1; g >= 0; --g) {
                const int old = D[g];
                latch = ((last >> g) & 1u) ? old : latch;
                const int src = g == 0 ? latch : ((first >> g) & 1u) ? latch : D[g - 1];
                const int diag = src + (int)(((e >> g) & 1u) ^ 1u);
                const int up = old + 1;
                ins |= (uint32_t)(up < diag) << g;
                D[g] = min(diag, up);
            }
            // A: deletions A[prev g] + 1, cyclic inside each motif: a pass without the wrap, the wrap into the first
            // states, a second pass; a tie keeps T
#pragma unroll
            for (int g = 1; g < SC; ++g) {
                const bool take = D[g - 1] + 1 < D[g] && !((first >> g) & 1u);
                D[g] = take ? D[g - 1] + 1 : D[g];
                del |= (uint32_t)take << g;
            }
            latch = 0;
#pragma unroll
            for (int g = SC - 1; g >= 0; --g) {
                latch = ((last >> g) & 1u) ? D[g] : latch;
                const bool take = latch + 1 < D[g] && ((first >> g) & 1u);
                D[g] = take ? latch + 1 : D[g];
                del |= (uint32_t)take << g;
            }
#pragma unroll
            for (int g = 1; g < SC; ++g) {
                const bool take = D[g - 1] + 1 < D[g] && !((first >> g) & 1u);
                D[g] = take ? D[g - 1] + 1 : D[g];
                del |= (uint32_t)take << g;
            }
            // b1 over all states, b2 over the states of the other motifs (SEG_BIG when there is one motif only)
            int v1, s1, v2, s2;
            seg_min<SC>(D, valid, v1, s1);
            const uint32_t own = seg_motif_mask(first, s1);
            seg_min<SC>(D, valid & ~own, v2, s2);
            // D = min(A, b + W), b = b1 for the states outside b1's motif, b2 inside; a tie keeps A
            const int c1 = v1 + switch_cost, c2 = v2 + switch_cost;
#pragma unroll
            for (int g = 0; g < SC; ++g) {
                const int cand = ((own >> g) & 1u) ? c2 : c1;
                const bool take = cand < D[g];
                D[g] = take ? cand : D[g];
                sw |= (uint32_t)take << g;
            }
            seg_pack<SC>(wptr + (uint64_t)(i0 + b) * (WAVE * W), ins, del, sw, (uint32_t)s1, (uint32_t)s2);
        }
    }
    int best, g;
    seg_min<SC>(D, valid, best, g);

    // ---- traceback from (n, end state), one block of NRA_STRUCT_BLOCK rows at a time (the lane's own stores above are
    // visible to its loads)
    for (int q = (n - 1) / NRA_STRUCT_BLOCK; n > 0 && q >= 0; --q) {
        const int i0 = q * NRA_STRUCT_BLOCK;
        const int top = min(n - i0, NRA_STRUCT_BLOCK);          // rows i0 + 1 .. i0 + top of this block
        const uint4 blk = *reinterpret_cast<const uint4*>(tract + i0);
        const uint32_t wd[4] = {blk.x, blk.y, blk.z, blk.w};
        uint32_t out[4] = {0u, 0u, 0u, 0u}, mot[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int h = NRA_STRUCT_BLOCK / G - 1; h >= 0; --h) {
            uint32_t rows[G][W];
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (h * G + k < top) seg_load<SC>(wptr + (uint64_t)(i0 + h * G + k) * (WAVE * W), rows[k]);
#pragma unroll
            for (int k = G - 1; k >= 0; --k) {
                const int b = h * G + k;
                if (b >= top) continue;
                const SegRow r = seg_unpack<SC>(rows[k]);
                if ((r.sw >> g) & 1u) {                          // continues at the A-layer of the source state
                    const bool in_own = (seg_motif_mask(first, (int)r.s1) >> g) & 1u;
                    g = in_own ? (int)r.s2 : (int)r.s1;
                }
                uint32_t nd = 0;
                while ((r.del >> g) & 1u) {                      // at most p - 1 deletions in a row
                    g = seg_prev(first, S, g);
                    ++nd;
                }
                const uint32_t m = (uint32_t)__popc(first & seg_upto(g)) - 1u;
                uint32_t op = 2u;
                if (!((r.ins >> g) & 1u)) {
                    const uint32_t c = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu;
                    op = ((seg_eq(eq, c) >> g) & 1u) ^ 1u;
                    g = seg_prev(first, S, g);
                }
                out[b >> 2] |= (op | (nd << 2)) << (8 * (b & 3));
                mot[b >> 2] |= m << (8 * (b & 3));
            }
        }
        *reinterpret_cast<uint4*>(path + rd.tract + i0) = make_uint4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<uint4*>(which + rd.tract + i0) = make_uint4(mot[0], mot[1], mot[2], mot[3]);
    }
    const uint32_t below = first & seg_upto(g);
    *reinterpret_cast<int4*>(res + 4 * (size_t)idx) = make_int4(best, g - (31 - __clz((int)below)), __popc(below) - 1, 0);
}

template <int SC>
static int launch_segment(hipStream_t st, int n_tracts, const NraStructRead* tracts, const NraSegSet* sets,
                          const uint8_t* codes, int switch_cost, uint32_t* ptrs, uint8_t* path, uint8_t* which,
                          int32_t* res)
{
    k_segment<SC><<<dim3((unsigned)((n_tracts + WAVE - 1) / WAVE)), WAVE, 0, st>>>(n_tracts, tracts, sets, codes,
                                                                                 switch_cost, ptrs, path, which, res);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_segment(hipStream_t st, int SC, int n_tracts, const NraStructRead* tracts,
                                  const NraSegSet* sets, const uint8_t* codes, int switch_cost, uint32_t* ptrs,
                                  uint8_t* path, uint8_t* which, int32_t* res)
{
    if (n_tracts <= 0) return (int)hipSuccess;
    switch (SC) {
    case 8: return launch_segment<8>(st, n_tracts, tracts, sets, codes, switch_cost, ptrs, path, which, res);
    case 16: return launch_segment<16>(st, n_tracts, tracts, sets, codes, switch_cost, ptrs, path, which, res);
    case 32: return launch_segment<32>(st, n_tracts, tracts, sets, codes, switch_cost, ptrs, path, which, res);
    default: return (int)hipErrorInvalidValue;
    }
}

#endif  // part 34
