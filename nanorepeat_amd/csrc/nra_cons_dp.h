// nra_cons_dp.h -- the banded unit-cost alignment of one tract to a backbone by one wave, and the walk back through
// its pointers: shared by k_cons_align (nra_consensus.hip, votes) and k_split_align (nra_split.hip, pileup rows).
//
//   cons_band_align<C>  The band holds 64 C diagonals; lane l owns the C consecutive diagonals k = l C .. l C + C - 1
//                       (k = j - i - lo) in registers.  In diagonal coordinates the diagonal predecessor of a cell is
//                       the lane's own cell of the row before, the insertion predecessor is cell k + 1 of the row before
//                       (one cross-lane shift per row), and the deletions of a row are D[k] = k + prefix-min(T[k'] - k'):
//                       serial over the lane's C cells and one wave scan in DPP steps.  Two pointer bits per cell
//                       (0 diagonal, 1 insertion, 2 deletion) are shifted into a 128-bit register and leave as one
//                       16-byte store per lane every 64 / C rows: [row block][lane], 1 KB per wave and store.
//   cons_walk_op / _base  one lane's view of those pointers and of the tract's bases on the way back from (n, t).
// The contract is include/nanorepeat_amd.h and DESIGN.md section 18.  No floating point.
#ifndef NRA_CONS_DP_H
#define NRA_CONS_DP_H
#include "nra_device.h"

#define CONS_TILE 64                          // rows per staged tile of tract and backbone bases

// lane l <- lane l + 1; lane 63 keeps `old`
__device__ __forceinline__ int cons_shl1(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, 0x130 /*wave_shl:1*/, 0xf, 0xf, false);
}

// exclusive prefix minimum over the lanes of the wave (lane 0: NRA_CONS_INF)
__device__ __forceinline__ int cons_excl_prefix_min(int v)
{
    const int inf = NRA_CONS_INF;
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x111 /*row_shr:1*/, 0xf, 0xf, false));
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x112 /*row_shr:2*/, 0xf, 0xf, false));
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x114 /*row_shr:4*/, 0xf, 0xf, false));
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x118 /*row_shr:8*/, 0xf, 0xf, false));
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x142 /*row_bcast:15*/, 0xa, 0xf, false));
    v = imin(v, __builtin_amdgcn_update_dpp(inf, v, 0x143 /*row_bcast:31*/, 0xc, 0xf, false));
    return dpp_shr1(inf, v);
}

// byte q (0..15) of a 16-byte piece
__device__ __forceinline__ uint32_t cons_byte(const uint4& v, int q)
{
    const uint32_t w = (q >> 2) == 0 ? v.x : (q >> 2) == 1 ? v.y : (q >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (q & 3))) & 0xffu;
}

// The whole wave aligns s (n codes) to b (t codes) in band class C and leaves the pointers at pblk.  Returns the
// distance when the band proves it and it is at most max_dist (kend = the band column of (n, t)), else NRA_CONS_WIDEN
// (align again in the next class) or NRA_CONS_LEFT_OUT.  The caller fences before a lane reads the pointers.
// FREE_END (k_flank_align, nra_flank.hip): the start is pinned and the end is free.  The band is centred on diagonal 0,
// j - i in [-h, h + 1] with h = 32 C - 1: a path from (0, 0) that leaves [-h, h] costs more than h, so a cell of row n
// with a banded value <= h holds its true value and every other cell is > h either way.  The distance is the minimum of
// row n, at the smallest column j* that attains it; kend is the band column of (n, j*), j* = n + kend - h.
template <int C, bool FREE_END = false>
__device__ __forceinline__ int cons_band_align(int n, int t, const uint8_t* __restrict__ s, const uint8_t* __restrict__ b,
                                               uint4* __restrict__ pblk, int lane, int max_dist, int& kend)
{
    constexpr int B = WAVE * C;               // diagonals of the band
    constexpr int S = 2 * C;                  // pointer bits per lane and row
    constexpr int R = 128 / S;                // rows per 16-byte piece
    constexpr int INF = NRA_CONS_INF;
    __shared__ uint8_t sb[B + CONS_TILE];
    __shared__ uint8_t ss[CONS_TILE];
    const int delta = t - n, ad = delta < 0 ? -delta : delta;
    const int extra = FREE_END ? B - 2 : B - 1 - ad;
    if constexpr (FREE_END) {
        if (-delta > extra >> 1) return (extra >> 1) >= max_dist ? NRA_CONS_LEFT_OUT : NRA_CONS_WIDEN;   // row n is below the band
    } else {
        if (extra < 0) return NRA_CONS_WIDEN; // the band does not hold both corners
    }
    const int h = extra >> 1;
    const int lo = FREE_END ? -h : imin(0, delta) - h;       // diagonal of band column 0
    const int w = FREE_END ? h : ad + 2 * h;  // distances up to w are proven
    const int k0 = lane * C;

    int D[C];
#pragma unroll
    for (int x = 0; x < C; ++x) {
        const int j = lo + k0 + x;
        D[x] = (j >= 0 && j <= t) ? j : INF;
    }
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;  // the pointer bits of up to R rows; the oldest row ends lowest
    for (int i0 = 0; i0 < n; i0 += CONS_TILE) {
        // row i = i0 + 1 + r, band column k: its diagonal step reads b[j - 1], j - 1 = i0 + lo + r + k -> sb[r + k]
        __syncthreads();
        for (int y = lane; y < B + CONS_TILE; y += WAVE) {
            const int jj = i0 + lo + y;
            sb[y] = (jj >= 0 && jj < t) ? b[jj] : (uint8_t)NRA_CONS_CODE_PAD;
        }
        ss[lane] = i0 + lane < n ? s[i0 + lane] : (uint8_t)NRA_CONS_CODE_OTHER;
        __syncthreads();
        const int nb = imin(CONS_TILE, n - i0);
        for (int r = 0; r < nb; ++r) {
            const int i = i0 + 1 + r;
            const int sc = ss[r];
            const int jb = i + lo + k0;                           // column j of the lane's cell 0
            const int up_next = cons_shl1(INF, D[0]);             // cell 0 of the next lane, row i - 1
            int dg[C], up[C], T[C];
#pragma unroll
            for (int x = 0; x < C; ++x) {
                dg[x] = D[x] + (int)(sb[r + k0 + x] != sc);
                up[x] = (x + 1 < C ? D[x + 1] : up_next) + 1;
                const bool valid = (unsigned)(jb + x) <= (unsigned)t;
                T[x] = valid ? imin(dg[x], up[x]) : INF;
            }
            // deletions: D[k] = k + min over k' <= k of (T[k'] - k')
            int run = INF;
            int pm[C];
#pragma unroll
            for (int x = 0; x < C; ++x) {
                run = imin(run, T[x] - (k0 + x));
                pm[x] = run;
            }
            const int before = cons_excl_prefix_min(run);
            uint32_t bits = 0;
#pragma unroll
            for (int x = 0; x < C; ++x) {
                const bool valid = (unsigned)(jb + x) <= (unsigned)t;
                const int e = valid ? imin(pm[x], before) + (k0 + x) : INF;
                const uint32_t code = dg[x] == e ? 0u : up[x] == e ? 1u : 2u;
                bits |= code << (2 * x);
                D[x] = e;
            }
            if constexpr (S == 32) {
                a0 = a1; a1 = a2; a2 = a3; a3 = bits;
            } else {
                a0 = (a0 >> S) | (a1 << (32 - S));
                a1 = (a1 >> S) | (a2 << (32 - S));
                a2 = (a2 >> S) | (a3 << (32 - S));
                a3 = (a3 >> S) | (bits << (32 - S));
            }
            if (i % R == 0 || i == n) pblk[(size_t)((i - 1) / R) * WAVE + lane] = make_uint4(a0, a1, a2, a3);
        }
    }
    if constexpr (FREE_END) {
        // the smallest value of row n and the smallest column that attains it
        const int jb = n + lo + k0;
        int best = INF;
#pragma unroll
        for (int x = 0; x < C; ++x) best = imin(best, (unsigned)(jb + x) <= (unsigned)t ? D[x] : INF);
        int vmin = best;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) vmin = imin(vmin, __shfl_xor(vmin, d));
        int at = INF;
#pragma unroll
        for (int x = C - 1; x >= 0; --x) at = ((unsigned)(jb + x) <= (unsigned)t && D[x] == vmin) ? k0 + x : at;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) at = imin(at, __shfl_xor(at, d));
        // every lane holds both results: say so, and the caller's walk on lane 0 stays in scalar registers
        vmin = __builtin_amdgcn_readfirstlane(vmin);
        kend = __builtin_amdgcn_readfirstlane(at);
        if (vmin > imin(w, max_dist)) return w >= max_dist ? NRA_CONS_LEFT_OUT : NRA_CONS_WIDEN;
        return vmin;
    }
    // D[n][t] is band column delta - lo
    kend = delta - lo;
    int mine = 0;
#pragma unroll
    for (int x = 0; x < C; ++x) mine |= D[x] & -(int)(x == kend % C);
    const int dist = __shfl(mine, kend / C);
    if (dist > imin(w, max_dist)) return w >= max_dist ? NRA_CONS_LEFT_OUT : NRA_CONS_WIDEN;
    return dist;
}

// One lane's walk back.  cons_walk_op: the step out of cell (i, j) on band column k (0 diagonal, 1 insertion,
// 2 deletion; the borders decide for themselves); cons_walk_base: the code of tract base i - 1.  Both fetch 16-byte
// pieces and keep the last one in (have, pw) / (have_s, sw), which start at -1 and zero.
template <int C>
__device__ __forceinline__ uint32_t cons_walk_op(const uint4* __restrict__ pblk, int n, int i, int j, int& k,
                                                 long long& have, uint4& pw)
{
    constexpr int B = WAVE * C, S = 2 * C, R = 128 / S;
    if (i == 0) return 2u;
    if (j == 0) return 1u;
    const int blk = (i - 1) / R, rr = (i - 1) % R;
    k = imin(imax(k, 0), B - 1);                                 // a proven path never leaves the band
    const long long key = (long long)blk * WAVE + k / C;
    if (key != have) {
        pw = pblk[key];
        have = key;
    }
    const int q = imin(R, n - blk * R);                          // rows of this block (the last one may be short)
    const int off = (rr + R - q) * S + 2 * (k % C);
    const uint32_t word = (off >> 5) == 0 ? pw.x : (off >> 5) == 1 ? pw.y : (off >> 5) == 2 ? pw.z : pw.w;
    return (word >> (off & 31)) & 3u;
}

__device__ __forceinline__ int cons_walk_base(const uint8_t* __restrict__ s, int i, long long& have_s, uint4& sw)
{
    const long long ks = (i - 1) >> 4;
    if (ks != have_s) {
        sw = *reinterpret_cast<const uint4*>(s + ks * 16);
        have_s = ks;
    }
    return (int)cons_byte(sw, (i - 1) & 15);
}

#endif  // NRA_CONS_DP_H
