// nra_consensus.hip -- allele consensus: banded unit-cost alignment of tracts to their group's backbone, column votes,
// and the next backbone (gfx950).
//
//   k_cons_align<C>  one wave per tract.  The band holds 64 C diagonals; lane l owns the C consecutive diagonals
//                    k = l C .. l C + C - 1 (k = j - i - lo) in registers.  In diagonal coordinates the diagonal
//                    predecessor of a cell is the lane's own cell of the row before, the insertion predecessor is cell
//                    k + 1 of the row before (one cross-lane shift per row), and the deletions of a row are
//                    D[k] = k + prefix-min(T[k'] - k'): serial over the lane's C cells and one wave scan in DPP steps.
//                    Two pointer bits per cell (0 diagonal, 1 insertion, 2 deletion) are shifted into a 128-bit
//                    register and leave as one 16-byte store per lane every 64 / C rows: [row block][lane], 1 KB per
//                    wave and store.  When the banded distance proves exact (include/nanorepeat_amd.h) and is at most
//                    max_dist, lane 0 walks back from (n, t) and adds the tract's votes to its group's tables with
//                    integer atomics (integer adds commute: the tables do not depend on the order).
//   k_cons_build     one wave per group: 64 backbone positions per step, each lane decides what its slot and its column
//                    emit, the output positions come from two ballots, and the wave notes whether the backbone changed.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 18 and tests/consensus_ref.py.  No floating point.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(32)

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

template <int C>
__global__ __launch_bounds__(WAVE) void k_cons_align(int n_items, const NraConsItem* __restrict__ items,
                                                     const NraConsGroup* __restrict__ groups,
                                                     const uint8_t* __restrict__ seqs,
                                                     const uint8_t* __restrict__ backbones, uint4* __restrict__ ptrs,
                                                     int32_t* __restrict__ tabs, int32_t* __restrict__ voters,
                                                     int32_t* __restrict__ status, int max_dist)
{
    constexpr int B = WAVE * C;               // diagonals of the band
    constexpr int S = 2 * C;                  // pointer bits per lane and row
    constexpr int R = 128 / S;                // rows per 16-byte piece
    constexpr int INF = NRA_CONS_INF;
    __shared__ uint8_t sb[B + CONS_TILE];
    __shared__ uint8_t ss[CONS_TILE];
    const int it = blockIdx.x;
    if (it >= n_items) return;
    const int lane = threadIdx.x;
    const NraConsItem item = items[it];
    const NraConsGroup grp = groups[item.group];
    const int n = item.n, t = grp.t;
    const int delta = t - n, ad = delta < 0 ? -delta : delta;
    const int extra = B - 1 - ad;
    if (extra < 0) {                          // the band does not hold both corners
        if (lane == 0) status[it] = NRA_CONS_WIDEN;
        return;
    }
    const int h = extra >> 1;
    const int lo = imin(0, delta) - h;        // diagonal of band column 0
    const int w = ad + 2 * h;                 // distances up to w are proven
    const uint8_t* s = seqs + item.seq;
    const uint8_t* b = backbones + grp.bb;
    uint4* pblk = ptrs + item.ptr;
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
    // D[n][t] is band column delta - lo
    const int kend = delta - lo;
    int mine = 0;
#pragma unroll
    for (int x = 0; x < C; ++x) mine |= D[x] & -(int)(x == kend % C);
    const int dist = __shfl(mine, kend / C);
    if (dist > imin(w, max_dist)) {
        if (lane == 0) status[it] = w >= max_dist ? NRA_CONS_LEFT_OUT : NRA_CONS_WIDEN;
        return;
    }
    __threadfence();                          // the other lanes' pointer stores, before lane 0 loads them
    __syncthreads();
    if (lane != 0) return;

    // ---- traceback on one lane
    int32_t* tab = tabs + grp.tab;
    int i = n, j = t, k = kend;
    long long have = -1, have_s = -1;
    uint4 pw = make_uint4(0, 0, 0, 0), sw = make_uint4(0, 0, 0, 0);
    int run_base = -1;                        // the insertion run of slot j: its base nearest the tract's start so far
    while (i > 0 || j > 0) {
        uint32_t op;
        if (i == 0) {
            op = 2u;
        } else if (j == 0) {
            op = 1u;
        } else {
            const int blk = (i - 1) / R, rr = (i - 1) % R;
            k = imin(imax(k, 0), B - 1);                         // a proven path never leaves the band
            const long long key = (long long)blk * WAVE + k / C;
            if (key != have) {
                pw = pblk[key];
                have = key;
            }
            const int q = imin(R, n - blk * R);                  // rows of this block (the last one may be short)
            const int off = (rr + R - q) * S + 2 * (k % C);
            const uint32_t word = (off >> 5) == 0 ? pw.x : (off >> 5) == 1 ? pw.y : (off >> 5) == 2 ? pw.z : pw.w;
            op = (word >> (off & 31)) & 3u;
        }
        int base = 0;
        if (op != 2u) {
            const long long ks = (i - 1) >> 4;
            if (ks != have_s) {
                sw = *reinterpret_cast<const uint4*>(s + ks * 16);
                have_s = ks;
            }
            base = (int)cons_byte(sw, (i - 1) & 15);
        }
        if (op == 1u) {
            run_base = base;
            --i;
            ++k;
            continue;
        }
        if (run_base >= 0) {
            if (run_base < 4) atomicAdd(tab + (size_t)j * NRA_CONS_TAB + 5 + run_base, 1);
            run_base = -1;
        }
        if (op == 0u) {
            if (base < 4) atomicAdd(tab + (size_t)(j - 1) * NRA_CONS_TAB + base, 1);
            --i;
            --j;
        } else {
            atomicAdd(tab + (size_t)(j - 1) * NRA_CONS_TAB + 4, 1);
            --j;
            --k;
        }
    }
    if (run_base >= 0 && run_base < 4) atomicAdd(tab + 5 + run_base, 1);      // a run that ends in slot 0
    atomicAdd(voters + item.group, 1);
    status[it] = dist;
}

__global__ __launch_bounds__(WAVE) void k_cons_build(int n_groups, const NraConsGroup* __restrict__ groups,
                                                     const uint8_t* __restrict__ backbones,
                                                     const int32_t* __restrict__ tabs,
                                                     const int32_t* __restrict__ voters,
                                                     uint8_t* __restrict__ new_backbones, int32_t* __restrict__ support,
                                                     int32_t* __restrict__ res)
{
    const int g = blockIdx.x;
    if (g >= n_groups) return;
    const int lane = threadIdx.x;
    const NraConsGroup grp = groups[g];
    const int t = grp.t, mv = voters[g];
    if (mv == 0) {                            // nobody voted: the host keeps the backbone it has
        if (lane == 0) { res[3 * g] = t; res[3 * g + 1] = 0; res[3 * g + 2] = 0; }
        return;
    }
    const uint8_t* b = backbones + grp.bb;
    const int32_t* tab = tabs + grp.tab;
    uint8_t* nb = new_backbones + grp.nb;
    int32_t* sup = support + grp.nb;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
    bool changed = false;
    for (int j0 = 0; j0 <= t; j0 += WAVE) {
        const int j = j0 + lane;
        bool e1 = false, e2 = false;
        int c1 = 0, s1 = 0, c2 = 0, s2 = 0;
        if (j <= t) {
            const int32_t* row = tab + (size_t)j * NRA_CONS_TAB;
            int tot = 0;
            for (int c = 0; c < 4; ++c) {
                const int v = row[5 + c];
                tot += v;
                if (v > s1) { s1 = v; c1 = c; }                  // a tie keeps the smaller code
            }
            e1 = 2 * tot > mv;
            if (j < t) {
                const int own = b[j];
                int mx = row[0];
                for (int c = 1; c < 5; ++c) mx = imax(mx, row[c]);
                c2 = 4;
                for (int c = 4; c >= 0; --c) c2 = row[c] == mx ? c : c2;      // the smallest tied code, deleted last
                if (row[own] == mx) c2 = own;
                s2 = mx;
                e2 = c2 != 4;
            }
        }
        const unsigned long long m1 = __ballot(e1), m2 = __ballot(e2);
        int pos = base + __popcll(m1 & below) + __popcll(m2 & below);
        if (e1) {
            nb[pos] = (uint8_t)c1;
            sup[pos] = s1;
            changed |= pos >= t || b[pos] != c1;
            ++pos;
        }
        if (e2) {
            nb[pos] = (uint8_t)c2;
            sup[pos] = s2;
            changed |= pos >= t || b[pos] != c2;
        }
        base += __popcll(m1) + __popcll(m2);
    }
    const bool any = __ballot(changed) != 0ull || base != t;
    if (lane == 0) { res[3 * g] = base; res[3 * g + 1] = any ? 1 : 0; res[3 * g + 2] = mv; }
}

template <int C>
static int launch_cons_align(hipStream_t st, int n_items, const NraConsItem* items, const NraConsGroup* groups,
                             const uint8_t* seqs, const uint8_t* backbones, uint4* ptrs, int32_t* tabs, int32_t* voters,
                             int32_t* status, int max_dist)
{
    k_cons_align<C><<<dim3((unsigned)n_items), WAVE, 0, st>>>(n_items, items, groups, seqs, backbones, ptrs, tabs, voters,
                                                             status, max_dist);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_cons_align(hipStream_t st, int c, int n_items, const NraConsItem* items,
                                     const NraConsGroup* groups, const uint8_t* seqs, const uint8_t* backbones,
                                     uint4* ptrs, int32_t* tabs, int32_t* voters, int32_t* status, int max_dist)
{
    if (n_items <= 0) return (int)hipSuccess;
    switch (c) {
    case 1: return launch_cons_align<1>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 2: return launch_cons_align<2>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 4: return launch_cons_align<4>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 8: return launch_cons_align<8>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    case 16: return launch_cons_align<16>(st, n_items, items, groups, seqs, backbones, ptrs, tabs, voters, status, max_dist);
    default: return (int)hipErrorInvalidValue;
    }
}

extern "C" int nra_launch_cons_build(hipStream_t st, int n_groups, const NraConsGroup* groups, const uint8_t* backbones,
                                     const int32_t* tabs, const int32_t* voters, uint8_t* new_backbones, int32_t* support,
                                     int32_t* res)
{
    if (n_groups <= 0) return (int)hipSuccess;
    k_cons_build<<<dim3((unsigned)n_groups), WAVE, 0, st>>>(n_groups, groups, backbones, tabs, voters, new_backbones,
                                                           support, res);
    return (int)hipGetLastError();
}

#endif  // part 32
