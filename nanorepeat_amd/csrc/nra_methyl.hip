// nra_methyl.hip -- CpG methylation per read: the MM/ML calls of a read counted over its tract and flank bins (gfx950).
//
//   k_read_methylation  one 256-thread workgroup per read, workgroups striding over the chunk's reads (sorted by length).
//                       (a) The read's deltas become the listed ranks L_j = j + d_0 + .. + d_j in place: tiles of 256,
//                           a wave scan of d_j + 1 in 64 bits by __shfl_up, the four wave totals through LDS, the tile
//                           carry in a register; a rank is stored saturated at INT32_MAX (a read has at most 4 000 000
//                           C, so a saturated rank matches none and still says "beyond n_c").
//                       (b) One pass over the read in tiles of 256 bases in the order of the sequenced strand O -- that
//                           is backwards through the stored bytes S when the read is stored reversed.  A base is a C of
//                           O when its stored byte is C (forward) or G (reversed); a wave ranks its 64 bases with a
//                           ballot of that and a popcount below the lane, the four wave counts go through LDS and the
//                           tile carry stays in a register.  Each thread loads its own byte and the next byte in O
//                           order (the one-base halo across lane, wave and tile edges is that second load; both are
//                           issued one tile ahead).  The C of a site (stored CG) that falls in the tract or a flank bin
//                           looks its rank up in L by binary search (L ascends) and adds its call to the segment's five
//                           counters in LDS with integer atomics: integer adds commute, the order does not matter.
//                       The two LDS hand-offs are double-buffered by tile parity: one barrier per tile.  The counters,
//                       n_c and the status leave once per read; a list that reaches beyond n_c zeroes the counters.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 28 and tests/methylation_ref.py.
#include "nanorepeat_amd.h"
#include "nra_device.h"

#include <climits>

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(40)

#define METH_WAVES (NRA_METH_THREADS / WAVE)
#define METH_ROWS (2 * NRA_METH_MAX_BINS + 1)

// position i of O (i < n, else two zero bytes): the stored byte there and the stored byte of position i + 1
__device__ __forceinline__ void meth_load(const uint8_t* __restrict__ S, int n, bool rev, int i, int& own, int& next)
{
    own = 0;
    next = 0;
    if (i < n) {
        const int t = rev ? n - 1 - i : i, q = rev ? t - 1 : t + 1;
        own = S[t];
        if (q >= 0 && q < n) next = S[q];
    }
}

__global__ __launch_bounds__(NRA_METH_THREADS) void k_read_methylation(
    int n_reads, const NraMethRead* __restrict__ reads, const uint8_t* __restrict__ seqs, int32_t* ranks,
    const uint8_t* __restrict__ probs, int flank, int bin, int nb, int lo_byte, int hi_byte,
    int32_t* __restrict__ counts, int32_t* __restrict__ n_c, int32_t* __restrict__ status)
{
    __shared__ long long s_scan[2][METH_WAVES];
    __shared__ int s_cnt[2][METH_WAVES];
    __shared__ int s_seg[METH_ROWS * NRA_METH_COUNTERS];
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int cells = (2 * nb + 1) * NRA_METH_COUNTERS;
    int par = 0;
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const NraMethRead rd = reads[r];
        const int n = rd.n;
        const bool rev = (rd.flags & NRA_METH_F_REVERSED) != 0, implicit = (rd.flags & NRA_METH_F_IMPLICIT) != 0;
        const bool too_many = (rd.flags & NRA_METH_F_TOO_MANY) != 0;
        const int m = too_many ? 0 : rd.m;
        int32_t* L = ranks + rd.mod;
        const uint8_t* pr = probs + rd.mod;
        const uint8_t* S = seqs + rd.seq;
        for (int i = tid; i < cells; i += NRA_METH_THREADS) s_seg[i] = 0;

        // (a) L_j = (d_0 + 1) + .. + (d_j + 1) - 1
        long long carry = -1;
        for (int j0 = 0; j0 < m; j0 += NRA_METH_THREADS, par ^= 1) {
            const int j = j0 + tid;
            long long v = j < m ? (long long)L[j] + 1 : 0;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const long long u = __shfl_up(v, o);
                if (lane >= o) v += u;
            }
            if (lane == WAVE - 1) s_scan[par][wave] = v;
            __syncthreads();
            long long before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < METH_WAVES; ++w) {
                const long long t = s_scan[par][w];
                total += t;
                if (w < wave) before += t;
            }
            if (j < m) {
                const long long rank = carry + before + v;
                L[j] = rank < (long long)INT_MAX ? (int32_t)rank : INT_MAX;
            }
            carry += total;
        }
        __syncthreads();                       // the ranks and the cleared counters, before any thread uses them

        // (b) the C of O, ranked; the sites among them, looked up and counted
        const int c_byte = rev ? 'G' : 'C', g_byte = rev ? 'C' : 'G';     // a C of O and the G after it, as stored
        int c_before = 0;                                                 // C of O in the tiles done
        int own, next;
        meth_load(S, n, rev, tid, own, next);
        for (int i0 = 0; i0 < n; i0 += NRA_METH_THREADS, par ^= 1) {
            const int i = i0 + tid;
            int own2, next2;
            meth_load(S, n, rev, i + NRA_METH_THREADS, own2, next2);
            const bool is_c = (own & 0xDF) == c_byte;                     // 0 beyond the read: not a C
            const unsigned long long bal = __ballot(is_c);
            if (lane == 0) s_cnt[par][wave] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < METH_WAVES; ++w) {
                const int t = s_cnt[par][w];
                total += t;
                if (w < wave) before += t;
            }
            if (is_c && (next & 0xDF) == g_byte) {
                const int t = rev ? n - 1 - i : i, s = rev ? t - 1 : t;   // the site's stored index
                int seg = -1;
                if (rd.lo <= s && s + 2 <= rd.hi) seg = nb;
                else if (s + 2 <= rd.lo) {
                    const int d = rd.lo - s - 2;
                    if (d < flank) seg = d / bin;
                } else if (s >= rd.hi) {
                    const int d = s - rd.hi;
                    if (d < flank) seg = nb + 1 + d / bin;
                }
                if (seg >= 0) {
                    const int rank = c_before + before + __popcll(bal & ((1ull << lane) - 1ull));
                    int a = 0, b = m;                                     // the first j with L_j >= rank
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (L[mid] < rank) a = mid + 1;
                        else b = mid;
                    }
                    int call = implicit ? 0 : -1;
                    if (a < m && L[a] == rank) call = pr[a];
                    int* c = s_seg + seg * NRA_METH_COUNTERS;
                    atomicAdd(c, 1);
                    if (call >= 0) {
                        atomicAdd(c + 1, 1);
                        if (call >= hi_byte) atomicAdd(c + 2, 1);
                        if (call <= lo_byte) atomicAdd(c + 3, 1);
                        if (call > 0) atomicAdd(c + 4, call);
                    }
                }
            }
            c_before += total;
            own = own2;
            next = next2;
        }
        __syncthreads();                       // every site counted
        const bool bad = too_many || (m > 0 && L[m - 1] >= c_before);
        int32_t* out = counts + (int64_t)r * cells;
        for (int i = tid; i < cells; i += NRA_METH_THREADS) out[i] = bad ? 0 : s_seg[i];
        if (tid == 0) {
            n_c[r] = c_before;
            status[r] = bad ? NRA_METH_BAD_TAG : NRA_METH_OK;
        }
        __syncthreads();                       // the counters are read before the next read clears them
    }
}

extern "C" int nra_launch_read_methylation(hipStream_t st, int n_grid, int n_reads, const NraMethRead* reads,
                                           const uint8_t* seqs, int32_t* ranks, const uint8_t* probs, int flank,
                                           int bin, int nb, int lo_byte, int hi_byte, int32_t* counts, int32_t* n_c,
                                           int32_t* status)
{
    if (n_reads <= 0) return (int)hipSuccess;
    k_read_methylation<<<dim3((unsigned)n_grid), NRA_METH_THREADS, 0, st>>>(n_reads, reads, seqs, ranks, probs, flank,
                                                                             bin, nb, lo_byte, hi_byte, counts, n_c,
                                                                             status);
    return (int)hipGetLastError();
}

#endif  // part 40
