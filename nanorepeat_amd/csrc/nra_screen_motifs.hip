// nra_screen_motifs.hip -- motif screen of unaligned reads (gfx950): which motif classes a read is made of.
//
//   k_screen_motifs  the tiles, the staging into LDS and the 16 positions per lane of k_screen_hits (nra_screen.hip), on
//                    the same device copy of the chunk.  Each lane rolls the forward code only; a valid window whose
//                    smallest period q is in 1..6 indexes the class table with the low 2q bits of its code (a rotation of
//                    the root): no canonical form, no hash, no postings.  The table (NRA_MOTIF_TAB_ENTRIES uint16) is read
//                    from memory on periodic windows only.  A lane sums the windows of a run of one class in a register
//                    and adds the sum to a small LDS map when the class changes; the map's counters leave as
//                    (read, class, count) entries with one global reservation per workgroup.  A class that finds the map
//                    full leaves as an entry of its own per sum: the host sums entries per (read, class) either way.
// The rule it implements (periodic windows, classes, m(r, C)) is DESIGN.md section 23.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(36)

#define MOTIFS_PER_LANE (NRA_SCREEN_TILE / NRA_SCREEN_THREADS)
#define MOTIFS_STAGE_U4 ((NRA_SCREEN_TILE + 15 + 15 + 15) / 16)   // tile + k - 1 (k <= 15) + alignment shift, in 16-byte units
#define MOTIFS_MAP_FREE 0xffffffffu

static_assert(NRA_SCREEN_TILE % NRA_SCREEN_THREADS == 0, "whole positions per lane");
static_assert((NRA_SCREEN_MAP & (NRA_SCREEN_MAP - 1)) == 0, "the LDS map is a power of two");
static_assert(NRA_SCREEN_MAP <= NRA_SCREEN_THREADS, "one lane per map counter at the flush");

__device__ __forceinline__ int motifs_code(uint32_t ch)
{
    const uint32_t u = ch & 0xDFu;              // lowercase ACGT -> uppercase; no other byte becomes one of them
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}

// count n windows of class `cls` for this tile's read
__device__ __forceinline__ void motifs_add(uint32_t* mkey, uint32_t* mval, uint32_t cls, uint32_t n, int32_t read,
                                           NraScreenEntry* entries, unsigned long long cap, unsigned long long* count)
{
    uint32_t h = (cls * 2654435761u) & (NRA_SCREEN_MAP - 1);
    for (int p = 0; p < NRA_SCREEN_MAP; ++p) {
        const uint32_t prev = atomicCAS(&mkey[h], MOTIFS_MAP_FREE, cls);
        if (prev == MOTIFS_MAP_FREE || prev == cls) {
            atomicAdd(&mval[h], n);
            return;
        }
        h = (h + 1) & (NRA_SCREEN_MAP - 1);
    }
    // the map is full: this sum becomes an entry of its own
    const unsigned long long at = atomicAdd(count, 1ull);
    if (at < cap) entries[at] = NraScreenEntry{read, (int32_t)cls, (int32_t)n};
}

__global__ __launch_bounds__(NRA_SCREEN_THREADS) void k_screen_motifs(
    const NraScreenTile* __restrict__ tiles, const uint8_t* __restrict__ seqs, int k,
    const uint16_t* __restrict__ class_tab, NraScreenEntry* __restrict__ entries, unsigned long long cap,
    unsigned long long* count)
{
    __shared__ uint4 stage[MOTIFS_STAGE_U4];
    __shared__ uint32_t mkey[NRA_SCREEN_MAP];
    __shared__ uint32_t mval[NRA_SCREEN_MAP];
    __shared__ uint32_t n_out;
    __shared__ unsigned long long out_base;

    const int tid = threadIdx.x;
    const NraScreenTile t = tiles[blockIdx.x];
    for (int i = tid; i < NRA_SCREEN_MAP; i += NRA_SCREEN_THREADS) { mkey[i] = MOTIFS_MAP_FREE; mval[i] = 0; }
    if (tid == 0) n_out = 0;

    // stage bytes [base, base + n_win + k - 1) from the 16-byte boundary below base, as k_screen_hits does
    const int64_t lo = t.base & ~(int64_t)15;
    const int shift = (int)(t.base - lo);
    const int n16 = (shift + t.n_win + k - 1 + 15) / 16;
    const uint4* src = reinterpret_cast<const uint4*>(seqs + lo);
    for (int i = tid; i < n16; i += NRA_SCREEN_THREADS) stage[i] = src[i];
    __syncthreads();

    const uint8_t* s = reinterpret_cast<const uint8_t*>(stage) + shift;
    const int p0 = tid * MOTIFS_PER_LANE;
    const int p1 = min(p0 + MOTIFS_PER_LANE, t.n_win);
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    uint32_t fwd = 0;
    int run = 0;
    uint32_t cur = 0, cur_n = 0;                  // class + 1 of the lane's current run of class windows, and their number
    for (int j = p0; j < p1 + k - 1; ++j) {       // the window at position i ends at byte i + k - 1
        const int c = motifs_code(s[j]);
        if (c < 0) { run = 0; continue; }
        fwd = ((fwd << 2) | (uint32_t)c) & kmask;
        if (++run < k) continue;
        // period q: the first k - q bases equal the last k - q; the smallest one wins
        int q = 0;
#pragma unroll
        for (int p = NRA_MOTIF_MAX_ROOT; p >= 1; --p)
            q = ((fwd ^ (fwd >> (2 * p))) & (kmask >> (2 * p))) == 0 ? p : q;
        uint32_t cls = 0;
        if (q) cls = class_tab[((1u << (2 * q)) - 4u) / 3u + (fwd & ((1u << (2 * q)) - 1u))];
        if (cls != cur) {
            if (cur) motifs_add(mkey, mval, cur - 1, cur_n, t.read, entries, cap, count);
            cur = cls; cur_n = 0;
        }
        ++cur_n;
    }
    if (cur) motifs_add(mkey, mval, cur - 1, cur_n, t.read, entries, cap, count);
    __syncthreads();

    // the map's counters: one reservation for the workgroup
    uint32_t mine = 0;
    const bool has = tid < NRA_SCREEN_MAP && mval[tid] != 0;
    if (has) mine = atomicAdd(&n_out, 1u);
    __syncthreads();
    if (tid == 0) out_base = n_out ? atomicAdd(count, (unsigned long long)n_out) : 0ull;
    __syncthreads();
    if (has) {
        const unsigned long long at = out_base + mine;
        if (at < cap) entries[at] = NraScreenEntry{t.read, (int32_t)mkey[tid], (int32_t)mval[tid]};
    }
}

extern "C" int nra_launch_screen_motifs(hipStream_t st, int64_t n_tiles, const NraScreenTile* tiles, const uint8_t* seqs,
                                        int k, const uint16_t* class_tab, NraScreenEntry* entries,
                                        unsigned long long cap, unsigned long long* count)
{
    if (n_tiles <= 0) return (int)hipSuccess;
    k_screen_motifs<<<dim3((unsigned)n_tiles), NRA_SCREEN_THREADS, 0, st>>>(tiles, seqs, k, class_tab, entries, cap, count);
    return (int)hipGetLastError();
}

#endif  // part 36
