// nra_screen.hip -- anchor k-mer screen of unaligned reads (gfx950).
//
//   k_screen_hits  one 256-thread workgroup per tile of NRA_SCREEN_TILE window positions of one read.  The tile's bytes
//                  (+ k - 1) are staged into LDS with 16-byte loads; each lane takes 16 consecutive positions, rolls the
//                  forward and reverse-complement codes over them, probes the open-addressing index with the canonical
//                  k-mer (one 8-byte slot per probe) and, on a hit, adds 1 to every (region, side) set of its postings in
//                  a small LDS map.  The map's non-zero counters leave as (read, set, count) entries with one global
//                  reservation per workgroup.  A set that finds the map full is counted with one entry per hit instead
//                  (a global reservation each): the host sums entries per (read, set) either way.
// The rule it implements (windows, canonical k-mers, sets, counts) is DESIGN.md section 13.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(27)

#define SCREEN_PER_LANE (NRA_SCREEN_TILE / NRA_SCREEN_THREADS)
#define SCREEN_STAGE_U4 ((NRA_SCREEN_TILE + 15 + 15 + 15) / 16)   // tile + k - 1 (k <= 15) + alignment shift, in 16-byte units
#define SCREEN_MAP_FREE 0xffffffffu

static_assert(NRA_SCREEN_TILE % NRA_SCREEN_THREADS == 0, "whole positions per lane");
static_assert((NRA_SCREEN_MAP & (NRA_SCREEN_MAP - 1)) == 0, "the LDS map is a power of two");

__device__ __forceinline__ int screen_code(uint32_t ch)
{
    const uint32_t u = ch & 0xDFu;              // lowercase ACGT -> uppercase; no other byte becomes one of them
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}

// count one hit of `set` for this tile's read
__device__ __forceinline__ void screen_add(uint32_t* mkey, uint32_t* mval, uint32_t set, int32_t read,
                                           NraScreenEntry* entries, unsigned long long cap, unsigned long long* count)
{
    uint32_t h = (set * 2654435761u) & (NRA_SCREEN_MAP - 1);
    for (int p = 0; p < NRA_SCREEN_MAP; ++p) {
        const uint32_t prev = atomicCAS(&mkey[h], SCREEN_MAP_FREE, set);
        if (prev == SCREEN_MAP_FREE || prev == set) {
            atomicAdd(&mval[h], 1u);
            return;
        }
        h = (h + 1) & (NRA_SCREEN_MAP - 1);
    }
    // the map is full: this hit becomes an entry of its own
    const unsigned long long at = atomicAdd(count, 1ull);
    if (at < cap) entries[at] = NraScreenEntry{read, (int32_t)set, 1};
}

__global__ __launch_bounds__(NRA_SCREEN_THREADS) void k_screen_hits(
    const NraScreenTile* __restrict__ tiles, const uint8_t* __restrict__ seqs, int k,
    const uint64_t* __restrict__ table, int log2_slots, const uint32_t* __restrict__ postings,
    NraScreenEntry* __restrict__ entries, unsigned long long cap, unsigned long long* count)
{
    __shared__ uint4 stage[SCREEN_STAGE_U4];
    __shared__ uint32_t mkey[NRA_SCREEN_MAP];
    __shared__ uint32_t mval[NRA_SCREEN_MAP];
    __shared__ uint32_t n_out;
    __shared__ unsigned long long out_base;

    const int tid = threadIdx.x;
    const NraScreenTile t = tiles[blockIdx.x];
    for (int i = tid; i < NRA_SCREEN_MAP; i += NRA_SCREEN_THREADS) { mkey[i] = SCREEN_MAP_FREE; mval[i] = 0; }
    if (tid == 0) n_out = 0;

    // stage bytes [base, base + n_win + k - 1) from the 16-byte boundary below base (the host pads the chunk's copy so
    // that the last 16-byte piece stays inside the allocation)
    const int64_t lo = t.base & ~(int64_t)15;
    const int shift = (int)(t.base - lo);
    const int n16 = (shift + t.n_win + k - 1 + 15) / 16;
    const uint4* src = reinterpret_cast<const uint4*>(seqs + lo);
    for (int i = tid; i < n16; i += NRA_SCREEN_THREADS) stage[i] = src[i];
    __syncthreads();

    const uint8_t* s = reinterpret_cast<const uint8_t*>(stage) + shift;
    const int p0 = tid * SCREEN_PER_LANE;
    const int p1 = min(p0 + SCREEN_PER_LANE, t.n_win);
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    const int rshift = 2 * (k - 1);
    const uint64_t smask = (1ull << log2_slots) - 1ull;
    uint32_t fwd = 0, rev = 0;
    int run = 0;
    for (int j = p0; j < p1 + k - 1; ++j) {       // the window at position i ends at byte i + k - 1
        const int c = screen_code(s[j]);
        if (c < 0) { run = 0; continue; }
        fwd = ((fwd << 2) | (uint32_t)c) & kmask;
        rev = (rev >> 2) | ((uint32_t)(3 - c) << rshift);
        if (++run < k) continue;
        const uint32_t key = fwd < rev ? fwd : rev;
        uint64_t h = ((uint64_t)key * NRA_SCREEN_HASH_MUL) >> (64 - log2_slots);
        for (;;) {
            const uint64_t slot = table[h];
            if (slot == NRA_SCREEN_EMPTY) break;
            if ((uint32_t)(slot & ((1ull << NRA_SCREEN_KEY_BITS) - 1)) == key) {
                const uint32_t n = (uint32_t)(slot >> NRA_SCREEN_KEY_BITS) & ((1u << NRA_SCREEN_CNT_BITS) - 1);
                const uint32_t first = (uint32_t)(slot >> (NRA_SCREEN_KEY_BITS + NRA_SCREEN_CNT_BITS));
                for (uint32_t q = 0; q < n; ++q) screen_add(mkey, mval, postings[first + q], t.read, entries, cap, count);
                break;
            }
            h = (h + 1) & smask;
        }
    }
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

static_assert(NRA_SCREEN_MAP <= NRA_SCREEN_THREADS, "one lane per map counter at the flush");

extern "C" int nra_launch_screen_hits(hipStream_t st, int64_t n_tiles, const NraScreenTile* tiles, const uint8_t* seqs,
                                      int k, const uint64_t* table, int log2_slots, const uint32_t* postings,
                                      NraScreenEntry* entries, unsigned long long cap, unsigned long long* count)
{
    if (n_tiles <= 0) return (int)hipSuccess;
    k_screen_hits<<<dim3((unsigned)n_tiles), NRA_SCREEN_THREADS, 0, st>>>(tiles, seqs, k, table, log2_slots, postings,
                                                                         entries, cap, count);
    return (int)hipGetLastError();
}

#endif  // part 27
