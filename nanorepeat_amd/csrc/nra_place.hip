// nra_place.hip -- seed hits of a streamed target against a device-resident index of short queries (gfx950).
//
//   k_place_hits   one 256-thread workgroup per tile of NRA_PLACE_TILE target windows.  The tile's bytes (+ k - 1) are
//                  staged into LDS with 16-byte loads; each lane takes 16 consecutive windows, rolls the forward and
//                  reverse-complement codes over them and probes the open-addressing table with the canonical k-mer (one
//                  8-byte slot per probe).  A window whose k-mer is a key adds 1 to the key's occurrence counter and puts
//                  (slot, position, forward bit) into the workgroup's LDS list; the list leaves with one global
//                  reservation per workgroup.  A lane that reads a counter already past the ceiling does neither: the
//                  counter only has to be right up to the ceiling (a counter is past the ceiling at the end exactly when
//                  the key has more windows than the ceiling, whatever the order, and a key that is not has every one of
//                  its windows in the list).  A tile makes at most one record per window and the host sizes the global
//                  list to the windows of the launch, so no launch overflows it and none is ever run twice.
// Diagonals need the query's length and are the host's (nra_place_host.cpp).  The rule is DESIGN.md section 31.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(43)

#define PLACE_PER_LANE (NRA_PLACE_TILE / NRA_PLACE_THREADS)
#define PLACE_STAGE_U4 ((NRA_PLACE_TILE + 14 + 15) / 16)   // tile + k - 1 (k <= 15) bytes in 16-byte units

static_assert(NRA_PLACE_TILE % NRA_PLACE_THREADS == 0, "whole windows per lane");
static_assert(NRA_PLACE_TILE % 16 == 0, "a tile starts on a 16-byte boundary of the chunk's copy");

__device__ __forceinline__ int place_code(uint32_t ch)
{
    const uint32_t u = ch & 0xDFu;              // lowercase ACGT -> uppercase; no other byte becomes one of them
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}

__global__ __launch_bounds__(NRA_PLACE_THREADS) void k_place_hits(
    int64_t n_win, const uint8_t* __restrict__ seqs, int k, const uint64_t* __restrict__ table, int log2_slots,
    uint32_t* occ, uint32_t ceiling, int32_t contig, int64_t pos0, NraPlaceRecord* __restrict__ records,
    unsigned long long* count, unsigned long long* n_valid)
{
    __shared__ uint4 stage[PLACE_STAGE_U4];
    __shared__ uint2 hits[NRA_PLACE_TILE];      // slot, position << 1 | forward
    __shared__ uint32_t n_out, n_ok;
    __shared__ unsigned long long out_base;

    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)blockIdx.x * NRA_PLACE_TILE;
    const int tile_win = (int)min((int64_t)NRA_PLACE_TILE, n_win - w0);
    if (tid == 0) { n_out = 0; n_ok = 0; }

    // bytes [w0, w0 + tile_win + k - 1): w0 is a multiple of 16 and the copy is padded, so whole 16-byte pieces
    const int n16 = (tile_win + k - 1 + 15) / 16;
    const uint4* src = reinterpret_cast<const uint4*>(seqs + w0);
    for (int i = tid; i < n16; i += NRA_PLACE_THREADS) stage[i] = src[i];
    __syncthreads();

    const uint8_t* s = reinterpret_cast<const uint8_t*>(stage);
    const int p0 = tid * PLACE_PER_LANE;
    const int p1 = min(p0 + PLACE_PER_LANE, tile_win);
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    const int rshift = 2 * (k - 1);
    const uint64_t smask = (1ull << log2_slots) - 1ull;
    uint32_t fwd = 0, rev = 0, valid = 0;
    int run = 0;
    for (int j = p0; j < p1 + k - 1; ++j) {       // the window at position i ends at byte i + k - 1
        const int c = place_code(s[j]);
        if (c < 0) { run = 0; continue; }
        fwd = ((fwd << 2) | (uint32_t)c) & kmask;
        rev = (rev >> 2) | ((uint32_t)(3 - c) << rshift);
        if (++run < k) continue;
        ++valid;
        const uint32_t key = fwd < rev ? fwd : rev;
        uint64_t h = ((uint64_t)key * NRA_SCREEN_HASH_MUL) >> (64 - log2_slots);
        for (;;) {
            const uint64_t slot = table[h];
            if (slot == NRA_SCREEN_EMPTY) break;
            if ((uint32_t)(slot & ((1ull << NRA_SCREEN_KEY_BITS) - 1)) == key) {
                // a stale value is a smaller one: a lane skips only a key that is past the ceiling for good
                if (__hip_atomic_load(&occ[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= ceiling) {
                    atomicAdd(&occ[h], 1u);
                    const uint32_t at = atomicAdd(&n_out, 1u);          // < NRA_PLACE_TILE: one per window
                    const uint32_t pos = (uint32_t)(pos0 + w0 + (j - (k - 1)));
                    hits[at] = make_uint2((uint32_t)h, pos << 1 | (fwd < rev ? 1u : 0u));
                }
                break;
            }
            h = (h + 1) & smask;
        }
    }
    if (valid) atomicAdd(&n_ok, valid);
    __syncthreads();

    if (tid == 0) {
        out_base = n_out ? atomicAdd(count, (unsigned long long)n_out) : 0ull;
        if (n_ok) atomicAdd(n_valid, (unsigned long long)n_ok);
    }
    __syncthreads();
    const uint32_t n = n_out;
    for (uint32_t i = tid; i < n; i += NRA_PLACE_THREADS)
        records[out_base + i] = NraPlaceRecord{hits[i].x, contig, hits[i].y};
}

extern "C" int nra_launch_place_hits(hipStream_t st, int64_t n_win, const uint8_t* seqs, int k, const uint64_t* table,
                                     int log2_slots, uint32_t* occ, uint32_t ceiling, int32_t contig, int64_t pos0,
                                     NraPlaceRecord* records, unsigned long long* count, unsigned long long* n_valid)
{
    if (n_win <= 0) return (int)hipSuccess;
    const int64_t n_tiles = (n_win + NRA_PLACE_TILE - 1) / NRA_PLACE_TILE;
    k_place_hits<<<dim3((unsigned)n_tiles), NRA_PLACE_THREADS, 0, st>>>(n_win, seqs, k, table, log2_slots, occ, ceiling,
                                                                        contig, pos0, records, count, n_valid);
    return (int)hipGetLastError();
}

#endif  // part 43
