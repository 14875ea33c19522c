// nra_scan.hip -- catalogue-free scan of unaligned reads (gfx950): where in a read the tandem runs lie.
//
//   k_scan_repeats  the tiles, the staging into LDS and the 16 positions per lane of k_screen_hits (nra_screen.hip).  Each
//                   lane rolls the forward code only and tests the periods 6..1 without a branch, as k_screen_motifs does;
//                   a periodic window indexes the table of every primitive p-mer (NRA_MOTIF_TAB_ENTRIES uint16, an entry is
//                   (class id + 1) << 1 | reverse) with the low 2q bits of its code.  The lane keeps its 16 entries in
//                   registers.  The tile leaves as segments: maximal runs of consecutive windows of one entry within the
//                   tile.  A lane's first and last entry go to LDS, so that a lane knows whether its head run continues the
//                   lane below and whether its tail run goes on in the lane above; where the run that reaches a lane's end
//                   began is a maximum scan over the lanes (shuffles within a wave, four wave totals through LDS), so a
//                   tile of one class leaves as one segment.  A segment is written by the lane it ends in; the slots come
//                   from one LDS counter and one global reservation per workgroup.  The tile's number of valid windows is
//                   a plain store per tile, summed by the host: one counter for all tiles was a second atomic on one
//                   address per tile and doubled the kernel's time.  No workgroup waits for another, and every loop is
//                   bounded by the lane's 16 positions, k or the wave.
// The rule it implements (periodic windows, class ids, orientation, islands) is DESIGN.md section 29.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(41)

#define SCAN_PER_LANE (NRA_SCREEN_TILE / NRA_SCREEN_THREADS)
#define SCAN_STAGE_U4 ((NRA_SCREEN_TILE + 15 + 15 + 15) / 16)   // tile + k - 1 (k <= 15) + alignment shift, in 16-byte units
#define SCAN_WAVES (NRA_SCREEN_THREADS / 64)
#define SCAN_NO_ENTRY 0xffffffffu                                // no table entry: what lies beyond either end of the tile

static_assert(NRA_SCREEN_TILE % NRA_SCREEN_THREADS == 0, "whole positions per lane");
static_assert(NRA_SCREEN_THREADS % 64 == 0, "whole waves");
static_assert(sizeof(NraScanSegment) == sizeof(int4), "a segment leaves with one 16-byte store");

__device__ __forceinline__ int scan_code(uint32_t ch)
{
    const uint32_t u = ch & 0xDFu;              // lowercase ACGT -> uppercase; no other byte becomes one of them
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}

__global__ __launch_bounds__(NRA_SCREEN_THREADS) void k_scan_repeats(
    const NraScanTile* __restrict__ tiles, const uint8_t* __restrict__ seqs, int k,
    const uint16_t* __restrict__ class_tab, NraScanSegment* __restrict__ segments, unsigned long long cap,
    unsigned long long* count, uint32_t* __restrict__ tile_valid)
{
    __shared__ uint4 stage[SCAN_STAGE_U4];
    __shared__ uint32_t first_e[NRA_SCREEN_THREADS];
    __shared__ uint32_t last_e[NRA_SCREEN_THREADS];
    __shared__ int wave_start[SCAN_WAVES];
    __shared__ uint32_t n_out, n_valid;
    __shared__ unsigned long long out_base;

    const int tid = threadIdx.x;
    const NraScanTile t = tiles[blockIdx.x];
    if (tid == 0) { n_out = 0; n_valid = 0; }

    // stage bytes [base, base + n_win + k - 1) from the 16-byte boundary below base, as k_screen_hits does
    const int64_t lo = t.base & ~(int64_t)15;
    const int shift = (int)(t.base - lo);
    const int n16 = (shift + t.n_win + k - 1 + 15) / 16;
    const uint4* src = reinterpret_cast<const uint4*>(seqs + lo);
    for (int i = tid; i < n16; i += NRA_SCREEN_THREADS) stage[i] = src[i];
    __syncthreads();

    // bytes past the tile's last window are inside `stage` (it holds NRA_SCREEN_TILE + 45 bytes) and their windows are
    // masked by n_win
    const uint8_t* s = reinterpret_cast<const uint8_t*>(stage) + shift;
    const int p0 = tid * SCAN_PER_LANE;
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    uint32_t fwd = 0;
    int run = 0;
    for (int j = 0; j < k - 1; ++j) {             // the window at position i ends at byte i + k - 1
        const int c = scan_code(s[p0 + j]);
        run = c < 0 ? 0 : run + 1;
        fwd = ((fwd << 2) | (uint32_t)(c & 3)) & kmask;
    }
    // the lane's 16 entries; on the way, where the run that reaches the lane's end began if that is past the lane's
    // first position (else -1), and the segments that end in front of the lane's last position
    uint32_t e[SCAN_PER_LANE];
    uint32_t valid = 0, n_mine = 0;
    int tail_start = -1;
#pragma unroll
    for (int i = 0; i < SCAN_PER_LANE; ++i) {
        const int c = scan_code(s[p0 + k - 1 + i]);
        run = c < 0 ? 0 : run + 1;
        fwd = ((fwd << 2) | (uint32_t)(c & 3)) & kmask;
        const bool ok = run >= k && p0 + i < t.n_win;
        // period q: the first k - q bases equal the last k - q; the smallest one wins
        int q = 0;
#pragma unroll
        for (int p = NRA_MOTIF_MAX_ROOT; p >= 1; --p)
            q = ((fwd ^ (fwd >> (2 * p))) & (kmask >> (2 * p))) == 0 ? p : q;
        uint32_t v = 0;
        if (ok && q) v = class_tab[((1u << (2 * q)) - 4u) / 3u + (fwd & ((1u << (2 * q)) - 1u))];
        e[i] = v;
        valid += (uint32_t)__popcll(__ballot(ok));
        if (i > 0 && v != e[i - 1]) {
            tail_start = p0 + i;
            n_mine += e[i - 1] != 0 ? 1u : 0u;
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
    first_e[tid] = e[0];
    last_e[tid] = e[SCAN_PER_LANE - 1];
    if (lane == 0 && valid) atomicAdd(&n_valid, valid);
    __syncthreads();

    // the lanes below and above: does the lane's first position start a run, does its last one end a segment
    const uint32_t below = tid ? last_e[tid - 1] : SCAN_NO_ENTRY;
    const uint32_t above = tid + 1 < NRA_SCREEN_THREADS ? first_e[tid + 1] : SCAN_NO_ENTRY;
    if (tail_start < 0 && below != e[0]) tail_start = p0;
    n_mine += e[SCAN_PER_LANE - 1] != 0 && e[SCAN_PER_LANE - 1] != above ? 1u : 0u;

    // maximum scan of tail_start over the lanes: lane 0 of the tile always starts a run, so every lane gets a start
    int incl = tail_start;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, o);
    }
    if (lane == 63) wave_start[wave] = incl;
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    uint32_t mine = 0;
    if (n_mine) mine = atomicAdd(&n_out, n_mine);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w)
        if (w < wave) excl = max(excl, wave_start[w]);
    if (tid == 0) {
        out_base = n_out ? atomicAdd(count, (unsigned long long)n_out) : 0ull;
        tile_valid[blockIdx.x] = n_valid;
    }
    __syncthreads();

    // the segments that end in this lane
    if (n_mine) {
        unsigned long long at = out_base + mine;
        int start = below != e[0] ? p0 : excl;
#pragma unroll
        for (int i = 0; i < SCAN_PER_LANE; ++i) {
            if (i > 0 && e[i] != e[i - 1]) start = p0 + i;
            const uint32_t next = i + 1 < SCAN_PER_LANE ? e[i + 1] : above;
            if (e[i] != 0 && e[i] != next) {
                if (at < cap)
                    *reinterpret_cast<int4*>(&segments[at]) = make_int4(t.read, t.pos + start, p0 + i + 1 - start, (int)e[i]);
                ++at;
            }
        }
    }
}

extern "C" int nra_launch_scan_repeats(hipStream_t st, int64_t n_tiles, const NraScanTile* tiles, const uint8_t* seqs,
                                       int k, const uint16_t* class_tab, NraScanSegment* segments,
                                       unsigned long long cap, unsigned long long* count, uint32_t* tile_valid)
{
    if (n_tiles <= 0) return (int)hipSuccess;
    k_scan_repeats<<<dim3((unsigned)n_tiles), NRA_SCREEN_THREADS, 0, st>>>(tiles, seqs, k, class_tab, segments, cap, count,
                                                                          tile_valid);
    return (int)hipGetLastError();
}

#endif  // part 41
