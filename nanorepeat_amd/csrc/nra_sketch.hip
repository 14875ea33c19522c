// nra_sketch.hip -- k-mer sketches of short sequences and the pairs of sequences that share k-mers (gfx950).
//
//   k_sketch        one 256-thread workgroup per sequence of at most NRA_SKETCH_MAX_LEN bases.  The bytes are staged into
//                   LDS with 16-byte loads from the 16-byte boundary below the sequence, as k_screen_hits does.  Each
//                   lane rolls the forward and the reverse-complement code over its 8 window positions; a window that is
//                   not valid, lies past the sequence or is periodic (period 1..6, the test of k_screen_motifs on the
//                   forward code: a window and its reverse complement have the same periods) becomes NRA_SKETCH_EMPTY,
//                   every other one min(forward, reverse).  The slots are sorted in LDS (bitonic, over the power of two
//                   that holds the sequence's windows, not always all 2048 slots), duplicates drop out by a compare with
//                   the slot below, and the kept slots leave in ascending order through a prefix scan over the lanes.
//   k_sketch_pairs  one workgroup per tile: sequence i against up to NRA_SKETCH_BLOCK later sequences of its group.
//                   The tile list is implicit: position s of the sorted order owns the tiles [tile_first[s],
//                   tile_first[s + 1]), and a workgroup finds its position by a bisection of tile_first (at the group
//                   limit an explicit list would hold 33 M tiles).  Sketch i goes into an open-addressing set of
//                   NRA_SKETCH_SET_SLOTS uint32 in LDS, at most half full.  Each wave takes the j's of the block in turn;
//                   its lanes probe j's entries strided, four loads ahead of the probes, and the wave sums the lanes'
//                   hits.  A pair at or over min_shared is appended through an LDS counter and the tile's pairs leave
//                   with one global reservation per workgroup.  No workgroup waits for another; every loop is bounded
//                   by the sequence, the set or the block; plain C++ with vector stores.
// The contract is DESIGN.md section 30.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(42)

#define SK_PER_LANE (NRA_SKETCH_MAX_LEN / NRA_SKETCH_THREADS)
#define SK_STAGE_U4 ((NRA_SKETCH_MAX_LEN + 15 + 15 + 15) / 16 + 1)   // sequence + k - 1 (k <= 15) + alignment shift
#define SK_WAVES (NRA_SKETCH_THREADS / 64)
#define SK_UNROLL 4                                                  // entries of j a lane loads before it probes

static_assert(NRA_SKETCH_MAX_LEN % NRA_SKETCH_THREADS == 0, "whole positions per lane");
static_assert(NRA_SKETCH_THREADS % 64 == 0, "whole waves");
static_assert(NRA_SKETCH_SET_SLOTS >= 2 * NRA_SKETCH_MAX_LEN, "the set is at most half full");
static_assert((NRA_SKETCH_SET_SLOTS & (NRA_SKETCH_SET_SLOTS - 1)) == 0, "the set's slots are a power of two");
static_assert(sizeof(NraSketchPair) == sizeof(int4), "a pair leaves with one 16-byte store");

__device__ __forceinline__ int sketch_code(uint32_t ch)
{
    const uint32_t u = ch & 0xDFu;              // lowercase ACGT -> uppercase; no other byte becomes one of them
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : -1;
}

__global__ __launch_bounds__(NRA_SKETCH_THREADS) void k_sketch(
    const uint8_t* __restrict__ seqs, const int64_t* __restrict__ seq_base, const int32_t* __restrict__ seq_len, int k,
    const int64_t* __restrict__ sk_off, uint32_t* __restrict__ sketch, int32_t* __restrict__ sk_len,
    int32_t* __restrict__ n_valid)
{
    __shared__ uint4 stage[SK_STAGE_U4];
    __shared__ uint32_t slot[NRA_SKETCH_MAX_LEN];
    __shared__ uint32_t wave_kept[SK_WAVES], wave_valid[SK_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = seq_base[blockIdx.x];
    const int len = seq_len[blockIdx.x];
    const int n_win = len >= k ? len - k + 1 : 0;
    if (n_win == 0) {                             // uniform over the workgroup
        if (tid == 0) { sk_len[blockIdx.x] = 0; n_valid[blockIdx.x] = 0; }
        return;
    }

    const int64_t lo = base & ~(int64_t)15;
    const int shift = (int)(base - lo);
    const int n16 = (shift + len + 15) / 16;      // at most (15 + 2048 + 15) / 16 = 129 < SK_STAGE_U4
    const uint4* src = reinterpret_cast<const uint4*>(seqs + lo);
    for (int i = tid; i < n16; i += NRA_SKETCH_THREADS) stage[i] = src[i];
    __syncthreads();

    // slots [0, n_sort): n_sort = the power of two that holds n_win, at least 2 * 64 so that every step below has work
    // for whole waves; the lanes whose 8 positions lie past n_sort hold nothing
    int n_sort = 128;
    while (n_sort < n_win) n_sort <<= 1;

    // bytes past the sequence's end are inside `stage` and their windows are masked by n_win
    const uint8_t* s = reinterpret_cast<const uint8_t*>(stage) + shift;
    const int p0 = tid * SK_PER_LANE;
    uint32_t valid = 0;
    if (p0 < n_sort) {
        const uint32_t kmask = (1u << (2 * k)) - 1u;
        const int top = 2 * (k - 1);
        uint32_t fwd = 0, rev = 0;
        int run = 0;
        const bool inside = p0 < n_win;
        for (int j = 0; j < k - 1; ++j) {         // the window at position i ends at byte i + k - 1
            const int c = inside ? sketch_code(s[p0 + j]) : -1;
            run = c < 0 ? 0 : run + 1;
            fwd = ((fwd << 2) | (uint32_t)(c & 3)) & kmask;
            rev = (rev >> 2) | ((uint32_t)(3 - (c & 3)) << top);
        }
#pragma unroll
        for (int i = 0; i < SK_PER_LANE; ++i) {
            const bool in = p0 + i < n_win;
            const int c = in ? sketch_code(s[p0 + k - 1 + i]) : -1;
            run = c < 0 ? 0 : run + 1;
            fwd = ((fwd << 2) | (uint32_t)(c & 3)) & kmask;
            rev = (rev >> 2) | ((uint32_t)(3 - (c & 3)) << top);
            const bool ok = in && run >= k;
            bool periodic = false;
#pragma unroll
            for (int p = 1; p <= NRA_MOTIF_MAX_ROOT; ++p)
                periodic = periodic || ((fwd ^ (fwd >> (2 * p))) & (kmask >> (2 * p))) == 0;
            valid += ok ? 1u : 0u;
            slot[p0 + i] = ok && !periodic ? min(fwd, rev) : NRA_SKETCH_EMPTY;
        }
    }
    __syncthreads();

    // bitonic sort of slot[0, n_sort), ascending: NRA_SKETCH_EMPTY sorts last
    for (int size = 2; size <= n_sort; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n_sort >> 1); t += NRA_SKETCH_THREADS) {
                const int a = 2 * t - (t & (stride - 1));          // the lower partner of compare t
                const int b = a + stride;
                const uint32_t x = slot[a], y = slot[b];
                const bool up = (a & size) == 0;
                if ((x > y) == up) { slot[a] = y; slot[b] = x; }
            }
            __syncthreads();
        }
    }

    // a slot is kept when it holds a k-mer that the slot below does not; the kept ones leave in order
    uint32_t kept = 0, keep_mask = 0;
    if (p0 < n_sort) {
        uint32_t below = p0 ? slot[p0 - 1] : NRA_SKETCH_EMPTY;
#pragma unroll
        for (int i = 0; i < SK_PER_LANE; ++i) {
            const uint32_t v = slot[p0 + i];
            if (v != NRA_SKETCH_EMPTY && v != below) { keep_mask |= 1u << i; ++kept; }
            below = v;
        }
    }
    uint32_t incl = kept, vsum = valid;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) vsum += __shfl_xor(vsum, d, 64);
    if (lane == 63) wave_kept[wave] = incl;
    if (lane == 0) wave_valid[wave] = vsum;
    __syncthreads();
    uint32_t at = incl - kept, total = 0, total_valid = 0;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) {
        if (w < wave) at += wave_kept[w];
        total += wave_kept[w];
        total_valid += wave_valid[w];
    }
    if (kept) {
        uint32_t* out = sketch + sk_off[blockIdx.x] + at;          // at + kept <= total <= n_win, the room the host left
#pragma unroll
        for (int i = 0; i < SK_PER_LANE; ++i)
            if (keep_mask >> i & 1u) *out++ = slot[p0 + i];
    }
    if (tid == 0) { sk_len[blockIdx.x] = (int32_t)total; n_valid[blockIdx.x] = (int32_t)total_valid; }
}

__device__ __forceinline__ uint32_t sketch_hash(uint32_t key)
{
    return (key * 2654435761u) >> 20;            // the top 12 bits: NRA_SKETCH_SET_SLOTS = 4096
}
static_assert(NRA_SKETCH_SET_SLOTS == 1 << 12, "sketch_hash gives 12 bits");

__global__ __launch_bounds__(NRA_SKETCH_THREADS) void k_sketch_pairs(
    int64_t tile0, int32_t n_sorted, const int64_t* __restrict__ tile_first, const int32_t* __restrict__ order,
    const int32_t* __restrict__ grp_end, const int64_t* __restrict__ sk_off, const uint32_t* __restrict__ sketch,
    const int32_t* __restrict__ sk_len, int min_shared, NraSketchPair* __restrict__ pairs, unsigned long long cap,
    unsigned long long* count)
{
    __shared__ uint32_t set[NRA_SKETCH_SET_SLOTS];
    __shared__ int2 found[NRA_SKETCH_BLOCK];      // (position j, shared) of the tile's pairs
    __shared__ uint32_t n_out;
    __shared__ unsigned long long out_base;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = tile0 + (int64_t)blockIdx.x;

    // the last position s with tile_first[s] <= tile: tile_first has n_sorted + 1 entries, the last is the tile count
    int lo = 0, hi = n_sorted;                    // tile_first[lo] <= tile < tile_first[hi]
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tile_first[mid] <= tile) lo = mid; else hi = mid;
    }
    const int s = lo;
    const int seq_i = order[s];
    const int len_i = sk_len[seq_i];
    if (len_i < min_shared) return;               // uniform: no j can share min_shared k-mers with it
    const int j0 = s + 1 + (int)(tile - tile_first[s]) * NRA_SKETCH_BLOCK;
    const int nj = min(NRA_SKETCH_BLOCK, grp_end[s] - j0);

    for (int i = tid; i < NRA_SKETCH_SET_SLOTS; i += NRA_SKETCH_THREADS) set[i] = NRA_SKETCH_EMPTY;
    if (tid == 0) n_out = 0;
    __syncthreads();
    const uint32_t* mine = sketch + sk_off[seq_i];
    for (int e = tid; e < len_i; e += NRA_SKETCH_THREADS) {
        const uint32_t key = mine[e];
        uint32_t h = sketch_hash(key);
        for (int probe = 0; probe < NRA_SKETCH_SET_SLOTS; ++probe) {      // the keys of a sketch are distinct
            if (atomicCAS(&set[h], NRA_SKETCH_EMPTY, key) == NRA_SKETCH_EMPTY) break;
            h = (h + 1) & (NRA_SKETCH_SET_SLOTS - 1);
        }
    }
    __syncthreads();

    for (int jj = wave; jj < nj; jj += SK_WAVES) {
        const int seq_j = order[j0 + jj];
        const int len_j = sk_len[seq_j];
        if (len_j < min_shared) continue;         // uniform over the wave
        const uint32_t* theirs = sketch + sk_off[seq_j];
        // four independent loads per lane are in flight before the first probe: with one load per turn the wave waited
        // for memory once per 64 entries
        int hits = 0;
        for (int e0 = 0; e0 < len_j; e0 += SK_UNROLL * 64) {
            uint32_t key[SK_UNROLL];
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u) {
                const int e = e0 + u * 64 + lane;
                key[u] = e < len_j ? theirs[e] : NRA_SKETCH_EMPTY;
            }
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u) {
                if (key[u] == NRA_SKETCH_EMPTY) continue;
                uint32_t h = sketch_hash(key[u]);
                for (int probe = 0; probe < NRA_SKETCH_SET_SLOTS; ++probe) {
                    const uint32_t v = set[h];
                    if (v == key[u]) { ++hits; break; }
                    if (v == NRA_SKETCH_EMPTY) break;
                    h = (h + 1) & (NRA_SKETCH_SET_SLOTS - 1);
                }
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) hits += __shfl_xor(hits, d, 64);
        if (lane == 0 && hits >= min_shared) found[atomicAdd(&n_out, 1u)] = make_int2(j0 + jj, hits);
    }
    __syncthreads();
    if (n_out == 0) return;
    if (tid == 0) out_base = atomicAdd(count, (unsigned long long)n_out);
    __syncthreads();
    if (tid < (int)n_out && out_base + tid < cap) {
        const int2 f = found[tid];
        *reinterpret_cast<int4*>(&pairs[out_base + tid]) = make_int4(seq_i, order[f.x], f.y, 0);
    }
}

extern "C" int nra_launch_sketch(hipStream_t st, int32_t n_seqs, const uint8_t* seqs, const int64_t* seq_base,
                                 const int32_t* seq_len, int k, const int64_t* sk_off, uint32_t* sketch, int32_t* sk_len,
                                 int32_t* n_valid)
{
    if (n_seqs <= 0) return (int)hipSuccess;
    k_sketch<<<dim3((unsigned)n_seqs), NRA_SKETCH_THREADS, 0, st>>>(seqs, seq_base, seq_len, k, sk_off, sketch, sk_len,
                                                                   n_valid);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_sketch_pairs(hipStream_t st, int64_t tile0, int64_t n_tiles, int32_t n_sorted,
                                       const int64_t* tile_first, const int32_t* order, const int32_t* grp_end,
                                       const int64_t* sk_off, const uint32_t* sketch, const int32_t* sk_len,
                                       int min_shared, NraSketchPair* pairs, unsigned long long cap,
                                       unsigned long long* count)
{
    if (n_tiles <= 0) return (int)hipSuccess;
    if (n_tiles > NRA_SKETCH_LAUNCH_TILES) return (int)hipErrorInvalidConfiguration;
    k_sketch_pairs<<<dim3((unsigned)n_tiles), NRA_SKETCH_THREADS, 0, st>>>(tile0, n_sorted, tile_first, order, grp_end,
                                                                          sk_off, sketch, sk_len, min_shared, pairs, cap,
                                                                          count);
    return (int)hipGetLastError();
}

#endif  // part 42
