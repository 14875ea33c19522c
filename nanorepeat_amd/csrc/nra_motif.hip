// nra_motif.hip -- tandem motif discovery: the tandem positions of every read tract per period 1..6 and their motif
// classes (gfx950).
//
//   k_tract_motifs  one wave per tract, four waves per 256-thread workgroup, workgroups striding over groups of four
//                   tracts (sorted by length, so the four run about as long).  Each lane takes 16 positions at a time
//                   (blocks lane, lane + 64, ...): two 16-byte loads give the block's bases and the 2P - 1 bases after
//                   it, packed into 2-bit codes, first base most significant.  Per position and period p the two
//                   p-words are compared; a tandem word's class (its smallest rotation) and primitivity come from
//                   p - 1 rotations in registers.  A lane keeps one pending (class, count) run per p and adds it to
//                   its wave's LDS histogram (dense class ids, code-to-id table in LDS) only when the class changes:
//                   a pure tract adds once per lane and period.  The top T come from T wave-wide arg-max passes over
//                   the histogram held in registers, with a packed key count << 10 | (1023 - id): ids are ordered by
//                   (p, code), so the largest key is the largest count, then the smallest p, then the smallest code.
// The contract (tandem positions, classes, order) is DESIGN.md section 15 and tests/motif_ref.py.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(29)

#define MOTIF_WAVES 4
#define MOTIF_HIST 1024                        // NRA_MOTIF_CLASSES rounded up to 16 entries per lane

// (smallest rotation of the p-base word w, w primitive); w holds 2p bits, first base most significant
template <int p>
__device__ __forceinline__ uint32_t motif_class(uint32_t w, bool& primitive)
{
    constexpr uint32_t mask = (1u << (2 * p)) - 1u;
    uint32_t m = w;
    bool prim = true;
#pragma unroll
    for (int r = 1; r < p; ++r) {
        const uint32_t x = ((w << (2 * r)) | (w >> (2 * (p - r)))) & mask;
        prim = prim && x != w;
        m = min(m, x);
    }
    primitive = prim;
    return m;
}

__device__ __forceinline__ int motif_code_offset(int p) { return ((1 << (2 * p)) - 4) / 3; }   // 0 4 20 84 340 1364

// one period at position k of a block: tandem test, class, run merge
template <int p>
__device__ __forceinline__ void motif_step(uint32_t win, uint32_t bad, int k, int rem, int max_p, uint32_t (&pc)[6],
                                           uint32_t (&pn)[6], uint32_t (&tot)[6], const int16_t* dense, int* hist)
{
    if (p > max_p) return;                                       // uniform
    constexpr uint32_t mask = (1u << (2 * p)) - 1u;
    const uint32_t w1 = win >> (24 - 2 * p);
    const uint32_t w2 = (win >> (24 - 4 * p)) & mask;
    const bool ok = w1 == w2 && ((bad >> k) & ((1u << (2 * p)) - 1u)) == 0u && k + 2 * p <= rem;
    if (ok) {
        bool prim;
        const uint32_t c = motif_class<p>(w1, prim);
        if (prim) {
            ++tot[p - 1];
            if (pn[p - 1] != 0u && pc[p - 1] == c) {
                ++pn[p - 1];
            } else {
                if (pn[p - 1] != 0u) atomicAdd(&hist[dense[motif_code_offset(p) + (int)pc[p - 1]]], (int)pn[p - 1]);
                pc[p - 1] = c;
                pn[p - 1] = 1u;
            }
        }
    }
}

__device__ __forceinline__ uint32_t motif_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ uint32_t motif_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(MOTIF_WAVES * WAVE) void k_tract_motifs(
    int n_tracts, const NraMotifTract* __restrict__ tracts, const uint8_t* __restrict__ codes,
    const int16_t* __restrict__ dense_of, int max_p, int top_n, int32_t* __restrict__ n_tandem,
    uint32_t* __restrict__ top_key)
{
    __shared__ int16_t s_dense[NRA_MOTIF_CODES];
    __shared__ int s_hist[MOTIF_WAVES][MOTIF_HIST];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    for (int i = threadIdx.x; i < NRA_MOTIF_CODES; i += MOTIF_WAVES * WAVE) s_dense[i] = dense_of[i];
    int* hist = s_hist[wave];
#pragma unroll
    for (int j = 0; j < MOTIF_HIST / WAVE; ++j) hist[lane + WAVE * j] = 0;
    const int groups = (n_tracts + MOTIF_WAVES - 1) / MOTIF_WAVES;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {      // uniform over the workgroup: the barriers hold
        __syncthreads();
        const int t = g * MOTIF_WAVES + wave;
        uint32_t tot[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (t < n_tracts) {
            const NraMotifTract tr = tracts[t];
            const uint8_t* s = codes + tr.off;
            const int n = tr.n;
            uint32_t pc[6] = {0u, 0u, 0u, 0u, 0u, 0u}, pn[6] = {0u, 0u, 0u, 0u, 0u, 0u};
            for (int b = lane; NRA_MOTIF_BLOCK * b + 2 <= n; b += WAVE) {
                const int i0 = NRA_MOTIF_BLOCK * b;
                const uint4 lo = *reinterpret_cast<const uint4*>(s + i0);
                const uint4 hi = *reinterpret_cast<const uint4*>(s + i0 + 16);
                const uint32_t wd[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                uint64_t bits = 0;                                // base j of the 32 at bits 63 - 2j .. 62 - 2j
                uint32_t bad = 0;                                 // bit j: base j is not ACGT
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const uint32_t c = (wd[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    bits |= (uint64_t)(c & 3u) << (62 - 2 * j);
                    bad |= (uint32_t)(c > 3u) << j;
                }
                const int rem = n - i0;                           // position k needs k + 2p <= rem
#pragma unroll
                for (int k = 0; k < NRA_MOTIF_BLOCK; ++k) {
                    const uint32_t win = (uint32_t)((bits << (2 * k)) >> 40);   // bases k .. k + 11
                    motif_step<1>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                    motif_step<2>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                    motif_step<3>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                    motif_step<4>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                    motif_step<5>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                    motif_step<6>(win, bad, k, rem, max_p, pc, pn, tot, s_dense, hist);
                }
            }
#pragma unroll
            for (int p = 1; p <= 6; ++p)
                if (pn[p - 1] != 0u) atomicAdd(&hist[s_dense[motif_code_offset(p) + (int)pc[p - 1]]], (int)pn[p - 1]);
        }
        __syncthreads();
        if (t < n_tracts) {
            // the lane's 16 histogram entries to keys; it zeroes them for the next tract (only this lane reads them)
            uint32_t key[MOTIF_HIST / WAVE];
#pragma unroll
            for (int j = 0; j < MOTIF_HIST / WAVE; ++j) {
                const int id = lane + WAVE * j;
                const uint32_t v = (uint32_t)hist[id];
                hist[id] = 0;
                key[j] = v ? (v << 10) | (uint32_t)(1023 - id) : 0u;
            }
            uint32_t prev = 0xffffffffu;
            for (int q = 0; q < top_n; ++q) {
                uint32_t m = 0u;
#pragma unroll
                for (int j = 0; j < MOTIF_HIST / WAVE; ++j) m = max(m, key[j] < prev ? key[j] : 0u);
                m = motif_wave_max(m);
                if (lane == 0) top_key[(int64_t)t * NRA_MOTIF_MAX_TOP + q] = m;
                prev = m;
            }
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const uint32_t sum = motif_wave_sum(tot[p]);
                if (lane == 0) n_tandem[(int64_t)t * NRA_MOTIF_MAX_P + p] = (int32_t)sum;
            }
        }
    }
}

extern "C" int nra_launch_tract_motifs(hipStream_t st, int n_grid, int n_tracts, const NraMotifTract* tracts,
                                       const uint8_t* codes, const int16_t* dense_of, int max_p, int top_n,
                                       int32_t* n_tandem, uint32_t* top_key)
{
    if (n_tracts <= 0) return (int)hipSuccess;
    k_tract_motifs<<<dim3((unsigned)n_grid), MOTIF_WAVES * WAVE, 0, st>>>(n_tracts, tracts, codes, dense_of, max_p,
                                                                          top_n, n_tandem, top_key);
    return (int)hipGetLastError();
}

#endif  // part 29
