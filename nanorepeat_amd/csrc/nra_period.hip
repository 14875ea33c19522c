// nra_period.hip -- tandem periods: the lag-match spectrum of every tract for the lags 1..64 (gfx950).
//
//   k_tract_periods  one wave per tract, four waves per 256-thread workgroup, workgroups striding over groups of four
//                    tracts (sorted by length, so the four run about as long).  Lane l owns lag p = l + 1.  The wave
//                    walks the tract in words of 32 bases: 64 words at a time, lane l packs word l of the 64 -- two
//                    16-byte loads to a 64-bit register of 2-bit codes (base j at bits 2j, 2j + 1) and a 64-bit
//                    validity mask (bit 2j: base j is A, C, G or T and lies inside the tract).  The wave then takes 62
//                    of them in turn: the word and the two after it come to every lane by v_readlane (the word index
//                    is uniform), each lane forms the word shifted by its own p from two of the three (a funnel
//                    shift by a lane constant), XORs, folds the two bits of a base, masks with both validity masks and
//                    adds two popcounts to two registers.  The tail (i + p < n) is in the masks.  No atomics, no
//                    reduction, no LDS; the two results leave as one coalesced store of [tract][lag] each.
// The contract (valid and matching positions per lag) is include/nanorepeat_amd.h, DESIGN.md section 22 and
// tests/period_ref.py.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(35)

#define PERIOD_WAVES 4
#define PERIOD_STEP 62                          // words a wave takes per 64 packed: a word borrows from the next two

static_assert(WAVE == NRA_PERIOD_MAX_P, "a lane per lag");

__device__ __forceinline__ uint64_t period_readlane(uint64_t v, int lane)   // `lane` is uniform over the wave
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(PERIOD_WAVES * WAVE) void k_tract_periods(
    int n_tracts, const NraPeriodTract* __restrict__ tracts, const uint8_t* __restrict__ codes,
    int32_t* __restrict__ match, int32_t* __restrict__ valid)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), lane = threadIdx.x % WAVE;   // uniform
    // lag p = lane + 1 as a shift by s = 1..32 bases of the pair (word, next) for p <= 32, (next, next2) beyond
    const bool far = lane >= 32;
    const int sh = 2 * (far ? lane - 31 : lane + 1);              // 2..64 bits
    const int groups = (n_tracts + PERIOD_WAVES - 1) / PERIOD_WAVES;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int t = g * PERIOD_WAVES + wave;
        if (t >= n_tracts) continue;                              // uniform over the wave; the kernel has no barrier
        const NraPeriodTract tr = tracts[t];
        const uint8_t* s = codes + tr.off;
        const int n = tr.n;
        const int n_words = (n + NRA_PERIOD_WORD - 1) / NRA_PERIOD_WORD;
        uint32_t n_match = 0, n_valid = 0;
        for (int w0 = 0; w0 < n_words; w0 += PERIOD_STEP) {
            // lane l packs word w0 + l; a word at or beyond the tract's end is empty and is not loaded
            uint64_t bits = 0, ok = 0;
            const int rem = n - NRA_PERIOD_WORD * (w0 + lane);    // bases of the tract from this word on
            if (rem > 0) {
                const uint8_t* at = s + (int64_t)NRA_PERIOD_WORD * (w0 + lane);
                const uint4 lo = *reinterpret_cast<const uint4*>(at);
                const uint4 hi = *reinterpret_cast<const uint4*>(at + 16);
                const uint32_t wd[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int j = 0; j < NRA_PERIOD_WORD; ++j) {
                    const uint32_t c = (wd[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    bits |= (uint64_t)(c & 3u) << (2 * j);
                    ok |= (uint64_t)(c <= 3u && j < rem) << (2 * j);
                }
            }
            const int count = min(PERIOD_STEP, n_words - w0);
            uint64_t b0 = period_readlane(bits, 0), m0 = period_readlane(ok, 0);
            uint64_t b1 = period_readlane(bits, 1), m1 = period_readlane(ok, 1);
            for (int w = 0; w < count; ++w) {
                const uint64_t b2 = period_readlane(bits, w + 2), m2 = period_readlane(ok, w + 2);
                const uint64_t ba = far ? b1 : b0, bb = far ? b2 : b1;
                const uint64_t ma = far ? m1 : m0, mb = far ? m2 : m1;
                // bases s .. s + 31 of the pair: the low part is empty when the shift is the whole word
                const uint64_t bs = (sh < 64 ? ba >> sh : 0ull) | (bb << (64 - sh));
                const uint64_t ms = (sh < 64 ? ma >> sh : 0ull) | (mb << (64 - sh));
                const uint64_t x = b0 ^ bs;
                const uint64_t both = m0 & ms;
                n_valid += (uint32_t)__popcll(both);
                n_match += (uint32_t)__popcll(both & ~(x | (x >> 1)));
                b0 = b1; m0 = m1;
                b1 = b2; m1 = m2;
            }
        }
        match[(int64_t)t * NRA_PERIOD_MAX_P + lane] = (int32_t)n_match;
        valid[(int64_t)t * NRA_PERIOD_MAX_P + lane] = (int32_t)n_valid;
    }
}

extern "C" int nra_launch_tract_periods(hipStream_t st, int n_grid, int n_tracts, const NraPeriodTract* tracts,
                                        const uint8_t* codes, int32_t* match, int32_t* valid)
{
    if (n_tracts <= 0) return (int)hipSuccess;
    k_tract_periods<<<dim3((unsigned)n_grid), PERIOD_WAVES * WAVE, 0, st>>>(n_tracts, tracts, codes, match, valid);
    return (int)hipGetLastError();
}

#endif  // part 35
