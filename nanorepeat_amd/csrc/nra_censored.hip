// nra_censored.hip -- the censored allele fit: exact sizes and lower bounds in one mixture likelihood (gfx950), float64.
//
//   k_censored_fit<KREG>   one wavefront per fit: EM of n closed components N(nu_k, tau^2) and an optional open component
//                          on a problem's N log-domain values, the first n_exact exact, the others right-censored.
//   k_censored_resp        one wavefront per model: one E-step from given w and nu, the N x (n + open) posteriors.
//   k_censored_boot<STAGED>  one wavefront per (problem, replicate, n, open) of the bootstrap: the replicate's values
//                          ys[idx[.]], its three starts by index, the three fits one after the other, the best kept.
//   k_censored_pick        one lane per replicate: the BIC rule over the replicate's records.
// The contract is include/nanorepeat_amd.h, DESIGN.md sections 26 and 27, tests/censored_ref.py and
// tests/censored_boot_ref.py.  The fit itself is nra_cens_body.h.
// Lane l owns the values l, l + 64, l + 128, ...; exact values come first, so at most one step of a lane's loop has
// lanes on both sides of the exact / censored branch.  KREG > 0 keeps the values in registers (N <= 64 * KREG), KREG == 0
// loads them on every pass.  Both forms visit a lane's values in the same ascending order and run the same operations
// on each, and a sum is the lane's partial in that order followed by an xor butterfly over the 64 lanes (a + b is b + a:
// both partners hold the same bits).  Nothing is contracted into an fma (pragma below) and nothing is reassociated, so a
// fit is a function of its values and its start alone -- not of the path, the kernel, the place in the batch or the
// run -- and every lane holds the same parameters, the same lb and takes the same exit.
// The model (at most 8 means, 9 log weights) lives in registers: every loop over components is unrolled over 8 with the
// wave-uniform guard k < n.  One pass over the values per iteration gives the E-step's sum and both M-step sums of every
// component.  The fit uses no LDS and no barriers (k_censored_boot keeps its 24 start means, its best ll and,
// staged, up to 512 values in 4.2 KiB of LDS, one wave per workgroup); no atomics; waves share nothing and never wait on each other; the loop over
// iterations is bounded by max_iter <= 500, the bootstrap's loop over starts by 3 and its binary searches by 21 steps.
#include "nanorepeat_amd.h"
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(39)

#include "nra_cens_body.h"

#pragma clang fp contract(off)

static_assert(sizeof(NraCensBootRec) == 8 * (2 * CENS_C + 4), "a record holds 8 means and 9 weights");

template <int KREG>
__global__ __launch_bounds__(WAVE) void k_censored_fit(const int32_t* __restrict__ ids,
                                                       const NraCensFit* __restrict__ fits,
                                                       const double* __restrict__ values,
                                                       const double* __restrict__ starts, int max_iter, double tol,
                                                       double* __restrict__ out_ll, double* __restrict__ out_w,
                                                       double* __restrict__ out_nu, int32_t* __restrict__ out_iter)
{
    const int fid = ids[blockIdx.x];
    const NraCensFit f = fits[fid];
    const int lane = threadIdx.x, N = f.n_points, n = f.n;
    const CensDirect src{values + f.off};

    double yr[KREG > 0 ? KREG : 1];
    cens_load<KREG>(src, lane, N, yr);

    CensModel M;
    cens_constants(M, f.tau, n, f.open);
#pragma unroll
    for (int k = 0; k < CENS_C; ++k) M.nu[k] = k < n ? starts[f.nu_off + k] : 0.0;
    CensEnd E;
    cens_em<KREG>(src, yr, lane, N, f.n_exact, M, max_iter, tol, E);

    if (lane == 0) {
        out_ll[fid] = E.lb * (double)N;
        out_iter[2 * (size_t)fid] = E.n_iter;
        out_iter[2 * (size_t)fid + 1] = E.converged;
#pragma unroll
        for (int k = 0; k < CENS_C; ++k)
            if (k < n) {
                out_nu[f.nu_off + k] = M.nu[k];
                out_w[f.w_off + k] = E.wk[k];
            }
        if (f.open) out_w[f.w_off + n] = E.wo;
    }
}

__global__ __launch_bounds__(WAVE) void k_censored_resp(const NraCensFit* __restrict__ models,
                                                        const double* __restrict__ values,
                                                        const double* __restrict__ w, const double* __restrict__ nu,
                                                        double* __restrict__ resp)
{
    const NraCensFit f = models[blockIdx.x];
    const int lane = threadIdx.x, N = f.n_points, n = f.n, nc = f.n + f.open;
    const double* __restrict__ Y = values + f.off;
    CensModel M;
    cens_constants(M, f.tau, n, f.open);
#pragma unroll
    for (int k = 0; k < CENS_C; ++k) {
        M.nu[k] = k < n ? nu[f.nu_off + k] : 0.0;
        M.lw[k] = k < n ? log(w[f.w_off + k]) : 0.0;
    }
    M.lwo = f.open ? log(w[f.w_off + n]) : 0.0;
    for (int i = lane; i < N; i += WAVE) {
        double r[CENS_C], t[CENS_C], ro;
        (void)cens_point(M, Y[i], i < f.n_exact, r, ro, t);
        double* __restrict__ out = resp + f.resp_off + (int64_t)i * nc;
#pragma unroll
        for (int k = 0; k < CENS_C; ++k)
            if (k < n) out[k] = r[k];
        if (f.open) out[n] = ro;
    }
}

// ---- the bootstrap

// position min(L - 1, floor((k + 0.5) / n * L)) of a sorted run of L values: censored.quant's float64 expression, the
// division and the product each rounded once as Python rounds them (nothing contracted), so the integer is Python's
__device__ __forceinline__ int cens_quant_pos(int k, int n, int L)
{
    const double q = ((double)k + 0.5) / (double)n;
    return min(L - 1, (int)floor(q * (double)L));
}

// value k (0-based) of the merge of the sorted runs src[0, m) and src[m, m + q): a binary search for how many of the k
// values before it come from the first run (at most 21 steps for m <= 2^20).  Equal values are interchangeable, so
// which of them the search settles on does not matter.
template <class Source>
__device__ __forceinline__ double cens_merged(const Source& src, int m, int q, int k)
{
    int lo = max(0, k - q), hi = min(k, m);
    for (int step = 0; step < 21 && lo < hi; ++step) {
        const int mid = (lo + hi) >> 1;             // mid < hi <= m and 0 <= k - mid - 1 < q
        if (src(mid) < src(m + (k - mid - 1))) lo = mid + 1;
        else hi = mid;
    }
    const int j = k - lo;                            // lo of the first run and j of the second precede value k
    if (lo >= m) return src(m + j);
    if (j >= q) return src(lo);
    const double a = src(lo), b = src(m + j);
    return a < b ? a : b;
}

// The model search of one wave: model (n, open) on the replicate's values `src` (N of them, the first mb exact), or
// nothing when the replicate does not fit that model.
template <class Source>
__device__ __forceinline__ void cens_boot_wave(const Source& src, int lane, int N, int mb, int n, int open, double tau,
                                               int max_iter, double tol, NraCensBootRec* __restrict__ rec)
{
    const int qb = N - mb;
    // n <= the distinct exact values: adjacent positions compared, reduced over the wave.  Every quantity here is the
    // same in every lane, so the wave leaves as one
    if (n > 1) {
        int distinct = 0;
        for (int i = lane + 1; i < mb; i += WAVE) distinct += src(i) != src(i - 1);
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) distinct += __shfl_xor(distinct, m, WAVE);
        if (n > __builtin_amdgcn_readfirstlane(distinct) + 1) {
            if (lane == 0) rec->fitted = 0;
            return;
        }
    }

    // The three starts, censored.start_means' by index: lane 8 t + k finds mean k of start t and leaves it in LDS, so
    // the searches are out of the way (and out of the registers) before the first fit.  The best ll so far sits there
    // too.  200 bytes of LDS per wave; the workgroup is one wave, so a barrier orders its LDS traffic and costs nothing
    __shared__ double s_start[3][CENS_C];
    __shared__ double s_best;
    if (lane < 3 * CENS_C && (lane & (CENS_C - 1)) < n) {
        const int t = lane / CENS_C, k = lane & (CENS_C - 1);
        double v;
        if (t == 0) v = src(cens_quant_pos(k, n, mb));
        else if (t == 1) v = cens_merged(src, mb, qb, cens_quant_pos(k, n, N));
        else if (k < n - 1) v = src(cens_quant_pos(k, n - 1, mb));
        else v = qb > 0 ? fmax(src(mb - 1), src(N - 1)) : src(mb - 1);      // the larger of the runs' last values
        s_start[t][k] = v;
    }
    __syncthreads();

    const double no_registers[1] = {0.0};
    CensModel M;
    cens_constants(M, tau, n, open);
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {
#pragma unroll
        for (int k = 0; k < CENS_C; ++k) M.nu[k] = k < n ? s_start[t][k] : 0.0;
        CensEnd E;
        cens_em<0>(src, no_registers, lane, N, mb, M, max_iter, tol, E);
        const double ll = E.lb * (double)N;
        // the best start is the largest ll, a tie to the lowest start.  The best model so far lives in the record
        // itself: a better start overwrites it (lane 0; stores of one lane to one address stay in order).  Every lane
        // holds the same ll and reads the same s_best, so the branch is wave-uniform
        if (t == 0 || ll > s_best) {
            if (lane == 0) {
                rec->ll = ll;
                rec->fitted = 1;
                rec->start = t;
                rec->n_iter = E.n_iter;
#pragma unroll
                for (int k = 0; k < CENS_C; ++k)
                    if (k < n) {
                        rec->nu[k] = M.nu[k];
                        rec->w[k] = E.wk[k];
                    }
                if (open) rec->w[n] = E.wo;
            }
            __syncthreads();                          // every lane has read s_best
            if (lane == 0) s_best = ll;
        }
        __syncthreads();
    }
}

// STAGED: the replicate's values are gathered once into LDS (N <= 64 * NRA_CENS_KREG, 4 KiB) and the fits read them
// there; otherwise every pass reads them through the index row.  Either way the fit is the streaming form of the body
// (KREG = 0) over a point source, so the bits are those of k_censored_fit on the materialised replicate.  Holding the
// values in registers as k_censored_fit<8> does costs this kernel its second wave per SIMD (255 VGPRs + 6 AGPRs) and
// was measured 38 % slower.
template <bool STAGED>
__global__ __launch_bounds__(WAVE) void k_censored_boot(const int32_t* __restrict__ jobs, int n_rep, int max_alleles,
                                                        const NraCensBootProblem* __restrict__ probs,
                                                        const double* __restrict__ values,
                                                        const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ rep_m, int max_iter, double tol,
                                                        NraCensBootRec* __restrict__ recs)
{
    const int slots = 2 * max_alleles;
    const int r = jobs[blockIdx.x / slots], slot = blockIdx.x % slots;
    const int n = slot / 2 + 1, open = slot & 1;
    const NraCensBootProblem P = probs[r / n_rep];
    const int lane = threadIdx.x, N = P.n_points;
    const int mb = rep_m[r];
    const CensGather src{values + P.off, idx + P.idx_off + (int64_t)(r % n_rep) * N};
    NraCensBootRec* __restrict__ rec = recs + (size_t)r * slots + slot;

    // the models of the replicate: n <= min(max_alleles, distinct exact values), open only with a bound
    if (mb == 0 || n > mb || (open && mb == N)) {
        if (lane == 0) rec->fitted = 0;
        return;
    }
    if constexpr (STAGED) {
        __shared__ double s_y[WAVE * NRA_CENS_KREG];
        for (int i = lane; i < N; i += WAVE) s_y[i] = src(i);
        __syncthreads();
        cens_boot_wave(CensDirect{s_y}, lane, N, mb, n, open, P.tau, max_iter, tol, rec);
    } else {
        cens_boot_wave(src, lane, N, mb, n, open, P.tau, max_iter, tol, rec);
    }
}

// One lane per replicate r of the launch group: censored.choose_model over its records in the order n ascending,
// open 0 before 1 -- the lowest BIC, within 1e-9 of it the fewest parameters, then open = 0 -- and the replicate's
// outputs, zeros where nothing is written.
__global__ __launch_bounds__(256) void k_censored_pick(int n_replicates, int n_rep, int max_alleles,
                                                       const NraCensBootProblem* __restrict__ probs,
                                                       const int32_t* __restrict__ rep_m,
                                                       const NraCensBootRec* __restrict__ recs,
                                                       int32_t* __restrict__ status, int32_t* __restrict__ model_n,
                                                       int32_t* __restrict__ model_open,
                                                       int32_t* __restrict__ best_start, int32_t* __restrict__ n_iter,
                                                       double* __restrict__ ll, double* __restrict__ bic,
                                                       double* __restrict__ nu, double* __restrict__ w)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_replicates) return;
    const NraCensBootProblem P = probs[r / n_rep];
    const int slots = 2 * max_alleles, mb = rep_m[r];
    const NraCensBootRec* __restrict__ mine = recs + (size_t)r * slots;
    double* __restrict__ o_nu = nu + (size_t)r * CENS_C;
    double* __restrict__ o_w = w + (size_t)r * (CENS_C + 1);
    for (int k = 0; k < CENS_C; ++k) o_nu[k] = 0.0;
    for (int k = 0; k <= CENS_C; ++k) o_w[k] = 0.0;
    if (mb == 0) {
        status[r] = NRA_CENS_BOOT_NO_EXACT;
        model_n[r] = 0;
        model_open[r] = P.n_points > mb;      // a bound, as CensoredFit without an exact value
        best_start[r] = 0;
        n_iter[r] = 0;
        ll[r] = 0.0;
        bic[r] = 0.0;
        return;
    }
    // BIC = -2 ll + (2 n + o - 1) lnN, the product first, nothing contracted: the host's bits
    double lowest = __builtin_huge_val();
    for (int s = 0; s < slots; ++s)
        if (mine[s].fitted) {
            const double b = -2.0 * mine[s].ll + (double)(2 * (s / 2 + 1) + (s & 1) - 1) * P.ln_n;
            lowest = b < lowest ? b : lowest;
        }
    int pick = 0, pick_params = 1 << 30;             // slot 0 = (1, 0) is always fitted when mb > 0
    double pick_bic = 0.0;
    for (int s = 0; s < slots; ++s)
        if (mine[s].fitted) {
            const double b = -2.0 * mine[s].ll + (double)(2 * (s / 2 + 1) + (s & 1) - 1) * P.ln_n;
            const int params = 2 * (s / 2 + 1) + (s & 1);
            if (b <= lowest + 1e-9 && params < pick_params) {
                pick = s;
                pick_params = params;
                pick_bic = b;
            }
        }
    const NraCensBootRec& m = mine[pick];
    const int n = pick / 2 + 1, open = pick & 1;
    status[r] = NRA_CENS_BOOT_FITTED;
    model_n[r] = n;
    model_open[r] = open;
    best_start[r] = m.start;
    n_iter[r] = m.n_iter;
    ll[r] = m.ll;
    bic[r] = pick_bic;
    for (int k = 0; k < n; ++k) o_nu[k] = m.nu[k];
    for (int k = 0; k < n + open; ++k) o_w[k] = m.w[k];
}

extern "C" int nra_launch_censored_fit(hipStream_t st, int kreg, int n, const int32_t* ids, const NraCensFit* fits,
                                       const double* values, const double* starts, int max_iter, double tol, double* ll,
                                       double* w, double* nu, int32_t* iter)
{
    if (n <= 0) return (int)hipSuccess;
    if (kreg == NRA_CENS_KREG)
        k_censored_fit<NRA_CENS_KREG><<<dim3((unsigned)n), WAVE, 0, st>>>(ids, fits, values, starts, max_iter, tol, ll, w,
                                                                          nu, iter);
    else if (kreg == 0)
        k_censored_fit<0><<<dim3((unsigned)n), WAVE, 0, st>>>(ids, fits, values, starts, max_iter, tol, ll, w, nu, iter);
    else
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int nra_launch_censored_resp(hipStream_t st, int n, const NraCensFit* models, const double* values,
                                        const double* w, const double* nu, double* resp)
{
    if (n <= 0) return (int)hipSuccess;
    k_censored_resp<<<dim3((unsigned)n), WAVE, 0, st>>>(models, values, w, nu, resp);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_censored_boot(hipStream_t st, int kreg, int n_jobs, const int32_t* jobs, int n_rep,
                                        int max_alleles, const NraCensBootProblem* probs, const double* values,
                                        const int32_t* idx, const int32_t* rep_m, int max_iter, double tol,
                                        NraCensBootRec* recs)
{
    if (n_jobs <= 0) return (int)hipSuccess;
    if (max_alleles < 1 || max_alleles > CENS_C || (int64_t)n_jobs * 2 * max_alleles > INT32_MAX)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)n_jobs * 2u * (unsigned)max_alleles);
    if (kreg == NRA_CENS_KREG)
        k_censored_boot<true><<<grid, WAVE, 0, st>>>(jobs, n_rep, max_alleles, probs, values, idx, rep_m, max_iter, tol,
                                                     recs);
    else if (kreg == 0)
        k_censored_boot<false><<<grid, WAVE, 0, st>>>(jobs, n_rep, max_alleles, probs, values, idx, rep_m, max_iter, tol,
                                                      recs);
    else
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int nra_launch_censored_pick(hipStream_t st, int n_replicates, int n_rep, int max_alleles,
                                        const NraCensBootProblem* probs, const int32_t* rep_m,
                                        const NraCensBootRec* recs, int32_t* status, int32_t* model_n,
                                        int32_t* model_open, int32_t* best_start, int32_t* n_iter, double* ll,
                                        double* bic, double* nu, double* w)
{
    if (n_replicates <= 0) return (int)hipSuccess;
    k_censored_pick<<<dim3((unsigned)((n_replicates + 255) / 256)), 256, 0, st>>>(
        n_replicates, n_rep, max_alleles, probs, rep_m, recs, status, model_n, model_open, best_start, n_iter, ll, bic,
        nu, w);
    return (int)hipGetLastError();
}

#endif  // part 39
