// nra_bootstrap.hip -- the order search of one bootstrap replicate of a phasing problem per workgroup (gfx950), float64.
//
//   k_mixture_boot<D, KREG>  256 threads build the replicate's sample from the kept sizes x, the problem's noise z and
//                            the replicate's indices, then fit orders first_n, first_n + 1, ... to it, ten starts
//                            each, until two components of an order's best start overlap (the answer is the order
//                            before), max_n is reached, or the start rows handed over end at n_cap (NEEDS_MORE).
// The contract is DESIGN.md section 24 and tests/bootstrap_ref.py; a fit is nra_mix_body.h, the body of k_mixture, so
// every fit has the bits k_mixture gives on the same points.  Point j of the sample (0 <= j < 100 m), axis a:
//   X[j][a] = x[r][a] + (z[j d + a] e) (10 + x[r][a]),  r = idx[j mod m]
// in this order and uncontracted: numpy's bits.  KREG > 0 builds the points once and keeps them in registers for all
// of the workgroup's fits; KREG == 0 builds them again on every pass.
// LDS beside the fit's: the best start of the current order and the model of the order before (w, mu, var).  The
// best-start choice, the overlap test and the stop use values every thread holds alike (reduced sums, LDS after a
// barrier, __syncthreads_or), so the workgroup never diverges at a barrier.  Loops are bounded: orders <= 32, starts
// 10, Lloyd steps 10, EM steps 100.  Workgroups share nothing and never wait on each other.
#include "nanorepeat_amd.h"
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(37)

#include "nra_mix_body.h"

// (nra_mix_body.h sets this too; restated here because the bits of the replicate's sample below depend on it: the
// formula must stay a multiply, a multiply and an add, never an fma)
#pragma clang fp contract(off)

// w, mu, var of a model: what a replicate reports
template <int D> struct BootModel {
    double w[MIX_C];
    double mu[MIX_C][D];
    double var[MIX_C][D];
};

// the point source of a replicate
template <int D> struct BootRows {
    const double* __restrict__ x;        // the problem's kept sizes
    const double* __restrict__ z;        // the problem's noise
    const int32_t* __restrict__ idx;     // the replicate's m indices
    int m;
    double e;
    __device__ __forceinline__ void operator()(int i, double (&p)[D]) const
    {
        const int r = idx[i % m];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double v = x[(size_t)r * D + a];
            p[a] = v + (z[(size_t)i * D + a] * e) * (10.0 + v);
        }
    }
};

template <int D, int KREG>
__global__ __launch_bounds__(MIX_T) void k_mixture_boot(const int32_t* __restrict__ jobs, int n_rep,
                                                        const NraBootProblem* __restrict__ probs,
                                                        const double* __restrict__ xs, const double* __restrict__ zs,
                                                        const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ starts,
                                                        int32_t* __restrict__ out_status,
                                                        int32_t* __restrict__ out_order,
                                                        int32_t* __restrict__ out_best, double* __restrict__ out_lb,
                                                        double* __restrict__ out_w, double* __restrict__ out_mu,
                                                        double* __restrict__ out_var)
{
    __shared__ MixParams<D> P[2];
    __shared__ double red[MIX_WAVES][5];
    __shared__ BootModel<D> best, prev;
    const int job = jobs[blockIdx.x];
    const int b = job % n_rep;
    const NraBootProblem pb = probs[job / n_rep];
    const int m = pb.m, N = NRA_BOOT_COPIES * m, t = threadIdx.x;
    const BootRows<D> src{xs + pb.x_off, zs + pb.z_off, idx + pb.idx_off + (int64_t)b * m, m, pb.e};

    double xr[KREG > 0 ? KREG : 1][D];
    double lse_r[KREG > 0 ? KREG : 1];
    if constexpr (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int i = k * MIX_T + t;
#pragma unroll
            for (int a = 0; a < D; ++a) xr[k][a] = 0.0;
            if (i < N) src(i, xr[k]);
            lse_r[k] = 0.0;
        }
    }

    const int32_t* st = starts + pb.start_off;      // the rows of the next fit
    int status = NRA_BOOT_NEEDS_MORE, order = 0;
    int prev_n = 1, prev_t = -1;                     // the order before and its best start; order 1 has no model
    double prev_lb = 0.0;
    for (int n = pb.first_n;; ++n) {
        if (n > pb.max_n) { status = NRA_BOOT_DECIDED; order = pb.max_n; break; }
        if (n > pb.n_cap) break;
        if (n == 1) continue;                        // no pair to overlap
        int best_t = 0;
        double best_lb = 0.0;
        for (int s = 0; s < NRA_BOOT_STARTS; ++s, st += n) {
            int cur, n_iter, converged;
            double lb;
            __syncthreads();                         // the fit before has been read
            mix_fit<D, KREG>(N, n, src, st, xr, lse_r, P, red, cur, lb, n_iter, converged);
            if (s == 0 || lb > best_lb) {            // the largest lb, a tie to the lowest start
                best_lb = lb;
                best_t = s;
                if (t < n) {
                    best.w[t] = P[cur].w[t];
#pragma unroll
                    for (int a = 0; a < D; ++a) { best.mu[t][a] = P[cur].mu[t][a]; best.var[t][a] = P[cur].var[t][a]; }
                }
            }
        }
        __syncthreads();
        // two components whose intervals mu +- z_o max(1, sd) overlap on every axis (touching counts)
        int hit = 0;
        for (int q = t; q < n * n; q += MIX_T) {
            const int i = q / n, j = q % n;
            if (i >= j) continue;
            int all = 1;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const double hi = pb.z_o * fmax(1.0, sqrt(best.var[i][a])), hj = pb.z_o * fmax(1.0, sqrt(best.var[j][a]));
                const double lo = fmax(best.mu[i][a] - hi, best.mu[j][a] - hj);
                const double up = fmin(best.mu[i][a] + hi, best.mu[j][a] + hj);
                if (!(lo - up <= 0.0)) all = 0;
            }
            hit |= all;
        }
        if (__syncthreads_or(hit)) { status = NRA_BOOT_DECIDED; order = n - 1; break; }
        if (t < n) {
            prev.w[t] = best.w[t];
#pragma unroll
            for (int a = 0; a < D; ++a) { prev.mu[t][a] = best.mu[t][a]; prev.var[t][a] = best.var[t][a]; }
        }
        prev_n = n;
        prev_t = best_t;
        prev_lb = best_lb;
    }
    __syncthreads();

    const int64_t r = pb.rep_off + b;
    if (t == 0) {
        out_status[r] = status;
        out_order[r] = order;
        out_best[r] = status == NRA_BOOT_DECIDED ? prev_t : -1;
        out_lb[r] = status == NRA_BOOT_DECIDED ? prev_lb : 0.0;
    }
    if (status == NRA_BOOT_DECIDED && order > 1 && order == prev_n && t < order) {
        const int64_t o = pb.comp_off + (int64_t)b * pb.n_cap + t;
        out_w[o] = prev.w[t];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            out_mu[2 * o + a] = a < D ? prev.mu[t][a < D ? a : 0] : 0.0;
            out_var[2 * o + a] = a < D ? prev.var[t][a < D ? a : 0] : 0.0;
        }
    }
}

template <int D, int KREG>
static int launch_boot(hipStream_t st, int n, const int32_t* jobs, int n_rep, const NraBootProblem* probs,
                       const double* x, const double* z, const int32_t* idx, const int32_t* starts, int32_t* status,
                       int32_t* order, int32_t* best_start, double* lb, double* w, double* mu, double* var)
{
    k_mixture_boot<D, KREG><<<dim3((unsigned)n), MIX_T, 0, st>>>(jobs, n_rep, probs, x, z, idx, starts, status, order,
                                                                 best_start, lb, w, mu, var);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_mixture_boot(hipStream_t st, int d, int kreg, int n, const int32_t* jobs, int n_rep,
                                       const NraBootProblem* probs, const double* x, const double* z,
                                       const int32_t* idx, const int32_t* starts, int32_t* status, int32_t* order,
                                       int32_t* best_start, double* lb, double* w, double* mu, double* var)
{
    if (n <= 0) return (int)hipSuccess;
#define BOOT_CASE(D_, K_) \
    if (d == D_ && kreg == K_) \
        return launch_boot<D_, K_>(st, n, jobs, n_rep, probs, x, z, idx, starts, status, order, best_start, lb, w, mu, var)
    BOOT_CASE(1, NRA_MIX_KREG_SMALL);
    BOOT_CASE(1, NRA_MIX_KREG);
    BOOT_CASE(1, 0);
    BOOT_CASE(2, NRA_MIX_KREG_SMALL);
    BOOT_CASE(2, NRA_MIX_KREG);
    BOOT_CASE(2, 0);
#undef BOOT_CASE
    return (int)hipErrorInvalidValue;
}

#endif  // part 37
