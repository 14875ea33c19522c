// nra_mixture.hip -- diagonal Gaussian mixture fits for the phasing step: one workgroup per fit (gfx950), float64.
//
//   k_mixture<D, KREG>  256 threads fit n components to the N x D sample of one problem from one start: Lloyd steps
//                       from the start means, a one-hot M-step, then EM until the mean log-likelihood moves by less
//                       than 1e-3.  The contract is DESIGN.md section 17 and tests/mixture_ref.py.
// The fit itself (the point order, the sums, the Lloyd and EM steps) is nra_mix_body.h, shared with k_mixture_boot.
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(31)

#include "nra_mix_body.h"

template <int D, int KREG>
__global__ __launch_bounds__(MIX_T) void k_mixture(const int32_t* __restrict__ fit_ids,
                                                   const NraMixFit* __restrict__ fits,
                                                   const NraMixProblem* __restrict__ probs,
                                                   const double* __restrict__ samples,
                                                   const int32_t* __restrict__ starts, double* __restrict__ out_lb,
                                                   double* __restrict__ out_w, double* __restrict__ out_mu,
                                                   double* __restrict__ out_var, int32_t* __restrict__ out_iter)
{
    __shared__ MixParams<D> P[2];
    __shared__ double red[MIX_WAVES][5];
    const int f = fit_ids[blockIdx.x];
    const NraMixFit ft = fits[f];
    const NraMixProblem pb = probs[ft.problem];
    const int N = pb.n, n = ft.n, t = threadIdx.x;
    const MixRows<D> src{samples + pb.off};

    double xr[KREG > 0 ? KREG : 1][D];
    double lse_r[KREG > 0 ? KREG : 1];
    if constexpr (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int i = k * MIX_T + t;
#pragma unroll
            for (int a = 0; a < D; ++a) xr[k][a] = i < N ? src.X[(size_t)i * D + a] : 0.0;
            lse_r[k] = 0.0;
        }
    }

    int cur, n_iter, converged;
    double lb;
    mix_fit<D, KREG>(N, n, src, starts + ft.off, xr, lse_r, P, red, cur, lb, n_iter, converged);

    if (t < n) {
        out_w[ft.off + t] = P[cur].w[t];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            out_mu[2 * (ft.off + t) + a] = a < D ? P[cur].mu[t][a < D ? a : 0] : 0.0;
            out_var[2 * (ft.off + t) + a] = a < D ? P[cur].var[t][a < D ? a : 0] : 0.0;
        }
    }
    if (t == 0) {
        out_lb[f] = lb;
        out_iter[2 * (size_t)f] = n_iter;
        out_iter[2 * (size_t)f + 1] = converged;
    }
}

template <int D, int KREG>
static int launch_mixture(hipStream_t st, int n, const int32_t* fit_ids, const NraMixFit* fits,
                          const NraMixProblem* probs, const double* samples, const int32_t* starts, double* lb,
                          double* w, double* mu, double* var, int32_t* iter)
{
    k_mixture<D, KREG><<<dim3((unsigned)n), MIX_T, 0, st>>>(fit_ids, fits, probs, samples, starts, lb, w, mu, var, iter);
    return (int)hipGetLastError();
}

extern "C" int nra_launch_mixture(hipStream_t st, int d, int kreg, int n, const int32_t* fit_ids, const NraMixFit* fits,
                                  const NraMixProblem* probs, const double* samples, const int32_t* starts, double* lb,
                                  double* w, double* mu, double* var, int32_t* iter)
{
    if (n <= 0) return (int)hipSuccess;
#define MIX_CASE(D_, K_) \
    if (d == D_ && kreg == K_) return launch_mixture<D_, K_>(st, n, fit_ids, fits, probs, samples, starts, lb, w, mu, var, iter)
    MIX_CASE(1, NRA_MIX_KREG_SMALL);
    MIX_CASE(1, NRA_MIX_KREG);
    MIX_CASE(1, 0);
    MIX_CASE(2, NRA_MIX_KREG_SMALL);
    MIX_CASE(2, NRA_MIX_KREG);
    MIX_CASE(2, 0);
#undef MIX_CASE
    return (int)hipErrorInvalidValue;
}

#endif  // part 31
