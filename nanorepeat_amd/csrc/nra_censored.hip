// nra_censored.hip -- the censored allele fit: exact sizes and lower bounds in one mixture likelihood (gfx950), float64.
//
//   k_censored_fit<KREG>  one wavefront per fit: EM of n closed components N(nu_k, tau^2) and an optional open component
//                         on a problem's N log-domain values, the first n_exact exact, the others right-censored.
//   k_censored_resp       one wavefront per model: one E-step from given w and nu, the N x (n + open) posteriors.
// The contract is include/nanorepeat_amd.h, DESIGN.md section 26 and tests/censored_ref.py.
// Lane l owns the values l, l + 64, l + 128, ...; exact values come first, so at most one step of a lane's loop has
// lanes on both sides of the exact / censored branch.  KREG > 0 keeps the values in registers (N <= 64 * KREG), KREG == 0
// loads them on every pass.  Both forms visit a lane's values in the same ascending order and run the same operations
// on each, and a sum is the lane's partial in that order followed by an xor butterfly over the 64 lanes (a + b is b + a:
// both partners hold the same bits).  Nothing is contracted into an fma (pragma below) and nothing is reassociated, so a
// fit is a function of its problem and its start alone -- not of the path, the place in the batch or the run -- and
// every lane holds the same parameters, the same lb and takes the same exit.
// The model (at most 8 means, 9 log weights) lives in registers: every loop over components is unrolled over 8 with the
// wave-uniform guard k < n.  One pass over the values per iteration gives the E-step's sum and both M-step sums of every
// component.  No LDS, no barriers, no atomics; waves share nothing and never wait on each other; the loop over
// iterations is bounded by max_iter <= 500.
#include "nanorepeat_amd.h"
#include "nra_device.h"

#ifndef NRA_PART
#define NRA_PART 0
#endif
#define NRA_HAS_PART(n) (NRA_PART == 0 || NRA_PART == (n))

#if NRA_HAS_PART(39)

#pragma clang fp contract(off)

#define CENS_C NRA_CENS_MAX_COMPONENTS
#define CENS_SQRT1_2 0.7071067811865476      // sqrt(1/2)
#define CENS_SQRT_2_PI 0.7978845608028654    // sqrt(2/pi)
#define CENS_2PI 6.283185307179586
#define CENS_10EPS (10.0 * 2.220446049250313e-16)

struct CensModel {
    double nu[CENS_C];
    double lw[CENS_C];       // log w_k
    double lwo;              // log w_o
    double tau, inv_tau;     // tau, 1 / tau
    double i2, hl;           // 1 / (2 tau^2), log(2 pi tau^2) / 2
    int n, open;
};

__device__ __forceinline__ void cens_constants(CensModel& M, double tau, int n, int open)
{
    M.n = n;
    M.open = open;
    M.tau = tau;
    M.inv_tau = 1.0 / tau;
    M.i2 = 1.0 / (2.0 * (tau * tau));
    M.hl = 0.5 * log(CENS_2PI * (tau * tau));
}

// The E-step of one value: r[k] = its posterior for closed component k (0 for k >= n), ro = for the open one, t[k] =
// what it adds to the mean of component k per unit of r (the value itself when exact, the mean of the normal truncated
// at the bound otherwise).  Returns log p(y).
__device__ __forceinline__ double cens_point(const CensModel& M, double y, bool exact, double (&r)[CENS_C], double& ro,
                                             double (&t)[CENS_C])
{
    double lp[CENS_C];
    double m = -__builtin_huge_val();
    const bool with_open = !exact && M.open;
    if (exact) {
#pragma unroll
        for (int k = 0; k < CENS_C; ++k) {
            lp[k] = 0.0;
            t[k] = y;
            if (k < M.n) {
                const double d = y - M.nu[k];
                lp[k] = (M.lw[k] - M.hl) - (d * d) * M.i2;
                m = fmax(m, lp[k]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < CENS_C; ++k) {
            lp[k] = 0.0;
            t[k] = 0.0;
            if (k < M.n) {
                const double z = (y - M.nu[k]) * M.inv_tau;
                const double u = z * CENS_SQRT1_2;
                double ls, lam;
                if (u <= 0.0) {
                    const double e = erfc(u);
                    ls = log(0.5 * e);
                    lam = (CENS_SQRT_2_PI * exp(-(u * u))) / e;
                } else {
                    const double e = erfcx(u);
                    ls = log(0.5 * e) - u * u;
                    lam = CENS_SQRT_2_PI / e;
                }
                lp[k] = M.lw[k] + ls;
                t[k] = M.nu[k] + M.tau * lam;
                m = fmax(m, lp[k]);
            }
        }
        if (with_open) m = fmax(m, M.lwo);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < CENS_C; ++k)
        if (k < M.n) s += exp(lp[k] - m);
    if (with_open) s += exp(M.lwo - m);
    const double lse = m + log(s);
#pragma unroll
    for (int k = 0; k < CENS_C; ++k) r[k] = k < M.n ? exp(lp[k] - lse) : 0.0;
    ro = with_open ? exp(M.lwo - lse) : 0.0;
    return lse;
}

__device__ __forceinline__ double cens_wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

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
    const double* __restrict__ Y = values + f.off;

    double yr[KREG > 0 ? KREG : 1];
    if constexpr (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int i = k * WAVE + lane;
            yr[k] = i < N ? Y[i] : 0.0;
        }
    }

    CensModel M;
    cens_constants(M, f.tau, n, f.open);
    const double w0 = 1.0 / (double)(n + f.open);
    double wk[CENS_C], wo = f.open ? w0 : 0.0;
#pragma unroll
    for (int k = 0; k < CENS_C; ++k) {
        M.nu[k] = k < n ? starts[f.nu_off + k] : 0.0;
        M.lw[k] = log(w0);
        wk[k] = w0;
    }
    M.lwo = log(w0);

    double lb = 0.0, lb_prev = -__builtin_huge_val();
    int n_iter = 0, converged = 0;
    for (int it = 1; it <= max_iter; ++it) {
        double sr[CENS_C], sy[CENS_C], so = 0.0, sl = 0.0;
#pragma unroll
        for (int k = 0; k < CENS_C; ++k) sr[k] = sy[k] = 0.0;
        auto body = [&](int i, double y) {
            double r[CENS_C], t[CENS_C], ro;
            sl += cens_point(M, y, i < f.n_exact, r, ro, t);
#pragma unroll
            for (int k = 0; k < CENS_C; ++k)
                if (k < n) {
                    sr[k] += r[k];
                    sy[k] += r[k] * t[k];
                }
            so += ro;
        };
        if constexpr (KREG > 0) {
            // one copy of the body: the value of step k is picked from the registers by a chain of selects
#pragma unroll 1
            for (int k = 0; k * WAVE < N; ++k) {
                double y = yr[0];
#pragma unroll
                for (int j = 1; j < KREG; ++j) y = k == j ? yr[j] : y;
                if (k * WAVE + lane < N) body(k * WAVE + lane, y);
            }
        } else {
            for (int i = lane; i < N; i += WAVE) body(i, Y[i]);
        }
        sl = cens_wave_sum(sl);
        so = cens_wave_sum(so);
#pragma unroll
        for (int k = 0; k < CENS_C; ++k)
            if (k < n) {
                sr[k] = cens_wave_sum(sr[k]);
                sy[k] = cens_wave_sum(sy[k]);
            }
        lb = sl / (double)N;
#pragma unroll
        for (int k = 0; k < CENS_C; ++k)
            if (k < n) {
                const double nk = sr[k] + CENS_10EPS;
                wk[k] = nk / (double)N;
                M.lw[k] = log(wk[k]);
                if (sr[k] > 1e-12) M.nu[k] = sy[k] / nk;
            }
        if (f.open) {
            wo = (so + CENS_10EPS) / (double)N;
            M.lwo = log(wo);
        }
        n_iter = it;
        if (fabs(lb - lb_prev) < tol) { converged = 1; break; }
        lb_prev = lb;
    }

    if (lane == 0) {
        out_ll[fid] = lb * (double)N;
        out_iter[2 * (size_t)fid] = n_iter;
        out_iter[2 * (size_t)fid + 1] = converged;
#pragma unroll
        for (int k = 0; k < CENS_C; ++k)
            if (k < n) {
                out_nu[f.nu_off + k] = M.nu[k];
                out_w[f.w_off + k] = wk[k];
            }
        if (f.open) out_w[f.w_off + n] = wo;
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

#endif  // part 39
