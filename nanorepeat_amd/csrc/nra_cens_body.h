// nra_cens_body.h -- the body of one censored fit (DESIGN.md sections 26 and 27), shared by k_censored_fit and
// k_censored_boot (nra_censored.hip): the E-step of one value, the wave sum, and the EM loop over a point source.
// A point source `src` gives value i of the fitted sample as src(i): "value i of the problem" (CensDirect) or "value
// ys[idx[i]] of the replicate" (CensGather).  Lane l owns the values l, l + 64, ...; with KREG > 0 they sit in the
// registers yr[] (filled by cens_load), with KREG == 0 they are read from the source on every pass.  Both forms and
// both sources visit a lane's values in the same ascending order and run the same operations on each, so a fit is a
// function of its values and its start alone.  Nothing here is contracted into an fma or reassociated.
#pragma once

#include "nanorepeat_amd.h"
#include "nra_device.h"

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

// what a fit ends with, next to the means in its CensModel
struct CensEnd {
    double wk[CENS_C], wo;   // the weights of the last M-step
    double lb;               // of the last E-step
    int n_iter, converged;
};

// value i of a problem
struct CensDirect {
    const double* __restrict__ y;
    __device__ __forceinline__ double operator()(int i) const { return y[i]; }
};

// value i of a replicate: the problem's value idx[i]
struct CensGather {
    const double* __restrict__ y;
    const int32_t* __restrict__ idx;
    __device__ __forceinline__ double operator()(int i) const { return y[idx[i]]; }
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
// at the bound otherwise).  Returns log p(y).  The model comes by value, not by reference: as compiled for gfx950,
// k_censored_fit takes 255 VGPRs and runs two waves per SIMD this way, and 256 VGPRs + 30 AGPRs and one wave with a
// reference into the caller's model.
__device__ __forceinline__ double cens_point(const CensModel M, double y, bool exact, double (&r)[CENS_C], double& ro,
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

// the lane's values of a sample of N into registers (KREG > 0); 0 beyond the sample
template <int KREG, class Source>
__device__ __forceinline__ void cens_load(const Source& src, int lane, int N, double (&yr)[KREG > 0 ? KREG : 1])
{
    if constexpr (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k) {
            const int i = k * WAVE + lane;
            yr[k] = i < N ? src(i) : 0.0;
        }
    }
}

// One fit of the model (M.n, M.open) from the start means in M.nu, weights 1 / (n + open), on the N values of `src`
// (the first n_exact exact): EM until |lb - lb of the E-step before| < tol or max_iter E-steps.  Leaves the means in
// M.nu and the rest in E; every lane ends with the same bits.
template <int KREG, class Source>
__device__ __forceinline__ void cens_em(const Source& src, const double (&yr)[KREG > 0 ? KREG : 1], int lane, int N,
                                        int n_exact, CensModel& M, int max_iter, double tol, CensEnd& E)
{
    const int n = M.n, open = M.open;
    const double w0 = 1.0 / (double)(n + open);
    E.wo = open ? w0 : 0.0;
#pragma unroll
    for (int k = 0; k < CENS_C; ++k) {
        M.lw[k] = log(w0);
        E.wk[k] = w0;
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
            sl += cens_point(M, y, i < n_exact, r, ro, t);
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
            for (int i = lane; i < N; i += WAVE) body(i, src(i));
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
                E.wk[k] = nk / (double)N;
                M.lw[k] = log(E.wk[k]);
                if (sr[k] > 1e-12) M.nu[k] = sy[k] / nk;
            }
        if (open) {
            E.wo = (so + CENS_10EPS) / (double)N;
            M.lwo = log(E.wo);
        }
        n_iter = it;
        if (fabs(lb - lb_prev) < tol) { converged = 1; break; }
        lb_prev = lb;
    }
    E.lb = lb;
    E.n_iter = n_iter;
    E.converged = converged;
}
