// nra_mix_body.h -- the body of one diagonal Gaussian mixture fit by a workgroup of 256 threads, shared by k_mixture
// (nra_mixture.hip: one fit per workgroup) and k_mixture_boot (nra_bootstrap.hip: the order search of one bootstrap
// replicate per workgroup).  The contract is DESIGN.md section 17 and tests/mixture_ref.py.
// Thread t owns the points t, t + 256, t + 512, ...  KREG > 0 keeps them in registers (N <= 256 * KREG), KREG == 0
// gets them from the kernel's point source on every pass.  Both forms visit a thread's points in the same ascending
// order and run the same operations on each, so a sum is the same chain of additions in either: the thread's partial
// in point order, a butterfly over the 64 lanes, the four waves in wave order through LDS.  Nothing is contracted
// into an fma (pragma below) and nothing is reassociated, so every value is a function of the points and the start
// alone -- not of the path, the kernel, the place in the batch or the run.  No atomics.
// Nothing is kept per point but (KREG > 0) its log-likelihood between the E-step's sum and the M-step's passes: labels
// and responsibilities are recomputed from the component parameters, which live in LDS in two sets (the pass reads
// one and thread 0 writes the other).  A pass handles one component: its 1 + 2 D sums fit in registers for any n.
#ifndef NRA_MIX_BODY_H
#define NRA_MIX_BODY_H
#include "nra_device.h"

#pragma clang fp contract(off)

#define MIX_T NRA_MIX_THREADS
#define MIX_WAVES (MIX_T / WAVE)
#define MIX_C NRA_MIX_MAX_COMPONENTS

template <int D> struct MixParams {
    double mu[MIX_C][D];
    double var[MIX_C][D];
    double inv[MIX_C][D];      // 1 / var
    double a[MIX_C];           // log w - (D log 2 pi + sum log var) / 2
    double w[MIX_C];
};

// the workgroup's sum of V values per thread, the same in every thread.  Fixed order: lanes by butterfly (a + b is
// b + a, so both partners hold the same bits), then waves 0..3.
template <int V> __device__ __forceinline__ void mix_wg_sum(double (&v)[V], double (*red)[5])
{
#pragma unroll
    for (int i = 0; i < V; ++i) {
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) v[i] += __shfl_xor(v[i], m, WAVE);
    }
    const int wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) red[wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) {
        double s = red[0][i];
#pragma unroll
        for (int wv = 1; wv < MIX_WAVES; ++wv) s += red[wv][i];
        v[i] = s;
    }
    __syncthreads();
}

// the point source of a sample that lies in memory: row i of an N x D array
template <int D> struct MixRows {
    const double* __restrict__ X;
    __device__ __forceinline__ void operator()(int i, double (&x)[D]) const
    {
        if constexpr (D == 2) {
            const double2 p = *reinterpret_cast<const double2*>(X + 2 * (size_t)i);
            x[0] = p.x; x[1] = p.y;
        } else {
            x[0] = X[i];
        }
    }
};

// body(k, x) for the thread's points in ascending k (point k * 256 + t)
template <int D, int KREG, class Src, class F>
__device__ __forceinline__ void mix_points(int N, const Src& src, const double (&xr)[KREG > 0 ? KREG : 1][D], F&& body)
{
    const int t = threadIdx.x;
    if constexpr (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k)
            if (k * MIX_T + t < N) body(k, xr[k]);
    } else {
        for (int k = 0, i = t; i < N; ++k, i += MIX_T) {
            double x[D];
            src(i, x);
            body(k, x);
        }
    }
}

// nearest mean by squared distance; a tie goes to the lowest component
template <int D> __device__ __forceinline__ int mix_label(const double (&x)[D], const double (*mu)[D], int n)
{
    int best = 0;
    double bd = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) { const double e = x[a] - mu[0][a]; bd += e * e; }
    for (int c = 1; c < n; ++c) {
        double dd = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) { const double e = x[a] - mu[c][a]; dd += e * e; }
        if (dd < bd) { bd = dd; best = c; }
    }
    return best;
}

template <int D> __device__ __forceinline__ double mix_logp(const double (&x)[D], const MixParams<D>& p, int c)
{
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) { const double e = x[a] - p.mu[c][a]; q += e * e * p.inv[c][a]; }
    return p.a[c] - 0.5 * q;
}

template <int D> __device__ __forceinline__ double mix_lse(const double (&x)[D], const MixParams<D>& p, int n)
{
    double m = mix_logp<D>(x, p, 0);
    for (int c = 1; c < n; ++c) m = fmax(m, mix_logp<D>(x, p, c));
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += exp(mix_logp<D>(x, p, c) - m);
    return m + log(s);
}

// scikit-learn's M-step for diagonal covariance from the sums of r, r x, r x^2 of component c
template <int D> __device__ __forceinline__ void mix_m_step(MixParams<D>& p, int c, const double (&s)[1 + 2 * D], int N)
{
    const double nk = s[0] + 10.0 * 2.220446049250313e-16;
    double logdet = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double mu = s[1 + a] / nk;
        const double var = s[1 + D + a] / nk - mu * mu + 1e-6;
        p.mu[c][a] = mu;
        p.var[c][a] = var;
        p.inv[c][a] = 1.0 / var;
        logdet += log(var);
    }
    p.w[c] = nk / (double)N;
    p.a[c] = log(p.w[c]) - 0.5 * ((double)D * 1.8378770664093453 + logdet);
}

// One fit of n components to the N points of `src` (in xr where KREG > 0) from the rows start_rows[0..n): Lloyd steps
// from the start means, a one-hot M-step, then EM until the mean log-likelihood moves by less than 1e-3.  P: two
// parameter sets in LDS, red: the reduction's LDS; nobody may still read either when the call begins.  On return
// every thread holds the same cur, lb, n_iter and converged, P[cur] is the fitted model and a barrier has passed
// since its last write.
template <int D, int KREG, class Src>
__device__ __forceinline__ void mix_fit(int N, int n, const Src& src, const int32_t* __restrict__ start_rows,
                                        const double (&xr)[KREG > 0 ? KREG : 1][D], double (&lse_r)[KREG > 0 ? KREG : 1],
                                        MixParams<D>* P, double (*red)[5], int& cur_out, double& lb_out, int& n_iter_out,
                                        int& converged_out)
{
    constexpr int V = 1 + 2 * D;
    const int t = threadIdx.x;
    int cur = 0;
    if (t < n) {
        double x[D];
        src(start_rows[t], x);
#pragma unroll
        for (int a = 0; a < D; ++a) P[0].mu[t][a] = x[a];
    }
    __syncthreads();

    // sums of component c over the points labelled c by the means of set `cur`
    auto hard_sums = [&](int c, double (&s)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = 0.0;
        mix_points<D, KREG>(N, src, xr, [&](int, const double (&x)[D]) {
            if (mix_label<D>(x, P[cur].mu, n) == c) {
                s[0] += 1.0;
#pragma unroll
                for (int a = 0; a < D; ++a) { s[1 + a] += x[a]; s[1 + D + a] += x[a] * x[a]; }
            }
        });
        mix_wg_sum<V>(s, red);
    };

    // Lloyd steps: at most 10, stop when no label changes
    for (int it = 0; it < NRA_MIX_LLOYD_STEPS; ++it) {
        for (int c = 0; c < n; ++c) {
            double s[V];
            hard_sums(c, s);
            if (t == 0) {
#pragma unroll
                for (int a = 0; a < D; ++a) P[cur ^ 1].mu[c][a] = s[0] > 0.0 ? s[1 + a] / s[0] : P[cur].mu[c][a];
            }
        }
        __syncthreads();
        double ch[1] = {0.0};
        mix_points<D, KREG>(N, src, xr, [&](int, const double (&x)[D]) {
            if (mix_label<D>(x, P[cur].mu, n) != mix_label<D>(x, P[cur ^ 1].mu, n)) ch[0] += 1.0;
        });
        mix_wg_sum<1>(ch, red);
        cur ^= 1;
        if (ch[0] == 0.0) break;
    }

    // responsibilities = one-hot labels
    for (int c = 0; c < n; ++c) {
        double s[V];
        hard_sums(c, s);
        if (t == 0) mix_m_step<D>(P[cur ^ 1], c, s, N);
    }
    __syncthreads();
    cur ^= 1;

    double lb = 0.0, lb_prev = -__builtin_huge_val();
    int n_iter = 0, converged = 0;
    for (int it = 1; it <= NRA_MIX_MAX_ITER; ++it) {
        double l[1] = {0.0};
        mix_points<D, KREG>(N, src, xr, [&](int k, const double (&x)[D]) {
            const double v = mix_lse<D>(x, P[cur], n);
            if constexpr (KREG > 0) lse_r[k] = v;
            l[0] += v;
        });
        mix_wg_sum<1>(l, red);
        lb = l[0] / (double)N;
        for (int c = 0; c < n; ++c) {
            double s[V];
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] = 0.0;
            mix_points<D, KREG>(N, src, xr, [&](int k, const double (&x)[D]) {
                double v;
                if constexpr (KREG > 0) v = lse_r[k];
                else v = mix_lse<D>(x, P[cur], n);
                const double r = exp(mix_logp<D>(x, P[cur], c) - v);
                s[0] += r;
#pragma unroll
                for (int a = 0; a < D; ++a) { s[1 + a] += r * x[a]; s[1 + D + a] += r * (x[a] * x[a]); }
            });
            mix_wg_sum<V>(s, red);
            if (t == 0) mix_m_step<D>(P[cur ^ 1], c, s, N);
        }
        __syncthreads();
        cur ^= 1;
        n_iter = it;
        if (fabs(lb - lb_prev) < NRA_MIX_TOL) { converged = 1; break; }
        lb_prev = lb;
    }
    cur_out = cur;
    lb_out = lb;
    n_iter_out = n_iter;
    converged_out = converged;
}

#endif  // NRA_MIX_BODY_H
