// nra_mixture_host.cpp -- C ABI of the mixture fits (nra_mixture_fit): argument checks, the samples packed at even
// offsets, one upload, one launch of k_mixture (nra_mixture.hip) per (axes, register class), one download of the
// per-fit results.  A fit is one workgroup and shares nothing with another, so a call is never chunked.
#include "nra_host_util.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

// the register class of a problem of n points: 256 * kreg holds it; 0 streams
int kreg_of(int64_t n, int32_t flags)
{
    if (flags & NRA_MIX_STREAM) return 0;
    if (!(flags & NRA_MIX_ONE_CLASS) && n <= (int64_t)NRA_MIX_THREADS * NRA_MIX_KREG_SMALL) return NRA_MIX_KREG_SMALL;
    return n <= (int64_t)NRA_MIX_THREADS * NRA_MIX_KREG ? NRA_MIX_KREG : 0;
}

}  // namespace

extern "C" {

int nra_mixture_fit(int device, int64_t n_samples, const double* samples, int32_t n_problems, const int64_t* prob_off,
                    const int32_t* prob_n, const int32_t* prob_d, int32_t n_fits, const int32_t* fit_problem,
                    const int32_t* fit_n, const int32_t* starts, int32_t flags, double* lb, double* w, double* mu,
                    double* var, int32_t* n_iter, int32_t* converged)
{
    if (n_samples < 0 || n_problems < 0 || n_fits < 0) return fail(NRA_E_ARG, "negative count");
    if (flags & ~(NRA_MIX_STREAM | NRA_MIX_ONE_CLASS)) return fail(NRA_E_ARG, "unknown flag");
    if (n_problems > 0 && (!prob_off || !prob_n || !prob_d)) return fail(NRA_E_ARG, "NULL problem array");
    if (n_samples > 0 && !samples) return fail(NRA_E_ARG, "samples is NULL");
    for (int32_t p = 0; p < n_problems; ++p) {
        const std::string who = "problem " + std::to_string(p);
        if (prob_d[p] != 1 && prob_d[p] != 2) return fail(NRA_E_ARG, who + ": d must be 1 or 2");
        if (prob_n[p] < 1) return fail(NRA_E_ARG, who + ": no points");
        if (prob_n[p] > NRA_MIX_MAX_N) return fail(NRA_E_RANGE, who + ": more than 4194304 points");
        if (prob_off[p] < 0 || prob_off[p] > n_samples || (int64_t)prob_n[p] * prob_d[p] > n_samples - prob_off[p])
            return fail(NRA_E_ARG, who + ": its rows are outside the samples");
        const double* x = samples + prob_off[p];
        for (int64_t i = 0, e = (int64_t)prob_n[p] * prob_d[p]; i < e; ++i)
            if (!std::isfinite(x[i])) return fail(NRA_E_ARG, who + ": a value is not finite");
    }
    if (n_fits > 0) {
        if (!fit_problem || !fit_n || !starts || !lb || !w || !mu || !var || !n_iter || !converged)
            return fail(NRA_E_ARG, "NULL fit array");
        int64_t off = 0;
        for (int32_t f = 0; f < n_fits; ++f) {
            const std::string who = "fit " + std::to_string(f);
            if (fit_problem[f] < 0 || fit_problem[f] >= n_problems) return fail(NRA_E_ARG, who + ": problem out of range");
            if (fit_n[f] < 1) return fail(NRA_E_ARG, who + ": n must be >= 1");
            if (fit_n[f] > prob_n[fit_problem[f]]) return fail(NRA_E_ARG, who + ": more components than points");
            if (fit_n[f] > NRA_MIX_MAX_COMPONENTS) return fail(NRA_E_RANGE, who + ": more than 32 components");
            for (int32_t c = 0; c < fit_n[f]; ++c)
                if (starts[off + c] < 0 || starts[off + c] >= prob_n[fit_problem[f]])
                    return fail(NRA_E_ARG, who + ": start index out of range");
            off += fit_n[f];
        }
    }
    if (int rc = use_device(device, n_fits > 0)) return rc;
    if (n_fits == 0) return NRA_OK;
    try {
        const size_t np = (size_t)n_problems, nf = (size_t)n_fits;
        // every problem at an even offset: a row of two doubles is one aligned 16-byte load
        std::vector<NraMixProblem> pr(np);
        int64_t total = 0;
        for (size_t p = 0; p < np; ++p) {
            pr[p].off = (uint64_t)total;
            pr[p].n = prob_n[p];
            pr[p].d = prob_d[p];
            total += ((int64_t)prob_n[p] * prob_d[p] + 1) / 2 * 2;
        }
        std::vector<double> packed((size_t)total, 0.0);
        for (size_t p = 0; p < np; ++p)
            std::memcpy(packed.data() + pr[p].off, samples + prob_off[p], (size_t)prob_n[p] * prob_d[p] * sizeof(double));
        std::vector<NraMixFit> ft(nf);
        int64_t n_comp = 0;
        for (size_t f = 0; f < nf; ++f) {
            ft[f].off = n_comp;
            ft[f].problem = fit_problem[f];
            ft[f].n = fit_n[f];
            n_comp += fit_n[f];
        }
        // the fits of one kernel, in the caller's order: (axes, register class) -> ids
        const int classes[3] = {NRA_MIX_KREG_SMALL, NRA_MIX_KREG, 0};
        std::vector<int32_t> ids;
        ids.reserve(nf);
        struct Launch { int d, kreg; size_t begin, count; };
        std::vector<Launch> launches;
        for (int d = 1; d <= 2; ++d)
            for (int kreg : classes) {
                const size_t begin = ids.size();
                for (size_t f = 0; f < nf; ++f)
                    if (prob_d[fit_problem[f]] == d && kreg_of(prob_n[fit_problem[f]], flags) == kreg)
                        ids.push_back((int32_t)f);
                if (ids.size() > begin) launches.push_back({d, kreg, begin, ids.size() - begin});
            }
        DevBuf<double> d_x, d_lb, d_w, d_mu, d_var;
        DevBuf<NraMixProblem> d_pr;
        DevBuf<NraMixFit> d_ft;
        DevBuf<int32_t> d_ids, d_st, d_it;
        NRA_HIP_TRY(d_x.alloc(packed.size()));
        NRA_HIP_TRY(d_pr.alloc(np));
        NRA_HIP_TRY(d_ft.alloc(nf));
        NRA_HIP_TRY(d_ids.alloc(nf));
        NRA_HIP_TRY(d_st.alloc((size_t)n_comp));
        NRA_HIP_TRY(d_lb.alloc(nf));
        NRA_HIP_TRY(d_w.alloc((size_t)n_comp));
        NRA_HIP_TRY(d_mu.alloc(2 * (size_t)n_comp));
        NRA_HIP_TRY(d_var.alloc(2 * (size_t)n_comp));
        NRA_HIP_TRY(d_it.alloc(2 * nf));
        NRA_HIP_TRY(hipMemcpy(d_x.p, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_pr.p, pr.data(), np * sizeof(NraMixProblem), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_ft.p, ft.data(), nf * sizeof(NraMixFit), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_ids.p, ids.data(), nf * sizeof(int32_t), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_st.p, starts, (size_t)n_comp * sizeof(int32_t), hipMemcpyHostToDevice));
        for (const Launch& l : launches) {
            const int e = nra_launch_mixture(nullptr, l.d, l.kreg, (int)l.count, d_ids.p + l.begin, d_ft.p, d_pr.p, d_x.p,
                                             d_st.p, d_lb.p, d_w.p, d_mu.p, d_var.p, d_it.p);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_mixture: ") + hipGetErrorString((hipError_t)e));
        }
        NRA_HIP_TRY(hipStreamSynchronize(nullptr));
        std::vector<int32_t> it(2 * nf);
        NRA_HIP_TRY(hipMemcpy(lb, d_lb.p, nf * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(w, d_w.p, (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(mu, d_mu.p, 2 * (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(var, d_var.p, 2 * (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(it.data(), d_it.p, it.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t f = 0; f < nf; ++f) {
            n_iter[f] = it[2 * f];
            converged[f] = it[2 * f + 1];
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "mixture fit: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
