// nra_censored_host.cpp -- C ABI of the censored allele fit (nra_censored_fit, nra_censored_posteriors): argument checks,
// one upload, one launch of k_censored_fit (nra_censored.hip) per register class or one of k_censored_resp, one download.
// A fit is one wavefront and shares nothing with another, so a call is never chunked.
#include "nra_host_util.h"

#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

// the problems of either entry point
int check_problems(int64_t n_values, const double* values, int32_t n_problems, const int64_t* prob_off,
                   const int32_t* prob_n, const int32_t* prob_n_exact, const double* prob_tau)
{
    if (n_values < 0 || n_problems < 0) return fail(NRA_E_ARG, "negative count");
    if (n_problems > 0 && (!prob_off || !prob_n || !prob_n_exact || !prob_tau)) return fail(NRA_E_ARG, "NULL problem array");
    if (n_values > 0 && !values) return fail(NRA_E_ARG, "values is NULL");
    for (int32_t p = 0; p < n_problems; ++p) {
        const std::string who = "problem " + std::to_string(p);
        if (prob_n[p] < 1) return fail(NRA_E_ARG, who + ": no values");
        if (prob_n[p] > NRA_CENS_MAX_N) return fail(NRA_E_RANGE, who + ": more than 1048576 values");
        if (prob_n_exact[p] < 1 || prob_n_exact[p] > prob_n[p])
            return fail(NRA_E_ARG, who + ": n_exact must be in 1..N");
        if (!std::isfinite(prob_tau[p]) || !(prob_tau[p] > 0.0)) return fail(NRA_E_ARG, who + ": tau must be finite and > 0");
        if (prob_off[p] < 0 || prob_off[p] > n_values || prob_n[p] > n_values - prob_off[p])
            return fail(NRA_E_ARG, who + ": its values are outside the buffer");
        const double* y = values + prob_off[p];
        for (int32_t i = 0; i < prob_n[p]; ++i)
            if (!std::isfinite(y[i])) return fail(NRA_E_ARG, who + ": a value is not finite");
    }
    return NRA_OK;
}

// the models of either entry point: item f = (n[f], open[f]) on problem problem_of(f)
template <class ProblemOf>
int check_models(const char* noun, int32_t n_items, const int32_t* n, const int32_t* open, int32_t n_problems,
                 const int32_t* prob_n, const int32_t* prob_n_exact, ProblemOf problem_of)
{
    for (int32_t f = 0; f < n_items; ++f) {
        const std::string who = std::string(noun) + " " + std::to_string(f);
        const int32_t p = problem_of(f);
        if (p < 0 || p >= n_problems) return fail(NRA_E_ARG, who + ": problem out of range");
        if (n[f] < 1 || n[f] > NRA_CENS_MAX_COMPONENTS) return fail(NRA_E_RANGE, who + ": n must be in 1..8");
        if (open[f] != 0 && open[f] != 1) return fail(NRA_E_ARG, who + ": open must be 0 or 1");
        if (open[f] == 1 && prob_n_exact[p] == prob_n[p])
            return fail(NRA_E_ARG, who + ": an open component on a problem without a bound");
    }
    return NRA_OK;
}

bool all_finite(const double* v, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int nra_censored_fit(int device, int64_t n_values, const double* values, int32_t n_problems, const int64_t* prob_off,
                     const int32_t* prob_n, const int32_t* prob_n_exact, const double* prob_tau, int32_t n_fits,
                     const int32_t* fit_problem, const int32_t* fit_n, const int32_t* fit_open, const double* starts,
                     int32_t max_iter, double tol, int32_t flags, double* ll, double* w, double* nu, int32_t* n_iter,
                     int32_t* converged)
{
    if (n_fits < 0) return fail(NRA_E_ARG, "negative count");
    if (flags & ~NRA_CENS_F_STREAM) return fail(NRA_E_ARG, "unknown flag");
    if (max_iter < 1) return fail(NRA_E_ARG, "max_iter must be >= 1");
    if (max_iter > NRA_CENS_MAX_ITER) return fail(NRA_E_RANGE, "max_iter is more than 500");
    if (!std::isfinite(tol) || tol < 0.0) return fail(NRA_E_ARG, "tol must be finite and >= 0");
    if (int rc = check_problems(n_values, values, n_problems, prob_off, prob_n, prob_n_exact, prob_tau)) return rc;
    int64_t n_nu = 0, n_w = 0;
    if (n_fits > 0) {
        if (!fit_problem || !fit_n || !fit_open || !starts || !ll || !w || !nu || !n_iter || !converged)
            return fail(NRA_E_ARG, "NULL fit array");
        if (int rc = check_models("fit", n_fits, fit_n, fit_open, n_problems, prob_n, prob_n_exact,
                                  [&](int32_t f) { return fit_problem[f]; }))
            return rc;
        for (int32_t f = 0; f < n_fits; ++f) {
            n_nu += fit_n[f];
            n_w += fit_n[f] + fit_open[f];
        }
        if (!all_finite(starts, n_nu)) return fail(NRA_E_ARG, "a start mean is not finite");
    }
    if (int rc = use_device(device, n_fits > 0)) return rc;
    if (n_fits == 0) return NRA_OK;
    try {
        const size_t nf = (size_t)n_fits;
        std::vector<NraCensFit> ft(nf);
        int64_t o_nu = 0, o_w = 0;
        for (size_t f = 0; f < nf; ++f) {
            const int32_t p = fit_problem[f];
            ft[f] = NraCensFit{prob_off[p], o_nu, o_w, 0, prob_tau[p], prob_n[p], prob_n_exact[p], fit_n[f], fit_open[f]};
            o_nu += fit_n[f];
            o_w += fit_n[f] + fit_open[f];
        }
        // the fits of one kernel, in the caller's order: register class -> ids
        const int classes[2] = {NRA_CENS_KREG, 0};
        std::vector<int32_t> ids;
        ids.reserve(nf);
        struct Launch { int kreg; size_t begin, count; };
        std::vector<Launch> launches;
        for (int kreg : classes) {
            const size_t begin = ids.size();
            for (size_t f = 0; f < nf; ++f) {
                const bool reg = !(flags & NRA_CENS_F_STREAM) && ft[f].n_points <= 64 * NRA_CENS_KREG;
                if ((reg ? NRA_CENS_KREG : 0) == kreg) ids.push_back((int32_t)f);
            }
            if (ids.size() > begin) launches.push_back({kreg, begin, ids.size() - begin});
        }
        DevBuf<double> d_y, d_st, d_ll, d_w, d_nu;
        DevBuf<NraCensFit> d_ft;
        DevBuf<int32_t> d_ids, d_it;
        NRA_HIP_TRY(d_y.alloc((size_t)n_values));
        NRA_HIP_TRY(d_st.alloc((size_t)n_nu));
        NRA_HIP_TRY(d_ft.alloc(nf));
        NRA_HIP_TRY(d_ids.alloc(nf));
        NRA_HIP_TRY(d_ll.alloc(nf));
        NRA_HIP_TRY(d_w.alloc((size_t)n_w));
        NRA_HIP_TRY(d_nu.alloc((size_t)n_nu));
        NRA_HIP_TRY(d_it.alloc(2 * nf));
        NRA_HIP_TRY(hipMemcpy(d_y.p, values, (size_t)n_values * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_st.p, starts, (size_t)n_nu * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_ft.p, ft.data(), nf * sizeof(NraCensFit), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_ids.p, ids.data(), nf * sizeof(int32_t), hipMemcpyHostToDevice));
        for (const Launch& l : launches) {
            const int e = nra_launch_censored_fit(nullptr, l.kreg, (int)l.count, d_ids.p + l.begin, d_ft.p, d_y.p, d_st.p,
                                                  max_iter, tol, d_ll.p, d_w.p, d_nu.p, d_it.p);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_censored_fit: ") + hipGetErrorString((hipError_t)e));
        }
        NRA_HIP_TRY(hipStreamSynchronize(nullptr));
        std::vector<int32_t> it(2 * nf);
        NRA_HIP_TRY(hipMemcpy(ll, d_ll.p, nf * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(w, d_w.p, (size_t)n_w * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(nu, d_nu.p, (size_t)n_nu * sizeof(double), hipMemcpyDeviceToHost));
        NRA_HIP_TRY(hipMemcpy(it.data(), d_it.p, it.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t f = 0; f < nf; ++f) {
            n_iter[f] = it[2 * f];
            converged[f] = it[2 * f + 1];
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "censored fit: host allocation failed");
    }
    return NRA_OK;
}

int nra_censored_posteriors(int device, int64_t n_values, const double* values, int32_t n_problems,
                            const int64_t* prob_off, const int32_t* prob_n, const int32_t* prob_n_exact,
                            const double* prob_tau, const int32_t* model_n, const int32_t* model_open, const double* w,
                            const double* nu, int64_t n_resp, double* resp)
{
    if (n_resp < 0) return fail(NRA_E_ARG, "negative count");
    if (int rc = check_problems(n_values, values, n_problems, prob_off, prob_n, prob_n_exact, prob_tau)) return rc;
    int64_t n_nu = 0, n_w = 0, need = 0;
    if (n_problems > 0) {
        if (!model_n || !model_open || !w || !nu) return fail(NRA_E_ARG, "NULL model array");
        if (int rc = check_models("model", n_problems, model_n, model_open, n_problems, prob_n, prob_n_exact,
                                  [](int32_t p) { return p; }))
            return rc;
        for (int32_t p = 0; p < n_problems; ++p) {
            n_nu += model_n[p];
            n_w += model_n[p] + model_open[p];
            need += (int64_t)prob_n[p] * (model_n[p] + model_open[p]);
        }
        if (!all_finite(nu, n_nu)) return fail(NRA_E_ARG, "a mean is not finite");
        for (int64_t i = 0; i < n_w; ++i)
            if (!std::isfinite(w[i]) || !(w[i] > 0.0)) return fail(NRA_E_ARG, "a weight is not finite and > 0");
        if (need > n_resp) return fail(NRA_E_RANGE, "resp holds fewer entries than the posteriors need");
        if (!resp) return fail(NRA_E_ARG, "resp is NULL");
    }
    if (int rc = use_device(device, n_problems > 0)) return rc;
    if (n_problems == 0) return NRA_OK;
    try {
        const size_t np = (size_t)n_problems;
        std::vector<NraCensFit> md(np);
        int64_t o_nu = 0, o_w = 0, o_r = 0;
        for (size_t p = 0; p < np; ++p) {
            md[p] = NraCensFit{prob_off[p], o_nu, o_w, o_r, prob_tau[p], prob_n[p], prob_n_exact[p], model_n[p],
                               model_open[p]};
            o_nu += model_n[p];
            o_w += model_n[p] + model_open[p];
            o_r += (int64_t)prob_n[p] * (model_n[p] + model_open[p]);
        }
        DevBuf<double> d_y, d_w, d_nu, d_r;
        DevBuf<NraCensFit> d_md;
        NRA_HIP_TRY(d_y.alloc((size_t)n_values));
        NRA_HIP_TRY(d_w.alloc((size_t)n_w));
        NRA_HIP_TRY(d_nu.alloc((size_t)n_nu));
        NRA_HIP_TRY(d_r.alloc((size_t)need));
        NRA_HIP_TRY(d_md.alloc(np));
        NRA_HIP_TRY(hipMemcpy(d_y.p, values, (size_t)n_values * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_w.p, w, (size_t)n_w * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_nu.p, nu, (size_t)n_nu * sizeof(double), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_md.p, md.data(), np * sizeof(NraCensFit), hipMemcpyHostToDevice));
        const int e = nra_launch_censored_resp(nullptr, n_problems, d_md.p, d_y.p, d_w.p, d_nu.p, d_r.p);
        if (e != 0) return fail(NRA_E_DEVICE, std::string("k_censored_resp: ") + hipGetErrorString((hipError_t)e));
        NRA_HIP_TRY(hipStreamSynchronize(nullptr));
        NRA_HIP_TRY(hipMemcpy(resp, d_r.p, (size_t)need * sizeof(double), hipMemcpyDeviceToHost));
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "censored posteriors: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
