// nra_censored_host.cpp -- C ABI of the censored allele fit (nra_censored_fit, nra_censored_posteriors): argument checks,
// one upload, one launch of k_censored_fit (nra_censored.hip) per register class or one of k_censored_resp, one download.
// A fit is one wavefront and shares nothing with another, so a call is never chunked.
// nra_censored_bootstrap: the same checks and those of the index rows; per launch group (whole problems whose records
// and index rows fit a byte budget) one packed upload, one launch of k_censored_boot per register class, one of
// k_censored_pick, one download.  The per-(replicate, n, open) records never leave the device.
#include "nra_host_util.h"

#include <cmath>
#include <cstdint>
#include <cstring>
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

// The model search of n_rep replicates of every problem.  A replicate is a function of its own
// row alone, so the split into launch groups is invisible in the results.
int nra_censored_bootstrap(int device, int64_t n_values, const double* values, int32_t n_problems,
                           const int64_t* prob_off, const int32_t* prob_n, const int32_t* prob_n_exact,
                           const double* prob_tau, const double* prob_ln_n, int32_t n_rep, const int32_t* idx,
                           const int32_t* rep_m, int32_t max_alleles, int32_t max_iter, double tol, int32_t flags,
                           int32_t* status, int32_t* model_n, int32_t* model_open, int32_t* best_start,
                           int32_t* n_iter, double* ll, double* bic, double* nu, double* w)
{
    if (flags & ~NRA_CENS_F_STREAM) return fail(NRA_E_ARG, "unknown flag");
    if (n_rep < 1) return fail(NRA_E_ARG, "fewer than one replicate");
    if (n_rep > NRA_CENS_BOOT_MAX_B) return fail(NRA_E_RANGE, "more than 1000 replicates");
    if (max_alleles < 1 || max_alleles > NRA_CENS_MAX_COMPONENTS) return fail(NRA_E_RANGE, "max_alleles must be in 1..8");
    if (max_iter < 1) return fail(NRA_E_ARG, "max_iter must be >= 1");
    if (max_iter > NRA_CENS_MAX_ITER) return fail(NRA_E_RANGE, "max_iter is more than 500");
    if (!std::isfinite(tol) || tol < 0.0) return fail(NRA_E_ARG, "tol must be finite and >= 0");
    if (int rc = check_problems(n_values, values, n_problems, prob_off, prob_n, prob_n_exact, prob_tau)) return rc;
    if ((int64_t)n_problems * n_rep > INT32_MAX) return fail(NRA_E_RANGE, "more than 2^31 - 1 replicates in all");
    if (n_problems > 0 && (!prob_ln_n || !idx || !rep_m || !status || !model_n || !model_open || !best_start || !n_iter ||
                           !ll || !bic || !nu || !w))
        return fail(NRA_E_ARG, "NULL array");
    std::vector<int64_t> idx_off;
    try {
        idx_off.resize((size_t)n_problems + 1, 0);
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "censored bootstrap: host allocation failed");
    }
    for (int32_t p = 0; p < n_problems; ++p) {
        const std::string who = "problem " + std::to_string(p);
        const int32_t N = prob_n[p], m = prob_n_exact[p];
        if (!std::isfinite(prob_ln_n[p])) return fail(NRA_E_ARG, who + ": lnN is not finite");
        const double* y = values + prob_off[p];
        for (int32_t i = 1; i < N; ++i)
            if (i != m && y[i] < y[i - 1]) return fail(NRA_E_ARG, who + ": its values are not ascending within a part");
        const int32_t* ix = idx + idx_off[(size_t)p];
        for (int32_t b = 0; b < n_rep; ++b) {
            const int32_t* row = ix + (int64_t)b * N;
            int32_t exact = 0;
            for (int32_t j = 0; j < N; ++j) {
                if (row[j] < 0 || row[j] >= N) return fail(NRA_E_ARG, who + ": a resampling index is outside its values");
                if (j > 0 && row[j] < row[j - 1]) return fail(NRA_E_ARG, who + ": a resampling row is not ascending");
                exact += row[j] < m;
            }
            if (rep_m[(int64_t)p * n_rep + b] != exact)
                return fail(NRA_E_ARG, who + ": rep_m disagrees with the resampling row");
        }
        idx_off[(size_t)p + 1] = idx_off[(size_t)p] + (int64_t)n_rep * N;
    }
    if (int rc = use_device(device, n_problems > 0)) return rc;
    if (n_problems == 0) return NRA_OK;
    try {
        const size_t np = (size_t)n_problems, slots = 2 * (size_t)max_alleles;
        // launch groups of whole problems: records and index rows each within the budget, at least one problem
        const int64_t budget = test_bytes("NRA_TEST_CENS_BOOT_BYTES", (int64_t)1 << 30);
        const int64_t rec_bytes_of_problem = (int64_t)n_rep * (int64_t)slots * (int64_t)sizeof(NraCensBootRec);
        DevBuf<char> d_up, d_down;
        DevBuf<NraCensBootRec> d_recs;
        std::vector<char> up, down;
        std::vector<NraCensBootProblem> pr;
        std::vector<int32_t> jobs;
        for (size_t p0 = 0; p0 < np;) {
            size_t p1 = p0;
            int64_t rec_bytes = 0, idx_bytes = 0, n_val = 0;
            while (p1 < np) {
                const int64_t ib = (idx_off[p1 + 1] - idx_off[p1]) * 4;
                if (p1 > p0 && (rec_bytes + rec_bytes_of_problem > budget || idx_bytes + ib > budget)) break;
                rec_bytes += rec_bytes_of_problem;
                idx_bytes += ib;
                n_val += prob_n[p1];
                ++p1;
            }
            const size_t gp = p1 - p0, gr = gp * (size_t)n_rep, r0 = p0 * (size_t)n_rep;
            const size_t n_idx = (size_t)(idx_off[p1] - idx_off[p0]);
            // the problems of the group, their values packed in order; the replicates of one kernel: class -> jobs
            pr.resize(gp);
            int64_t o_val = 0;
            for (size_t p = p0; p < p1; ++p) {
                pr[p - p0] = NraCensBootProblem{o_val, idx_off[p] - idx_off[p0], prob_tau[p], prob_ln_n[p], prob_n[p],
                                                prob_n_exact[p]};
                o_val += prob_n[p];
            }
            const int classes[2] = {NRA_CENS_KREG, 0};
            struct Launch { int kreg; size_t begin, count; };
            std::vector<Launch> launches;
            jobs.clear();
            jobs.reserve(gr);
            for (int kreg : classes) {
                const size_t begin = jobs.size();
                for (size_t p = 0; p < gp; ++p) {
                    const bool reg = !(flags & NRA_CENS_F_STREAM) && pr[p].n_points <= 64 * NRA_CENS_KREG;
                    if ((reg ? NRA_CENS_KREG : 0) == kreg)
                        for (int32_t b = 0; b < n_rep; ++b) jobs.push_back((int32_t)(p * (size_t)n_rep + b));
                }
                if (jobs.size() > begin) launches.push_back({kreg, begin, jobs.size() - begin});
            }
            // one buffer up: values, problems, idx, rep_m, jobs (8-byte parts first)
            const size_t b_y = (size_t)n_val * 8, b_pr = gp * sizeof(NraCensBootProblem), b_idx = n_idx * 4, b_m = gr * 4;
            const size_t o_y = 0, o_pr = o_y + b_y, o_idx = o_pr + b_pr, o_m = o_idx + b_idx, o_jobs = o_m + b_m,
                         up_bytes = o_jobs + gr * 4;
            up.assign(up_bytes, 0);
            for (size_t p = p0; p < p1; ++p)
                std::memcpy(up.data() + o_y + (size_t)pr[p - p0].off * 8, values + prob_off[p], (size_t)prob_n[p] * 8);
            std::memcpy(up.data() + o_pr, pr.data(), b_pr);
            std::memcpy(up.data() + o_idx, idx + idx_off[p0], b_idx);
            std::memcpy(up.data() + o_m, rep_m + r0, b_m);
            std::memcpy(up.data() + o_jobs, jobs.data(), gr * 4);
            // one buffer down: ll, bic, nu, w, then status, n, open, best start, n_iter
            const size_t q_ll = 0, q_bic = q_ll + gr * 8, q_nu = q_bic + gr * 8,
                         q_w = q_nu + gr * 8 * NRA_CENS_MAX_COMPONENTS,
                         q_st = q_w + gr * 8 * (NRA_CENS_MAX_COMPONENTS + 1), q_n = q_st + gr * 4, q_o = q_n + gr * 4,
                         q_bs = q_o + gr * 4, q_it = q_bs + gr * 4, down_bytes = q_it + gr * 4;
            NRA_HIP_TRY(d_up.ensure(up_bytes));
            NRA_HIP_TRY(d_down.ensure(down_bytes));
            NRA_HIP_TRY(d_recs.ensure(gr * slots));
            NRA_HIP_TRY((hipError_t)nra_copy_h2d(d_up.p, up.data(), up_bytes));
            const NraCensBootProblem* g_pr = reinterpret_cast<const NraCensBootProblem*>(d_up.p + o_pr);
            const int32_t* g_m = reinterpret_cast<const int32_t*>(d_up.p + o_m);
            for (const Launch& l : launches) {
                const int e = nra_launch_censored_boot(
                    nullptr, l.kreg, (int)l.count, reinterpret_cast<const int32_t*>(d_up.p + o_jobs) + l.begin, n_rep,
                    max_alleles, g_pr, reinterpret_cast<const double*>(d_up.p + o_y),
                    reinterpret_cast<const int32_t*>(d_up.p + o_idx), g_m, max_iter, tol, d_recs.p);
                if (e != 0) return fail(NRA_E_DEVICE, std::string("k_censored_boot: ") + hipGetErrorString((hipError_t)e));
            }
            const int e = nra_launch_censored_pick(
                nullptr, (int)gr, n_rep, max_alleles, g_pr, g_m, d_recs.p, reinterpret_cast<int32_t*>(d_down.p + q_st),
                reinterpret_cast<int32_t*>(d_down.p + q_n), reinterpret_cast<int32_t*>(d_down.p + q_o),
                reinterpret_cast<int32_t*>(d_down.p + q_bs), reinterpret_cast<int32_t*>(d_down.p + q_it),
                reinterpret_cast<double*>(d_down.p + q_ll), reinterpret_cast<double*>(d_down.p + q_bic),
                reinterpret_cast<double*>(d_down.p + q_nu), reinterpret_cast<double*>(d_down.p + q_w));
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_censored_pick: ") + hipGetErrorString((hipError_t)e));
            NRA_HIP_TRY(hipStreamSynchronize(nullptr));
            down.resize(down_bytes);
            NRA_HIP_TRY((hipError_t)nra_copy_d2h(down.data(), d_down.p, down_bytes));
            std::memcpy(ll + r0, down.data() + q_ll, gr * 8);
            std::memcpy(bic + r0, down.data() + q_bic, gr * 8);
            std::memcpy(nu + r0 * NRA_CENS_MAX_COMPONENTS, down.data() + q_nu, gr * 8 * NRA_CENS_MAX_COMPONENTS);
            std::memcpy(w + r0 * (NRA_CENS_MAX_COMPONENTS + 1), down.data() + q_w, gr * 8 * (NRA_CENS_MAX_COMPONENTS + 1));
            std::memcpy(status + r0, down.data() + q_st, gr * 4);
            std::memcpy(model_n + r0, down.data() + q_n, gr * 4);
            std::memcpy(model_open + r0, down.data() + q_o, gr * 4);
            std::memcpy(best_start + r0, down.data() + q_bs, gr * 4);
            std::memcpy(n_iter + r0, down.data() + q_it, gr * 4);
            p0 = p1;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "censored bootstrap: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
