// nra_bootstrap_host.cpp -- C ABI of the bootstrap of the mixture fits (nra_mixture_bootstrap): argument checks, one
// upload of everything the replicates read, one launch of k_mixture_boot (nra_bootstrap.hip) per (axes, register
// class), one download of the per-replicate results.  A replicate is one workgroup and shares nothing with another,
// so a call is never chunked.
#include "nra_host_util.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

// the register class of a sample of n points: 256 * kreg holds it; 0 rebuilds the points on every pass
int kreg_of(int64_t n, int32_t flags)
{
    if (flags & NRA_MIX_STREAM) return 0;
    if (!(flags & NRA_MIX_ONE_CLASS) && n <= (int64_t)NRA_MIX_THREADS * NRA_MIX_KREG_SMALL) return NRA_MIX_KREG_SMALL;
    return n <= (int64_t)NRA_MIX_THREADS * NRA_MIX_KREG ? NRA_MIX_KREG : 0;
}

// the start rows of a problem: orders max(first_n, 2) .. n_cap, ten starts each, n rows per start
int64_t start_rows_of(int32_t first_n, int32_t n_cap)
{
    int64_t rows = 0;
    for (int32_t n = std::max(first_n, 2); n <= n_cap; ++n) rows += (int64_t)NRA_BOOT_STARTS * n;
    return rows;
}

bool all_finite(const double* v, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline size_t pad8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int nra_mixture_bootstrap(int device, int64_t n_x, const double* x, int64_t n_z, const double* z, int32_t n_problems,
                          const int32_t* prob_m, const int32_t* prob_d, const int64_t* prob_x_off,
                          const int64_t* prob_z_off, const double* prob_e, const double* prob_zo,
                          const int32_t* prob_first_n, const int32_t* prob_n_cap, const int32_t* prob_max_n,
                          const int64_t* prob_start_off, int64_t n_starts, const int32_t* starts, int32_t n_rep,
                          const int32_t* idx, int32_t flags, int32_t* status, int32_t* order, int32_t* best_start,
                          double* lb, double* w, double* mu, double* var)
{
    if (n_x < 0 || n_z < 0 || n_problems < 0 || n_starts < 0) return fail(NRA_E_ARG, "negative count");
    if (flags & ~(NRA_MIX_STREAM | NRA_MIX_ONE_CLASS)) return fail(NRA_E_ARG, "unknown flag");
    if (n_rep < 1) return fail(NRA_E_ARG, "fewer than one replicate");
    if (n_rep > NRA_BOOT_MAX_B) return fail(NRA_E_RANGE, "more than 1000 replicates");
    if ((int64_t)n_problems * n_rep > INT32_MAX) return fail(NRA_E_RANGE, "more than 2^31 - 1 replicates in all");
    if (n_problems > 0 && (!prob_m || !prob_d || !prob_x_off || !prob_z_off || !prob_e || !prob_zo || !prob_first_n ||
                           !prob_n_cap || !prob_max_n || !prob_start_off || !x || !z || !idx || !status || !order ||
                           !best_start || !lb || !w || !mu || !var))
        return fail(NRA_E_ARG, "NULL array");
    for (int32_t p = 0; p < n_problems; ++p) {
        const std::string who = "problem " + std::to_string(p);
        if (prob_d[p] != 1 && prob_d[p] != 2) return fail(NRA_E_ARG, who + ": d must be 1 or 2");
        if (prob_m[p] < 1) return fail(NRA_E_ARG, who + ": no reads");
        if ((int64_t)prob_m[p] * NRA_BOOT_COPIES > NRA_MIX_MAX_N) return fail(NRA_E_RANGE, who + ": more than 4194304 points");
        if (prob_first_n[p] < 1 || prob_first_n[p] > 2 || prob_n_cap[p] < 1 || prob_max_n[p] < prob_n_cap[p])
            return fail(NRA_E_ARG, who + ": orders must satisfy first_n = 1 or 2, 1 <= n_cap <= max_n");
        if (prob_n_cap[p] > NRA_MIX_MAX_COMPONENTS) return fail(NRA_E_RANGE, who + ": more than 32 components");
    }
    std::vector<int64_t> idx_off;
    try {
        idx_off.resize((size_t)n_problems + 1, 0);
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "mixture bootstrap: host allocation failed");
    }
    for (int32_t p = 0; p < n_problems; ++p) {
        const std::string who = "problem " + std::to_string(p);
        const int64_t m = prob_m[p], md = m * prob_d[p], n = m * NRA_BOOT_COPIES;
        if (prob_x_off[p] < 0 || prob_x_off[p] > n_x || md > n_x - prob_x_off[p])
            return fail(NRA_E_ARG, who + ": its sizes are outside x");
        if (prob_z_off[p] < 0 || prob_z_off[p] > n_z || md * NRA_BOOT_COPIES > n_z - prob_z_off[p])
            return fail(NRA_E_ARG, who + ": its noise is outside z");
        const int64_t rows = start_rows_of(prob_first_n[p], prob_n_cap[p]);
        if (prob_start_off[p] < 0 || prob_start_off[p] > n_starts || rows > n_starts - prob_start_off[p])
            return fail(NRA_E_ARG, who + ": its start rows are outside starts");
        if (rows > 0 && !starts) return fail(NRA_E_ARG, "starts is NULL");
        if (!std::isfinite(prob_e[p]) || !std::isfinite(prob_zo[p]) || !all_finite(x + prob_x_off[p], md) ||
            !all_finite(z + prob_z_off[p], md * NRA_BOOT_COPIES))
            return fail(NRA_E_ARG, who + ": a value is not finite");
        for (int64_t i = 0; i < rows; ++i)
            if (starts[prob_start_off[p] + i] < 0 || starts[prob_start_off[p] + i] >= n)
                return fail(NRA_E_ARG, who + ": start row out of range");
        const int32_t* ix = idx + idx_off[(size_t)p];
        for (int64_t i = 0, e = m * n_rep; i < e; ++i)
            if (ix[i] < 0 || ix[i] >= m) return fail(NRA_E_ARG, who + ": a resampling index is outside its reads");
        idx_off[(size_t)p + 1] = idx_off[(size_t)p] + m * n_rep;
    }
    if (int rc = use_device(device, n_problems > 0)) return rc;
    if (n_problems == 0) return NRA_OK;
    try {
        const size_t np = (size_t)n_problems, nr = np * (size_t)n_rep;
        std::vector<NraBootProblem> pr(np);
        int64_t n_comp = 0;
        for (size_t p = 0; p < np; ++p) {
            pr[p] = NraBootProblem{prob_x_off[p], prob_z_off[p], idx_off[p], prob_start_off[p],
                                   (int64_t)p * n_rep, n_comp, prob_e[p], prob_zo[p], prob_m[p], prob_d[p],
                                   prob_first_n[p], prob_n_cap[p], prob_max_n[p], 0};
            n_comp += (int64_t)n_rep * prob_n_cap[p];
        }
        // the replicates of one kernel, problems in the caller's order: (axes, register class) -> jobs
        const int classes[3] = {NRA_MIX_KREG_SMALL, NRA_MIX_KREG, 0};
        std::vector<int32_t> jobs;
        jobs.reserve(nr);
        struct Launch { int d, kreg; size_t begin, count; };
        std::vector<Launch> launches;
        for (int d = 1; d <= 2; ++d)
            for (int kreg : classes) {
                const size_t begin = jobs.size();
                for (size_t p = 0; p < np; ++p)
                    if (prob_d[p] == d && kreg_of((int64_t)prob_m[p] * NRA_BOOT_COPIES, flags) == kreg)
                        for (int32_t b = 0; b < n_rep; ++b) jobs.push_back((int32_t)(p * (size_t)n_rep + b));
                if (jobs.size() > begin) launches.push_back({d, kreg, begin, jobs.size() - begin});
            }
        // one buffer up: x, z, problems, idx, starts, jobs -- every part at a multiple of 8 bytes
        const size_t n_idx = (size_t)idx_off[np];
        const size_t b_x = (size_t)n_x * 8, b_z = (size_t)n_z * 8, b_pr = np * sizeof(NraBootProblem),
                     b_idx = pad8(n_idx * 4), b_st = pad8((size_t)n_starts * 4), b_jobs = pad8(nr * 4);
        const size_t o_x = 0, o_z = o_x + b_x, o_pr = o_z + b_z, o_idx = o_pr + b_pr, o_st = o_idx + b_idx,
                     o_jobs = o_st + b_st, up_bytes = o_jobs + b_jobs;
        std::vector<char> up(up_bytes, 0);
        if (b_x) std::memcpy(up.data() + o_x, x, b_x);
        if (b_z) std::memcpy(up.data() + o_z, z, b_z);
        std::memcpy(up.data() + o_pr, pr.data(), b_pr);
        if (n_idx) std::memcpy(up.data() + o_idx, idx, n_idx * 4);
        if (n_starts) std::memcpy(up.data() + o_st, starts, (size_t)n_starts * 4);
        std::memcpy(up.data() + o_jobs, jobs.data(), nr * 4);
        // one buffer down: lb, w, mu, var, then status, order, best start
        const size_t nc = (size_t)n_comp;
        const size_t q_lb = 0, q_w = q_lb + nr * 8, q_mu = q_w + nc * 8, q_var = q_mu + 2 * nc * 8,
                     q_status = q_var + 2 * nc * 8, q_order = q_status + nr * 4, q_best = q_order + nr * 4,
                     down_bytes = q_best + nr * 4;
        DevBuf<char> d_up, d_down;
        NRA_HIP_TRY(d_up.alloc(up_bytes));
        NRA_HIP_TRY(d_down.alloc(down_bytes));
        NRA_HIP_TRY((hipError_t)nra_copy_h2d(d_up.p, up.data(), up_bytes));
        NRA_HIP_TRY(hipMemsetAsync(d_down.p, 0, down_bytes, nullptr));
        for (const Launch& l : launches) {
            const int e = nra_launch_mixture_boot(
                nullptr, l.d, l.kreg, (int)l.count, reinterpret_cast<const int32_t*>(d_up.p + o_jobs) + l.begin, n_rep,
                reinterpret_cast<const NraBootProblem*>(d_up.p + o_pr), reinterpret_cast<const double*>(d_up.p + o_x),
                reinterpret_cast<const double*>(d_up.p + o_z), reinterpret_cast<const int32_t*>(d_up.p + o_idx),
                reinterpret_cast<const int32_t*>(d_up.p + o_st), reinterpret_cast<int32_t*>(d_down.p + q_status),
                reinterpret_cast<int32_t*>(d_down.p + q_order), reinterpret_cast<int32_t*>(d_down.p + q_best),
                reinterpret_cast<double*>(d_down.p + q_lb), reinterpret_cast<double*>(d_down.p + q_w),
                reinterpret_cast<double*>(d_down.p + q_mu), reinterpret_cast<double*>(d_down.p + q_var));
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_mixture_boot: ") + hipGetErrorString((hipError_t)e));
        }
        NRA_HIP_TRY(hipStreamSynchronize(nullptr));
        std::vector<char> down(down_bytes);
        NRA_HIP_TRY((hipError_t)nra_copy_d2h(down.data(), d_down.p, down_bytes));
        std::memcpy(lb, down.data() + q_lb, nr * 8);
        std::memcpy(w, down.data() + q_w, nc * 8);
        std::memcpy(mu, down.data() + q_mu, 2 * nc * 8);
        std::memcpy(var, down.data() + q_var, 2 * nc * 8);
        std::memcpy(status, down.data() + q_status, nr * 4);
        std::memcpy(order, down.data() + q_order, nr * 4);
        std::memcpy(best_start, down.data() + q_best, nr * 4);
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "mixture bootstrap: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
