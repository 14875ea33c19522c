// nra_period_host.cpp -- C ABI of the tandem period spectra (nra_tract_periods): argument checks, the order of the
// tracts (length, descending), the chunks that bound the device and host buffers (codes and results), and the launches
// of k_tract_periods (nra_period.hip).  NRA_DEBUG in the environment traces every chunk on stderr.
#include "nra_host_util.h"

#include <algorithm>
#include <cstdio>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const int64_t kChunkBudget = int64_t(1) << 28;  // bytes per chunk (one tract beyond it goes alone)
const int kGroupsPerCU = 8;                     // workgroups of 4 waves resident per CU

// what a tract costs of a chunk's budget: its codes and its two rows of results (on the device, and again on the host)
int64_t tract_cost(int64_t len)
{
    return round_up(len, NRA_PERIOD_ALIGN) + 2 * NRA_PERIOD_MAX_P * (int64_t)sizeof(int32_t);
}

int run_chunk(size_t first, size_t last, const std::vector<int32_t>& order, const char* seqs, const int64_t* seq_off,
              int n_cu, int32_t max_period, int32_t* match, int32_t* valid)
{
    const size_t n = last - first;
    if (getenv("NRA_DEBUG")) fprintf(stderr, "nra_tract_periods: chunk of %zu tract(s)\n", n);
    std::vector<NraPeriodTract> tr(n);
    int64_t code_bytes = 0;
    for (size_t l = 0; l < n; ++l) {
        const int32_t t = order[first + l];
        tr[l].off = (uint64_t)code_bytes;
        tr[l].n = (int32_t)(seq_off[t + 1] - seq_off[t]);
        tr[l].pad = 0;
        code_bytes += round_up(tr[l].n, NRA_PERIOD_ALIGN);
    }
    std::vector<uint8_t> codes((size_t)code_bytes + NRA_PERIOD_PAD, (uint8_t)kCodeOther);
    for (size_t l = 0; l < n; ++l) encode(codes.data() + tr[l].off, seqs + seq_off[order[first + l]], tr[l].n);
    DevBuf<NraPeriodTract> d_tr;
    DevBuf<uint8_t> d_codes;
    DevBuf<int32_t> d_match, d_valid;
    NRA_HIP_TRY(d_tr.alloc(n));
    NRA_HIP_TRY(d_codes.alloc(codes.size()));
    NRA_HIP_TRY(d_match.alloc(n * NRA_PERIOD_MAX_P));
    NRA_HIP_TRY(d_valid.alloc(n * NRA_PERIOD_MAX_P));
    NRA_HIP_TRY(hipMemcpy(d_tr.p, tr.data(), n * sizeof(NraPeriodTract), hipMemcpyHostToDevice));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int64_t groups = ((int64_t)n + 3) / 4;
    const int grid = (int)std::min<int64_t>(groups, (int64_t)n_cu * kGroupsPerCU);
    const int e = nra_launch_tract_periods(nullptr, grid, (int)n, d_tr.p, d_codes.p, d_match.p, d_valid.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_tract_periods: ") + hipGetErrorString((hipError_t)e));
    NRA_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> m(n * NRA_PERIOD_MAX_P), v(n * NRA_PERIOD_MAX_P);
    NRA_HIP_TRY(hipMemcpy(m.data(), d_match.p, m.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    NRA_HIP_TRY(hipMemcpy(v.data(), d_valid.p, v.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l) {
        const int64_t t = order[first + l];
        for (int p = 0; p < max_period; ++p) {
            match[t * max_period + p] = m[l * NRA_PERIOD_MAX_P + (size_t)p];
            valid[t * max_period + p] = v[l * NRA_PERIOD_MAX_P + (size_t)p];
        }
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_tract_periods(int device, int32_t n_tracts, const char* seqs, const int64_t* seq_off, int32_t max_period,
                      int32_t* match, int32_t* valid)
{
    if (max_period < 1 || max_period > NRA_PERIOD_MAX_P) return fail(NRA_E_ARG, "max_period must be in 1..64");
    if (n_tracts < 0) return fail(NRA_E_ARG, "negative tract count");
    if (n_tracts > 0) {
        if (!seq_off || !match || !valid) return fail(NRA_E_ARG, "NULL tract array");
        if (int rc = check_tract_offsets(n_tracts, seq_off, NRA_PERIOD_MAX_N, "tract")) return rc;
        if (seq_off[n_tracts] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device, n_tracts > 0)) return rc;
    if (n_tracts == 0) return NRA_OK;
    try {
        int n_cu = 0;
        NRA_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n_cu, 1);

        // length descending, then index: the four tracts of a workgroup step run about as long
        std::vector<int32_t> order((size_t)n_tracts);
        std::iota(order.begin(), order.end(), 0);
        auto len_of = [&](int32_t t) { return seq_off[t + 1] - seq_off[t]; };
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len_of(a) > len_of(b); });
        const int64_t budget = test_bytes("NRA_TEST_PERIOD_CHUNK_BYTES", kChunkBudget);
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            int64_t bytes = 0;
            while (j < order.size()) {
                const int64_t b = tract_cost(len_of(order[j]));
                if (j > i && bytes + b > budget) break;
                bytes += b;
                ++j;
            }
            const int rc = run_chunk(i, j, order, seqs, seq_off, n_cu, max_period, match, valid);
            if (rc != NRA_OK) return rc;
            i = j;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "tract periods: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
