// nra_motif_host.cpp -- C ABI of the tandem motif discovery (nra_tract_motifs): argument checks, the class tables,
// the order of the tracts (length, descending), the chunks that bound the device buffers, and the launches of
// k_tract_motifs (nra_motif.hip).
#include "nra_host_util.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const int64_t kCodeBudget = int64_t(1) << 28;   // tract bytes per chunk (one tract beyond it goes alone)
const int kGroupsPerCU = 5;                     // workgroups of 4 waves resident per CU (26 KiB of LDS each)

int code_offset(int p) { return ((1 << (2 * p)) - 4) / 3; }

// Lyndon words of 1..6 bases: dense_of[code_offset(p) + code] = dense id (-1 for a code that is not a class), and the
// inverse (p, code) per dense id, in (p, code) order
void class_tables(std::vector<int16_t>& dense_of, std::vector<int8_t>& p_of, std::vector<int32_t>& code_of)
{
    dense_of.assign(NRA_MOTIF_CODES, -1);
    p_of.clear();
    code_of.clear();
    for (int p = 1; p <= NRA_MOTIF_MAX_P; ++p) {
        const uint32_t mask = (1u << (2 * p)) - 1u;
        for (uint32_t w = 0; w <= mask; ++w) {
            bool lyndon = true;
            for (int r = 1; r < p && lyndon; ++r) {
                const uint32_t x = ((w << (2 * r)) | (w >> (2 * (p - r)))) & mask;
                lyndon = x > w;                     // strictly smaller than every other rotation
            }
            if (!lyndon) continue;
            dense_of[(size_t)(code_offset(p) + (int)w)] = (int16_t)p_of.size();
            p_of.push_back((int8_t)p);
            code_of.push_back((int32_t)w);
        }
    }
}

struct Outputs {
    int32_t max_p, top_n;
    int32_t *n_tandem, *top_code, *top_count;
    int8_t* top_p;
    const int8_t* p_of;
    const int32_t* code_of;
};

int run_chunk(size_t first, size_t last, const std::vector<int32_t>& order, const char* seqs, const int64_t* seq_off,
              const int16_t* dev_dense, int n_cu, const Outputs& o)
{
    const size_t n = last - first;
    std::vector<NraMotifTract> tr(n);
    int64_t code_bytes = 0;
    for (size_t l = 0; l < n; ++l) {
        const int32_t t = order[first + l];
        tr[l].off = (uint64_t)code_bytes;
        tr[l].n = (int32_t)(seq_off[t + 1] - seq_off[t]);
        tr[l].pad = 0;
        code_bytes += round_up(tr[l].n, NRA_MOTIF_BLOCK);
    }
    std::vector<uint8_t> codes((size_t)code_bytes + NRA_MOTIF_PAD, (uint8_t)NRA_MOTIF_CODE_OTHER);
    for (size_t l = 0; l < n; ++l) encode(codes.data() + tr[l].off, seqs + seq_off[order[first + l]], tr[l].n);
    DevBuf<NraMotifTract> d_tr;
    DevBuf<uint8_t> d_codes;
    DevBuf<int32_t> d_tandem;
    DevBuf<uint32_t> d_key;
    NRA_HIP_TRY(d_tr.alloc(n));
    NRA_HIP_TRY(d_codes.alloc(codes.size()));
    NRA_HIP_TRY(d_tandem.alloc(n * NRA_MOTIF_MAX_P));
    NRA_HIP_TRY(d_key.alloc(n * NRA_MOTIF_MAX_TOP));
    NRA_HIP_TRY(hipMemcpy(d_tr.p, tr.data(), n * sizeof(NraMotifTract), hipMemcpyHostToDevice));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int64_t groups = ((int64_t)n + 3) / 4;
    const int grid = (int)std::min<int64_t>(groups, (int64_t)n_cu * kGroupsPerCU);
    const int e = nra_launch_tract_motifs(nullptr, grid, (int)n, d_tr.p, d_codes.p, dev_dense, o.max_p, o.top_n,
                                          d_tandem.p, d_key.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_tract_motifs: ") + hipGetErrorString((hipError_t)e));
    NRA_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> tandem(n * NRA_MOTIF_MAX_P);
    std::vector<uint32_t> key(n * NRA_MOTIF_MAX_TOP);
    NRA_HIP_TRY(hipMemcpy(tandem.data(), d_tandem.p, tandem.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    NRA_HIP_TRY(hipMemcpy(key.data(), d_key.p, key.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l) {
        const int64_t t = order[first + l];
        for (int p = 0; p < o.max_p; ++p) o.n_tandem[t * o.max_p + p] = tandem[l * NRA_MOTIF_MAX_P + (size_t)p];
        for (int q = 0; q < o.top_n; ++q) {
            const uint32_t k = key[l * NRA_MOTIF_MAX_TOP + (size_t)q];
            const int64_t at = t * o.top_n + q;
            if (k == 0u) {
                o.top_p[at] = 0; o.top_code[at] = -1; o.top_count[at] = 0;
            } else {
                const int id = 1023 - (int)(k & 1023u);
                o.top_p[at] = o.p_of[id]; o.top_code[at] = o.code_of[id]; o.top_count[at] = (int32_t)(k >> 10);
            }
        }
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_tract_motifs(int device, int32_t n_tracts, const char* seqs, const int64_t* seq_off, int32_t max_period,
                     int32_t top_n, int32_t* n_tandem, int8_t* top_p, int32_t* top_code, int32_t* top_count)
{
    if (max_period < 1 || max_period > NRA_MOTIF_MAX_P) return fail(NRA_E_ARG, "max_period must be in 1..6");
    if (top_n < 1 || top_n > NRA_MOTIF_MAX_TOP) return fail(NRA_E_ARG, "top_n must be in 1..8");
    if (n_tracts < 0) return fail(NRA_E_ARG, "negative tract count");
    if (n_tracts > 0) {
        if (!seq_off || !n_tandem || !top_p || !top_code || !top_count) return fail(NRA_E_ARG, "NULL tract array");
        if (int rc = check_tract_offsets(n_tracts, seq_off, NRA_MOTIF_MAX_N, "tract")) return rc;
        if (seq_off[n_tracts] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device, n_tracts > 0)) return rc;
    if (n_tracts == 0) return NRA_OK;
    try {
        std::vector<int16_t> dense_of;
        std::vector<int8_t> p_of;
        std::vector<int32_t> code_of;
        class_tables(dense_of, p_of, code_of);
        DevBuf<int16_t> d_dense;
        NRA_HIP_TRY(d_dense.alloc(dense_of.size()));
        NRA_HIP_TRY(hipMemcpy(d_dense.p, dense_of.data(), dense_of.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        int n_cu = 0;
        NRA_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n_cu, 1);

        // length descending, then index: the four tracts of a workgroup step run about as long
        std::vector<int32_t> order((size_t)n_tracts);
        std::iota(order.begin(), order.end(), 0);
        auto len_of = [&](int32_t t) { return seq_off[t + 1] - seq_off[t]; };
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len_of(a) > len_of(b); });
        const int64_t budget = test_bytes("NRA_TEST_MOTIF_CHUNK_BYTES", kCodeBudget);
        const Outputs o{max_period, top_n, n_tandem, top_code, top_count, top_p, p_of.data(), code_of.data()};
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            int64_t bytes = 0;
            while (j < order.size()) {
                const int64_t b = round_up(len_of(order[j]), NRA_MOTIF_BLOCK);
                if (j > i && bytes + b > budget) break;
                bytes += b;
                ++j;
            }
            const int rc = run_chunk(i, j, order, seqs, seq_off, d_dense.p, n_cu, o);
            if (rc != NRA_OK) return rc;
            i = j;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "tract motifs: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
