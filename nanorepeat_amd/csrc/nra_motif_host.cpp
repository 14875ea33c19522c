// nra_motif_host.cpp -- C ABI of the tandem motif discovery (nra_tract_motifs): argument checks, the class tables,
// the order of the tracts (length, descending), the chunks that bound the device buffers, and the launches of
// k_tract_motifs (nra_motif.hip).
#include "nanorepeat_amd.h"
#include "nra_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

namespace {

int fail(int code, const std::string& msg) { return nra_set_error(code, msg.c_str()); }

#define MOTIF_HIP_TRY(expr)                                                                      \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? NRA_E_NOMEM : NRA_E_DEVICE,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

const int64_t kCodeBudget = int64_t(1) << 28;   // tract bytes per chunk (one tract beyond it goes alone)
const int kGroupsPerCU = 5;                     // workgroups of 4 waves resident per CU (26 KiB of LDS each)

int base_code(unsigned char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return NRA_MOTIF_CODE_OTHER;
    }
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

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

template <class T> struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
};

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
    uint8_t lut[256];
    for (int c = 0; c < 256; ++c) lut[c] = (uint8_t)base_code((unsigned char)c);
    std::vector<uint8_t> codes((size_t)code_bytes + NRA_MOTIF_PAD, (uint8_t)NRA_MOTIF_CODE_OTHER);
    for (size_t l = 0; l < n; ++l) {
        const int32_t t = order[first + l];
        const unsigned char* s = reinterpret_cast<const unsigned char*>(seqs + seq_off[t]);
        uint8_t* dst = codes.data() + tr[l].off;
        for (int32_t i = 0; i < tr[l].n; ++i) dst[i] = lut[s[i]];
    }
    DevBuf<NraMotifTract> d_tr;
    DevBuf<uint8_t> d_codes;
    DevBuf<int32_t> d_tandem;
    DevBuf<uint32_t> d_key;
    MOTIF_HIP_TRY(d_tr.alloc(n));
    MOTIF_HIP_TRY(d_codes.alloc(codes.size()));
    MOTIF_HIP_TRY(d_tandem.alloc(n * NRA_MOTIF_MAX_P));
    MOTIF_HIP_TRY(d_key.alloc(n * NRA_MOTIF_MAX_TOP));
    MOTIF_HIP_TRY(hipMemcpy(d_tr.p, tr.data(), n * sizeof(NraMotifTract), hipMemcpyHostToDevice));
    MOTIF_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int64_t groups = ((int64_t)n + 3) / 4;
    const int grid = (int)std::min<int64_t>(groups, (int64_t)n_cu * kGroupsPerCU);
    const int e = nra_launch_tract_motifs(nullptr, grid, (int)n, d_tr.p, d_codes.p, dev_dense, o.max_p, o.top_n,
                                          d_tandem.p, d_key.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_tract_motifs: ") + hipGetErrorString((hipError_t)e));
    MOTIF_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> tandem(n * NRA_MOTIF_MAX_P);
    std::vector<uint32_t> key(n * NRA_MOTIF_MAX_TOP);
    MOTIF_HIP_TRY(hipMemcpy(tandem.data(), d_tandem.p, tandem.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    MOTIF_HIP_TRY(hipMemcpy(key.data(), d_key.p, key.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
        if (seq_off[0] < 0) return fail(NRA_E_ARG, "negative tract offset");
        for (int32_t t = 0; t < n_tracts; ++t) {
            const int64_t len = seq_off[t + 1] - seq_off[t];
            if (len < 0) return fail(NRA_E_ARG, "tract offsets must not decrease");
            if (len > NRA_MOTIF_MAX_N)
                return fail(NRA_E_RANGE, "tract " + std::to_string(t) + " is longer than 200000 bases");
        }
        if (seq_off[n_tracts] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    if (n_tracts == 0) return NRA_OK;
    MOTIF_HIP_TRY(hipSetDevice(device));
    try {
        std::vector<int16_t> dense_of;
        std::vector<int8_t> p_of;
        std::vector<int32_t> code_of;
        class_tables(dense_of, p_of, code_of);
        DevBuf<int16_t> d_dense;
        MOTIF_HIP_TRY(d_dense.alloc(dense_of.size()));
        MOTIF_HIP_TRY(hipMemcpy(d_dense.p, dense_of.data(), dense_of.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        int n_cu = 0;
        MOTIF_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n_cu, 1);

        // length descending, then index: the four tracts of a workgroup step run about as long
        std::vector<int32_t> order((size_t)n_tracts);
        std::iota(order.begin(), order.end(), 0);
        auto len_of = [&](int32_t t) { return seq_off[t + 1] - seq_off[t]; };
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len_of(a) > len_of(b); });
        int64_t budget = kCodeBudget;
        if (const char* e = getenv("NRA_TEST_MOTIF_CHUNK_BYTES")) budget = std::max<int64_t>(1, atoll(e));
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
