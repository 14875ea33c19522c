// nra_structure_host.cpp -- C ABI of the repeat structure alignment (nra_read_structure): argument checks, the order of
// the reads (phase capacity, then tract length), the chunks that bound the traceback pointers' device memory, and the
// launches of k_structure (nra_structure.hip).
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

#define STRUCT_HIP_TRY(expr)                                                                     \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? NRA_E_NOMEM : NRA_E_DEVICE,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

const int64_t kPtrBudget = int64_t(1) << 30;    // traceback pointer bytes per chunk (one wave beyond it goes alone)
const int64_t kCodeBudget = int64_t(1) << 28;   // tract bytes per chunk

int base_code(unsigned char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return NRA_STRUCT_CODE_OTHER;
    }
}

// the kernel's phase capacity for motif length p: exact up to 6, then 8, 16, 32, 64
int capacity(int p) { return p <= 6 ? p : p <= 8 ? 8 : p <= 16 ? 16 : p <= 32 ? 32 : 64; }

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

template <class T> struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
};

struct Chunk {
    int P;
    size_t first, last;        // positions [first, last) of the sorted order
};

int run_chunk(const Chunk& ck, const std::vector<int32_t>& order, const char* seqs, const int64_t* seq_off,
              const int32_t* read_motif, const NraStructMotif* dev_motifs, int32_t* edits, int32_t* start_phase,
              uint8_t* path)
{
    const int W = NRA_STRUCT_WORDS(ck.P);
    const size_t n = ck.last - ck.first;
    std::vector<NraStructRead> rd(n);
    int64_t code_bytes = 0, ptr_words = 0;
    for (size_t w0 = 0; w0 < n; w0 += 64) {                      // waves: the first lane holds the longest tract
        const int64_t rows = seq_off[order[ck.first + w0] + 1] - seq_off[order[ck.first + w0]];
        for (size_t l = w0; l < std::min(n, w0 + 64); ++l) {
            const int32_t r = order[ck.first + l];
            rd[l].tract = (uint64_t)code_bytes;
            rd[l].ptr = (uint64_t)ptr_words;
            rd[l].n = (int32_t)(seq_off[r + 1] - seq_off[r]);
            rd[l].motif = read_motif[r];
            code_bytes += round_up(rd[l].n, NRA_STRUCT_BLOCK);
        }
        ptr_words += rows * 64 * W;
    }
    uint8_t lut[256];
    for (int c = 0; c < 256; ++c) lut[c] = (uint8_t)base_code((unsigned char)c);
    std::vector<uint8_t> codes((size_t)code_bytes + NRA_STRUCT_BLOCK, (uint8_t)NRA_STRUCT_CODE_OTHER);
    for (size_t l = 0; l < n; ++l) {
        const int32_t r = order[ck.first + l];
        const unsigned char* s = reinterpret_cast<const unsigned char*>(seqs + seq_off[r]);
        uint8_t* dst = codes.data() + rd[l].tract;
        for (int32_t i = 0; i < rd[l].n; ++i) dst[i] = lut[s[i]];
    }
    DevBuf<NraStructRead> d_rd;
    DevBuf<uint8_t> d_codes, d_path;
    DevBuf<uint32_t> d_ptr;
    DevBuf<int32_t> d_res;
    STRUCT_HIP_TRY(d_rd.alloc(n));
    STRUCT_HIP_TRY(d_codes.alloc(codes.size()));
    STRUCT_HIP_TRY(d_path.alloc(codes.size()));
    STRUCT_HIP_TRY(d_ptr.alloc((size_t)ptr_words));
    STRUCT_HIP_TRY(d_res.alloc(2 * n));
    STRUCT_HIP_TRY(hipMemcpy(d_rd.p, rd.data(), n * sizeof(NraStructRead), hipMemcpyHostToDevice));
    STRUCT_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int e = nra_launch_structure(nullptr, ck.P, (int)n, d_rd.p, dev_motifs, d_codes.p, d_ptr.p, d_path.p, d_res.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_structure: ") + hipGetErrorString((hipError_t)e));
    STRUCT_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> res(2 * n);
    std::vector<uint8_t>& out = codes;                            // the codes are no longer needed
    STRUCT_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    STRUCT_HIP_TRY(hipMemcpy(out.data(), d_path.p, out.size(), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l) {
        const int32_t r = order[ck.first + l];
        edits[r] = res[2 * l];
        start_phase[r] = res[2 * l + 1];
        if (rd[l].n) std::memcpy(path + seq_off[r], out.data() + rd[l].tract, (size_t)rd[l].n);
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_read_structure(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off, int32_t n_reads,
                       const char* seqs, const int64_t* seq_off, const int32_t* read_motif, int32_t* edits,
                       int32_t* start_phase, uint8_t* path)
{
    if (n_motifs < 1) return fail(NRA_E_ARG, "n_motifs must be >= 1");
    if (!motifs || !motif_off) return fail(NRA_E_ARG, "motifs or motif_off is NULL");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (motif_off[0] < 0) return fail(NRA_E_ARG, "negative motif offset");
    for (int32_t m = 0; m < n_motifs; ++m) {
        const int64_t p = motif_off[m + 1] - motif_off[m];
        if (p < 1) return fail(NRA_E_ARG, "motif " + std::to_string(m) + " is empty");
        if (p > NRA_STRUCT_MAX_P)
            return fail(NRA_E_RANGE, "motif " + std::to_string(m) + " is longer than 64 bases");
        for (int64_t i = motif_off[m]; i < motif_off[m + 1]; ++i)
            if (!std::strchr("ACGT", motifs[i]) || motifs[i] == 0)
                return fail(NRA_E_ARG, "motif " + std::to_string(m) + " has a base other than A, C, G, T");
    }
    if (n_reads > 0) {
        if (!seq_off || !read_motif || !edits || !start_phase) return fail(NRA_E_ARG, "NULL read array");
        if (seq_off[0] < 0) return fail(NRA_E_ARG, "negative read offset");
        for (int32_t r = 0; r < n_reads; ++r) {
            const int64_t len = seq_off[r + 1] - seq_off[r];
            if (len < 0) return fail(NRA_E_ARG, "read offsets must not decrease");
            if (len > NRA_STRUCT_MAX_N)
                return fail(NRA_E_RANGE, "tract " + std::to_string(r) + " is longer than 200000 bases");
            if (read_motif[r] < 0 || read_motif[r] >= n_motifs) return fail(NRA_E_ARG, "read_motif out of range");
        }
        if (seq_off[n_reads] > seq_off[0] && (!seqs || !path)) return fail(NRA_E_ARG, "seqs or path is NULL");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    if (n_reads == 0) return NRA_OK;
    STRUCT_HIP_TRY(hipSetDevice(device));
    try {
        // motif masks: eq[c] bit j <=> u[(j - 1) mod p] has code c
        std::vector<NraStructMotif> mo((size_t)n_motifs);
        for (int32_t m = 0; m < n_motifs; ++m) {
            const char* u = motifs + motif_off[m];
            const int p = (int)(motif_off[m + 1] - motif_off[m]);
            NraStructMotif& x = mo[(size_t)m];
            std::memset(&x, 0, sizeof(x));
            x.p = p;
            for (int j = 0; j < p; ++j) x.eq[base_code((unsigned char)u[(j + p - 1) % p])] |= 1ull << j;
        }
        DevBuf<NraStructMotif> d_mo;
        STRUCT_HIP_TRY(d_mo.alloc(mo.size()));
        STRUCT_HIP_TRY(hipMemcpy(d_mo.p, mo.data(), mo.size() * sizeof(NraStructMotif), hipMemcpyHostToDevice));

        // (capacity, length descending, index): the 64 lanes of a wave have one capacity and similar lengths
        std::vector<int32_t> order((size_t)n_reads);
        std::iota(order.begin(), order.end(), 0);
        auto cap_of = [&](int32_t r) { return capacity((int)(motif_off[read_motif[r] + 1] - motif_off[read_motif[r]])); };
        auto len_of = [&](int32_t r) { return seq_off[r + 1] - seq_off[r]; };
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            const int ca = cap_of(a), cb = cap_of(b);
            if (ca != cb) return ca < cb;
            if (len_of(a) != len_of(b)) return len_of(a) > len_of(b);
            return a < b;
        });
        int64_t ptr_budget = kPtrBudget;
        if (const char* e = getenv("NRA_TEST_STRUCT_PTR_BYTES")) ptr_budget = std::max<int64_t>(1, atoll(e));
        // chunks: whole waves of one capacity while the pointers and codes stay within the budgets
        std::vector<Chunk> chunks;
        for (size_t i = 0; i < order.size();) {
            const int P = cap_of(order[i]);
            size_t j = i;
            int64_t ptr_bytes = 0, code_bytes = 0;
            while (j < order.size() && cap_of(order[j]) == P) {
                size_t w1 = j;
                int64_t cb = 0;
                while (w1 < order.size() && w1 < j + 64 && cap_of(order[w1]) == P)
                    cb += round_up(len_of(order[w1++]), NRA_STRUCT_BLOCK);
                const int64_t pb = len_of(order[j]) * 64 * NRA_STRUCT_WORDS(P) * 4;
                if (j > i && (ptr_bytes + pb > ptr_budget || code_bytes + cb > kCodeBudget)) break;
                ptr_bytes += pb; code_bytes += cb;
                j = w1;
            }
            chunks.push_back(Chunk{P, i, j});
            i = j;
        }
        for (const Chunk& ck : chunks) {
            const int rc = run_chunk(ck, order, seqs, seq_off, read_motif, d_mo.p, edits, start_phase, path);
            if (rc != NRA_OK) return rc;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "read structure: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
