// nra_segment_host.cpp -- C ABI of the motif-run alignment (nra_tract_segments): argument checks, the motif sets as state
// masks, the order of the tracts (state class, then tract length), the chunks that bound the traceback pointers' device
// memory, and the launches of k_segment (nra_segment.hip).
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

#define SEG_HIP_TRY(expr)                                                                        \
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

// the kernel's state class for a set of S states
int state_class(int S) { return S <= 8 ? 8 : S <= 16 ? 16 : 32; }

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

template <class T> struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
};

struct Chunk {
    int SC;
    size_t first, last;        // positions [first, last) of the sorted order
};

int run_chunk(const Chunk& ck, const std::vector<int32_t>& order, const char* seqs, const int64_t* seq_off,
              const int32_t* tract_set, const NraSegSet* dev_sets, int switch_cost, int32_t* edits,
              int32_t* start_phase, int32_t* start_motif, uint8_t* path, uint8_t* motif_of)
{
    const int W = NRA_SEG_WORDS(ck.SC);
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
            rd[l].motif = tract_set[r];
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
    DevBuf<uint8_t> d_codes, d_path, d_which;
    DevBuf<uint32_t> d_ptr;
    DevBuf<int32_t> d_res;
    SEG_HIP_TRY(d_rd.alloc(n));
    SEG_HIP_TRY(d_codes.alloc(codes.size()));
    SEG_HIP_TRY(d_path.alloc(codes.size()));
    SEG_HIP_TRY(d_which.alloc(codes.size()));
    SEG_HIP_TRY(d_ptr.alloc((size_t)ptr_words));
    SEG_HIP_TRY(d_res.alloc(4 * n));
    SEG_HIP_TRY(hipMemcpy(d_rd.p, rd.data(), n * sizeof(NraStructRead), hipMemcpyHostToDevice));
    SEG_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int e = nra_launch_segment(nullptr, ck.SC, (int)n, d_rd.p, dev_sets, d_codes.p, switch_cost, d_ptr.p, d_path.p,
                                     d_which.p, d_res.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_segment: ") + hipGetErrorString((hipError_t)e));
    SEG_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> res(4 * n);
    std::vector<uint8_t>& out = codes;                            // the codes are no longer needed
    std::vector<uint8_t> mot(codes.size());
    SEG_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    SEG_HIP_TRY(hipMemcpy(out.data(), d_path.p, out.size(), hipMemcpyDeviceToHost));
    SEG_HIP_TRY(hipMemcpy(mot.data(), d_which.p, mot.size(), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l) {
        const int32_t r = order[ck.first + l];
        edits[r] = res[4 * l];
        start_phase[r] = res[4 * l + 1];
        start_motif[r] = res[4 * l + 2];
        if (rd[l].n) {
            std::memcpy(path + seq_off[r], out.data() + rd[l].tract, (size_t)rd[l].n);
            std::memcpy(motif_of + seq_off[r], mot.data() + rd[l].tract, (size_t)rd[l].n);
        }
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_tract_segments(int device, int32_t n_sets, const int32_t* set_motif_off, const char* motifs,
                       const int64_t* motif_off, int32_t n_tracts, const char* seqs, const int64_t* seq_off,
                       const int32_t* tract_set, int32_t switch_cost, int32_t* edits, int32_t* start_phase,
                       int32_t* start_motif, uint8_t* path, uint8_t* motif_of)
{
    if (n_sets < 1) return fail(NRA_E_ARG, "n_sets must be >= 1");
    if (!set_motif_off || !motifs || !motif_off) return fail(NRA_E_ARG, "set_motif_off, motifs or motif_off is NULL");
    if (n_tracts < 0) return fail(NRA_E_ARG, "negative tract count");
    if (switch_cost <= 0) return fail(NRA_E_ARG, "switch_cost must be >= 1");
    if (switch_cost > NRA_SEG_MAX_SWITCH) return fail(NRA_E_RANGE, "switch_cost is larger than 1000");
    if (set_motif_off[0] < 0 || motif_off[0] < 0) return fail(NRA_E_ARG, "negative offset");
    std::vector<int> states((size_t)n_sets);
    for (int32_t q = 0; q < n_sets; ++q) {
        const int64_t M = (int64_t)set_motif_off[q + 1] - set_motif_off[q];
        if (M < 1) return fail(NRA_E_ARG, "set " + std::to_string(q) + " is empty");
        if (M > NRA_SEG_MAX_MOTIFS) return fail(NRA_E_RANGE, "set " + std::to_string(q) + " has more than 8 motifs");
        int64_t S = 0;
        for (int32_t m = set_motif_off[q]; m < set_motif_off[q + 1]; ++m) {
            const int64_t p = motif_off[m + 1] - motif_off[m];
            if (p < 1) return fail(NRA_E_ARG, "motif " + std::to_string(m) + " is empty");
            for (int64_t i = motif_off[m]; i < motif_off[m + 1]; ++i)
                if (!std::strchr("ACGT", motifs[i]) || motifs[i] == 0)
                    return fail(NRA_E_ARG, "motif " + std::to_string(m) + " has a base other than A, C, G, T");
            S += p;
        }
        if (S > NRA_SEG_MAX_STATES)
            return fail(NRA_E_RANGE, "set " + std::to_string(q) + " has more than 32 motif bases in all");
        states[(size_t)q] = (int)S;
    }
    if (n_tracts > 0) {
        if (!seq_off || !tract_set || !edits || !start_phase || !start_motif) return fail(NRA_E_ARG, "NULL tract array");
        if (seq_off[0] < 0) return fail(NRA_E_ARG, "negative tract offset");
        for (int32_t r = 0; r < n_tracts; ++r) {
            const int64_t len = seq_off[r + 1] - seq_off[r];
            if (len < 0) return fail(NRA_E_ARG, "tract offsets must not decrease");
            if (len > NRA_STRUCT_MAX_N)
                return fail(NRA_E_RANGE, "tract " + std::to_string(r) + " is longer than 200000 bases");
            if (tract_set[r] < 0 || tract_set[r] >= n_sets) return fail(NRA_E_ARG, "tract_set out of range");
        }
        if (seq_off[n_tracts] > seq_off[0] && (!seqs || !path || !motif_of))
            return fail(NRA_E_ARG, "seqs, path or motif_of is NULL");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    if (n_tracts == 0) return NRA_OK;
    SEG_HIP_TRY(hipSetDevice(device));
    try {
        // state masks: state g = (motif m, phase j) in (m, j) order; eq[c] bit g <=> u_m[(j - 1) mod p_m] has code c
        std::vector<NraSegSet> ss((size_t)n_sets);
        for (int32_t q = 0; q < n_sets; ++q) {
            NraSegSet& x = ss[(size_t)q];
            std::memset(&x, 0, sizeof(x));
            x.S = states[(size_t)q];
            int g = 0;
            for (int32_t m = set_motif_off[q]; m < set_motif_off[q + 1]; ++m) {
                const char* u = motifs + motif_off[m];
                const int p = (int)(motif_off[m + 1] - motif_off[m]);
                x.first |= 1u << g;
                x.last |= 1u << (g + p - 1);
                for (int j = 0; j < p; ++j, ++g) x.eq[base_code((unsigned char)u[(j + p - 1) % p])] |= 1u << g;
            }
        }
        DevBuf<NraSegSet> d_sets;
        SEG_HIP_TRY(d_sets.alloc(ss.size()));
        SEG_HIP_TRY(hipMemcpy(d_sets.p, ss.data(), ss.size() * sizeof(NraSegSet), hipMemcpyHostToDevice));

        // (state class, length descending, index): the 64 lanes of a wave have one class and similar lengths
        std::vector<int32_t> order((size_t)n_tracts);
        std::iota(order.begin(), order.end(), 0);
        auto cls_of = [&](int32_t r) { return state_class(states[(size_t)tract_set[r]]); };
        auto len_of = [&](int32_t r) { return seq_off[r + 1] - seq_off[r]; };
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            const int ca = cls_of(a), cb = cls_of(b);
            if (ca != cb) return ca < cb;
            if (len_of(a) != len_of(b)) return len_of(a) > len_of(b);
            return a < b;
        });
        int64_t ptr_budget = kPtrBudget;
        if (const char* e = getenv("NRA_TEST_SEG_PTR_BYTES")) ptr_budget = std::max<int64_t>(1, atoll(e));
        // chunks: whole waves of one class while the pointers and codes stay within the budgets
        std::vector<Chunk> chunks;
        for (size_t i = 0; i < order.size();) {
            const int SC = cls_of(order[i]);
            size_t j = i;
            int64_t ptr_bytes = 0, code_bytes = 0;
            while (j < order.size() && cls_of(order[j]) == SC) {
                size_t w1 = j;
                int64_t cb = 0;
                while (w1 < order.size() && w1 < j + 64 && cls_of(order[w1]) == SC)
                    cb += round_up(len_of(order[w1++]), NRA_STRUCT_BLOCK);
                const int64_t pb = len_of(order[j]) * 64 * NRA_SEG_WORDS(SC) * 4;
                if (j > i && (ptr_bytes + pb > ptr_budget || code_bytes + cb > kCodeBudget)) break;
                ptr_bytes += pb; code_bytes += cb;
                j = w1;
            }
            chunks.push_back(Chunk{SC, i, j});
            i = j;
        }
        for (const Chunk& ck : chunks) {
            const int rc = run_chunk(ck, order, seqs, seq_off, tract_set, d_sets.p, switch_cost, edits, start_phase,
                                     start_motif, path, motif_of);
            if (rc != NRA_OK) return rc;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "tract segments: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
