// nra_extend_host.cpp -- C ABI of the anchored wraparound extension (nra_extend_tracts): argument checks, the order of
// the reads (phase capacity, then tract length), one upload of all tracts, one launch of k_extend (nra_extend.hip) per
// capacity, one download of the four results per read.  Nothing is kept per row, so a call is never chunked.
#include "nanorepeat_amd.h"
#include "nra_internal.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

namespace {

int fail(int code, const std::string& msg) { return nra_set_error(code, msg.c_str()); }

#define EXT_HIP_TRY(expr)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? NRA_E_NOMEM : NRA_E_DEVICE,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

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

}  // namespace

extern "C" {

int nra_extend_tracts(int device, int32_t n_motifs, const char* motifs, const int64_t* motif_off, int32_t n_reads,
                      const char* seqs, const int64_t* seq_off, const int32_t* read_motif, int32_t match,
                      int32_t mismatch, int32_t gap, int32_t* score, int32_t* end, int32_t* end_phase,
                      int32_t* motif_bases)
{
    if (n_motifs < 1) return fail(NRA_E_ARG, "n_motifs must be >= 1");
    if (!motifs || !motif_off) return fail(NRA_E_ARG, "motifs or motif_off is NULL");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (match < 1 || match > 127) return fail(NRA_E_ARG, "match must be in 1..127");
    if (mismatch < 0 || mismatch > 127) return fail(NRA_E_ARG, "mismatch must be in 0..127");
    if (gap < 1 || gap > 127) return fail(NRA_E_ARG, "gap must be in 1..127");
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
        if (!seq_off || !read_motif || !score || !end || !end_phase || !motif_bases)
            return fail(NRA_E_ARG, "NULL read array");
        if (seq_off[0] < 0) return fail(NRA_E_ARG, "negative read offset");
        for (int32_t r = 0; r < n_reads; ++r) {
            const int64_t len = seq_off[r + 1] - seq_off[r];
            if (len < 0) return fail(NRA_E_ARG, "read offsets must not decrease");
            if (len > NRA_STRUCT_MAX_N)
                return fail(NRA_E_RANGE, "tract " + std::to_string(r) + " is longer than 200000 bases");
            if (read_motif[r] < 0 || read_motif[r] >= n_motifs) return fail(NRA_E_ARG, "read_motif out of range");
        }
        if (seq_off[n_reads] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    if (n_reads == 0) return NRA_OK;
    EXT_HIP_TRY(hipSetDevice(device));
    try {
        // motif masks: eq[c] bit j <=> u[(j - 1) mod p] has code c; bits j >= p stay 0 (the kernel relies on it)
        std::vector<NraStructMotif> mo((size_t)n_motifs);
        for (int32_t m = 0; m < n_motifs; ++m) {
            const char* u = motifs + motif_off[m];
            const int p = (int)(motif_off[m + 1] - motif_off[m]);
            NraStructMotif& x = mo[(size_t)m];
            std::memset(&x, 0, sizeof(x));
            x.p = p;
            for (int j = 0; j < p; ++j) x.eq[base_code((unsigned char)u[(j + p - 1) % p])] |= 1ull << j;
        }
        // (capacity, length descending, index): the 64 lanes of a wave have one capacity and similar lengths
        const size_t n = (size_t)n_reads;
        std::vector<int32_t> order(n);
        std::iota(order.begin(), order.end(), 0);
        auto cap_of = [&](int32_t r) { return capacity((int)(motif_off[read_motif[r] + 1] - motif_off[read_motif[r]])); };
        auto len_of = [&](int32_t r) { return seq_off[r + 1] - seq_off[r]; };
        std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
            const int cx = cap_of(x), cy = cap_of(y);
            if (cx != cy) return cx < cy;
            if (len_of(x) != len_of(y)) return len_of(x) > len_of(y);
            return x < y;
        });
        // tracts as one code byte per base at 16-byte offsets, padded by one block: the kernel loads whole blocks
        std::vector<NraStructRead> rd(n);
        int64_t code_bytes = 0;
        for (size_t l = 0; l < n; ++l) {
            const int32_t r = order[l];
            rd[l].tract = (uint64_t)code_bytes;
            rd[l].ptr = 0;
            rd[l].n = (int32_t)len_of(r);
            rd[l].motif = read_motif[r];
            code_bytes += round_up(rd[l].n, NRA_STRUCT_BLOCK);
        }
        uint8_t lut[256];
        for (int c = 0; c < 256; ++c) lut[c] = (uint8_t)base_code((unsigned char)c);
        std::vector<uint8_t> codes((size_t)code_bytes + NRA_STRUCT_BLOCK, (uint8_t)NRA_STRUCT_CODE_OTHER);
        for (size_t l = 0; l < n; ++l) {
            const unsigned char* s = reinterpret_cast<const unsigned char*>(seqs + seq_off[order[l]]);
            uint8_t* dst = codes.data() + rd[l].tract;
            for (int32_t i = 0; i < rd[l].n; ++i) dst[i] = lut[s[i]];
        }
        DevBuf<NraStructMotif> d_mo;
        DevBuf<NraStructRead> d_rd;
        DevBuf<uint8_t> d_codes;
        DevBuf<int32_t> d_res;
        EXT_HIP_TRY(d_mo.alloc(mo.size()));
        EXT_HIP_TRY(d_rd.alloc(n));
        EXT_HIP_TRY(d_codes.alloc(codes.size()));
        EXT_HIP_TRY(d_res.alloc(4 * n));
        EXT_HIP_TRY(hipMemcpy(d_mo.p, mo.data(), mo.size() * sizeof(NraStructMotif), hipMemcpyHostToDevice));
        EXT_HIP_TRY(hipMemcpy(d_rd.p, rd.data(), n * sizeof(NraStructRead), hipMemcpyHostToDevice));
        EXT_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
        for (size_t i = 0; i < n;) {                                  // one launch per capacity
            const int P = cap_of(order[i]);
            size_t j = i;
            while (j < n && cap_of(order[j]) == P) ++j;
            const int e = nra_launch_extend(nullptr, P, (int)(j - i), d_rd.p + i, d_mo.p, d_codes.p, match, mismatch,
                                            gap, d_res.p + 4 * i);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_extend: ") + hipGetErrorString((hipError_t)e));
            i = j;
        }
        EXT_HIP_TRY(hipStreamSynchronize(nullptr));
        std::vector<int32_t> res(4 * n);
        EXT_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t l = 0; l < n; ++l) {
            const int32_t r = order[l];
            score[r] = res[4 * l];
            end[r] = res[4 * l + 1];
            end_phase[r] = res[4 * l + 2];
            motif_bases[r] = res[4 * l + 3];
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "extend tracts: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
