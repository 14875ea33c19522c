// nra_lane_host.h -- the host plan of the kernels that give a tract to a lane (k_structure, k_segment, k_extend): the
// order of the tracts (kernel class, then length), their layout and codes, the chunks that bound the traceback
// pointers' device memory, and one run of a range of the order: upload, launch, download, scatter.
#ifndef NRA_LANE_HOST_H
#define NRA_LANE_HOST_H
#include "nra_host_util.h"

#include <numeric>
#include <vector>

namespace nra_host {

const int64_t kPtrBudget = int64_t(1) << 30;    // traceback pointer bytes per chunk (one wave beyond it goes alone)
const int64_t kCodeBudget = int64_t(1) << 28;   // tract bytes per chunk

// eq[c] bit j <=> u[(j - 1) mod p] has code c; bits j >= p stay 0 (k_extend relies on it)
inline std::vector<NraStructMotif> motif_masks(int32_t n_motifs, const char* motifs, const int64_t* motif_off)
{
    std::vector<NraStructMotif> mo((size_t)n_motifs);
    for (int32_t m = 0; m < n_motifs; ++m) {
        const char* u = motifs + motif_off[m];
        const int p = (int)(motif_off[m + 1] - motif_off[m]);
        NraStructMotif& x = mo[(size_t)m];
        std::memset(&x, 0, sizeof(x));
        x.p = p;
        for (int j = 0; j < p; ++j) x.eq[kBase.of[(unsigned char)u[(j + p - 1) % p]]] |= 1ull << j;
    }
    return mo;
}

// the kernels' phase capacity for motif length p: exact up to 6, then 8, 16, 32, 64
inline int capacity(int p) { return p <= 6 ? p : p <= 8 ? 8 : p <= 16 ? 16 : p <= 32 ? 32 : 64; }

// (class, length descending, index): the 64 lanes of a wave have one class and similar lengths
template <class ClassOf> std::vector<int32_t> lane_order(int32_t n, const int64_t* seq_off, ClassOf class_of)
{
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    auto len_of = [&](int32_t r) { return seq_off[r + 1] - seq_off[r]; };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const int ca = class_of(a), cb = class_of(b);
        if (ca != cb) return ca < cb;
        if (len_of(a) != len_of(b)) return len_of(a) > len_of(b);
        return a < b;
    });
    return order;
}

struct Chunk {
    int cls;
    size_t first, last;        // positions [first, last) of the order
};

// chunks: whole waves of one class while the pointers (words_of(class) dwords per row and lane, a wave has the rows of
// its first lane) and the codes stay within the budgets
template <class ClassOf, class WordsOf>
std::vector<Chunk> lane_chunks(const std::vector<int32_t>& order, const int64_t* seq_off, ClassOf class_of,
                               WordsOf words_of, int64_t ptr_budget)
{
    auto len_of = [&](int32_t r) { return seq_off[r + 1] - seq_off[r]; };
    std::vector<Chunk> chunks;
    for (size_t i = 0; i < order.size();) {
        const int cls = class_of(order[i]);
        size_t j = i;
        int64_t ptr_bytes = 0, code_bytes = 0;
        while (j < order.size() && class_of(order[j]) == cls) {
            size_t w1 = j;
            int64_t cb = 0;
            while (w1 < order.size() && w1 < j + 64 && class_of(order[w1]) == cls)
                cb += round_up(len_of(order[w1++]), NRA_STRUCT_BLOCK);
            const int64_t pb = len_of(order[j]) * 64 * words_of(cls) * 4;
            if (j > i && (ptr_bytes + pb > ptr_budget || code_bytes + cb > kCodeBudget)) break;
            ptr_bytes += pb; code_bytes += cb;
            j = w1;
        }
        chunks.push_back(Chunk{cls, i, j});
        i = j;
    }
    return chunks;
}

// what a run brings back: of the `stride` result words a kernel writes per tract, the first words.size() go to
// words[q][tract]; byte plane q (a byte per tract base, laid out as the codes) goes to planes[q] at the tract's offset
struct LaneOut {
    int stride;
    std::vector<int32_t*> words;
    std::vector<uint8_t*> planes;
};

// One run of the tracts order[0 .. n): a code byte per base at 16-byte offsets, padded by one block (the kernels load
// whole blocks); `words` pointer dwords per (row, lane) of a wave of 64, 0 for a kernel that keeps none; NraStructRead.
// motif = table[tract].  launch(reads, codes, pointers, planes, results) starts the kernels on the null stream and
// returns a hipError_t; `kernel` names them in the error.
template <class Launch>
int run_lanes(const int32_t* order, size_t n, const char* seqs, const int64_t* seq_off, const int32_t* table, int words,
              const LaneOut& out, const char* kernel, Launch launch)
{
    std::vector<NraStructRead> rd(n);
    int64_t code_bytes = 0, ptr_words = 0;
    for (size_t w0 = 0; w0 < n; w0 += 64) {                      // waves: the first lane holds the longest tract
        const int64_t rows = seq_off[order[w0] + 1] - seq_off[order[w0]];
        for (size_t l = w0; l < std::min(n, w0 + 64); ++l) {
            const int32_t r = order[l];
            rd[l].tract = (uint64_t)code_bytes;
            rd[l].ptr = (uint64_t)ptr_words;
            rd[l].n = (int32_t)(seq_off[r + 1] - seq_off[r]);
            rd[l].motif = table[r];
            code_bytes += round_up(rd[l].n, NRA_STRUCT_BLOCK);
        }
        ptr_words += rows * 64 * words;
    }
    std::vector<uint8_t> codes((size_t)code_bytes + NRA_STRUCT_BLOCK, (uint8_t)kCodeOther);
    for (size_t l = 0; l < n; ++l) encode(codes.data() + rd[l].tract, seqs + seq_off[order[l]], rd[l].n);

    const size_t n_planes = out.planes.size();
    DevBuf<NraStructRead> d_rd;
    DevBuf<uint8_t> d_codes;
    DevBuf<uint32_t> d_ptr;
    DevBuf<int32_t> d_res;
    std::vector<DevBuf<uint8_t>> d_planes(n_planes);
    std::vector<uint8_t*> planes(n_planes);
    NRA_HIP_TRY(d_rd.alloc(n));
    NRA_HIP_TRY(d_codes.alloc(codes.size()));
    for (size_t q = 0; q < n_planes; ++q) {
        NRA_HIP_TRY(d_planes[q].alloc(codes.size()));
        planes[q] = d_planes[q].p;
    }
    if (words) NRA_HIP_TRY(d_ptr.alloc((size_t)ptr_words));
    NRA_HIP_TRY(d_res.alloc((size_t)out.stride * n));
    NRA_HIP_TRY(hipMemcpy(d_rd.p, rd.data(), n * sizeof(NraStructRead), hipMemcpyHostToDevice));
    NRA_HIP_TRY(hipMemcpy(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice));
    const int e = launch(d_rd.p, d_codes.p, d_ptr.p, planes.data(), d_res.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string(kernel) + ": " + hipGetErrorString((hipError_t)e));
    NRA_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> res((size_t)out.stride * n);
    NRA_HIP_TRY(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l)
        for (size_t q = 0; q < out.words.size(); ++q) out.words[q][order[l]] = res[(size_t)out.stride * l + q];
    for (size_t q = 0; q < n_planes; ++q) {
        std::vector<uint8_t>& bytes = codes;                      // the codes are no longer needed
        NRA_HIP_TRY(hipMemcpy(bytes.data(), planes[q], bytes.size(), hipMemcpyDeviceToHost));
        for (size_t l = 0; l < n; ++l)
            if (rd[l].n) std::memcpy(out.planes[q] + seq_off[order[l]], bytes.data() + rd[l].tract, (size_t)rd[l].n);
    }
    return NRA_OK;
}

}  // namespace nra_host

#endif  // NRA_LANE_HOST_H
