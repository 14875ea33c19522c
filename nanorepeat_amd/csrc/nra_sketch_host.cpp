// nra_sketch_host.cpp -- C ABI of the sketch pairs (nra_sketch_pairs): argument checks, the order of the sequences by
// group, the launches of k_sketch and k_sketch_pairs (nra_sketch.hip) with the pair list that grows once, and the sort
// of the pairs.  NRA_DEBUG in the environment traces the launches and the regrowth on stderr.
#include "nra_host_util.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

static_assert(NRA_SKETCH_MAX_N == NRA_SKETCH_MAX_LEN, "the public limit is the kernels' limit");
const size_t kPad = 64;                          // bytes after the copy: the kernel's last 16-byte load stays inside
// a launch of NRA_SKETCH_LAUNCH_TILES workgroups of 256 threads is 2^31 threads: at the group limit (33.5 M tiles, 2^33
// threads in one grid) one launch ran 31 744 of its tiles and reported no error
const int64_t kTilesPerLaunch = NRA_SKETCH_LAUNCH_TILES;

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct Device {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    DevBuf<uint8_t> seqs;
    DevBuf<int64_t> seq_base, sk_off, tile_first;
    DevBuf<int32_t> seq_len, sk_len, n_valid, order, grp_end;
    DevBuf<uint32_t> sketch;
    DevBuf<NraSketchPair> pairs;
    DevBuf<unsigned long long> count;
    ~Device()
    {
        for (hipEvent_t e : {ev0, ev1, ev2})
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <class T> hipError_t upload(DevBuf<T>& buf, const std::vector<T>& v, hipStream_t st)
{
    hipError_t e = buf.alloc(v.size());
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

}  // namespace

extern "C" {

int nra_sketch_pairs(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, const int32_t* group,
                     int32_t k, int32_t min_shared, int64_t* n_pairs, int32_t* pair_a, int32_t* pair_b,
                     int32_t* pair_shared, int32_t* sketch_size, nra_sketch_stats_t* stats)
{
    if (k < 11 || k > 15 || k % 2 == 0) return fail(NRA_E_ARG, "k must be odd and in 11..15");
    if (min_shared < 1) return fail(NRA_E_ARG, "min_shared must be at least 1");
    if (n_seqs < 0) return fail(NRA_E_ARG, "negative sequence count");
    if (!n_pairs) return fail(NRA_E_ARG, "n_pairs is NULL");
    if (*n_pairs < 0) return fail(NRA_E_ARG, "negative pair capacity");
    if (*n_pairs > 0 && (!pair_a || !pair_b || !pair_shared)) return fail(NRA_E_ARG, "NULL output array");
    nra_sketch_stats_t st{};
    std::vector<NraSketchPair> pairs;
    std::vector<int32_t> sk_len;
    try {
        std::vector<int32_t> order;               // the sequences with a group, by (group, index)
        std::vector<int32_t> grp_end;             // per position: one past the last position of its group
        std::vector<int64_t> tile_first;          // per position: its first tile; one more entry, the tile count
        if (n_seqs > 0) {
            if (!seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
            if (!group) return fail(NRA_E_ARG, "group is NULL");
            if (int rc = check_tract_offsets(n_seqs, seq_off, NRA_SKETCH_MAX_LEN, "sequence", "sequence")) return rc;
            if (seq_off[n_seqs] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
            for (int32_t s = 0; s < n_seqs; ++s)
                if (group[s] >= 0) order.push_back(s);
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return group[a] < group[b]; });
            grp_end.resize(order.size());
            tile_first.assign(order.size() + 1, 0);
            for (size_t g0 = 0; g0 < order.size();) {
                size_t g1 = g0 + 1;
                while (g1 < order.size() && group[order[g1]] == group[order[g0]]) ++g1;
                if (g1 - g0 > (size_t)NRA_SKETCH_MAX_GROUP)
                    return fail(NRA_E_RANGE, "group " + std::to_string(group[order[g0]]) + " has more than " +
                                                 std::to_string(NRA_SKETCH_MAX_GROUP) + " sequences");
                for (size_t s = g0; s < g1; ++s) {
                    grp_end[s] = (int32_t)g1;
                    tile_first[s + 1] =
                        tile_first[s] + (int64_t)((g1 - 1 - s + NRA_SKETCH_BLOCK - 1) / NRA_SKETCH_BLOCK);
                }
                st.n_compared += (int64_t)(g1 - g0) * (int64_t)(g1 - g0 - 1) / 2;
                g0 = g1;
            }
            st.n_tiles = tile_first.back();
        }
        if (int rc = use_device(device, n_seqs > 0)) return rc;
        if (n_seqs > 0) {
            const bool debug = getenv("NRA_DEBUG") != nullptr;
            const auto t_up = std::chrono::steady_clock::now();
            const int64_t b0 = seq_off[0], bytes = seq_off[n_seqs] - b0;
            std::vector<int64_t> seq_base(n_seqs), sk_off(n_seqs + 1, 0);
            std::vector<int32_t> seq_len(n_seqs);
            for (int32_t s = 0; s < n_seqs; ++s) {
                seq_base[s] = seq_off[s] - b0;
                seq_len[s] = (int32_t)(seq_off[s + 1] - seq_off[s]);
                sk_off[s + 1] = sk_off[s] + std::max<int32_t>(0, seq_len[s] - k + 1);   // room for every window
            }
            Device d;
            NRA_HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
            NRA_HIP_TRY(hipEventCreate(&d.ev0));
            NRA_HIP_TRY(hipEventCreate(&d.ev1));
            NRA_HIP_TRY(hipEventCreate(&d.ev2));
            NRA_HIP_TRY(d.count.alloc(1));
            NRA_HIP_TRY(d.seqs.alloc((size_t)bytes + kPad));
            if (bytes) NRA_HIP_TRY(hipMemcpyAsync(d.seqs.p, seqs + b0, (size_t)bytes, hipMemcpyHostToDevice, d.stream));
            NRA_HIP_TRY(hipMemsetAsync(d.seqs.p + bytes, 0, kPad, d.stream));
            NRA_HIP_TRY(upload(d.seq_base, seq_base, d.stream));
            NRA_HIP_TRY(upload(d.seq_len, seq_len, d.stream));
            NRA_HIP_TRY(upload(d.sk_off, sk_off, d.stream));
            NRA_HIP_TRY(upload(d.order, order, d.stream));
            NRA_HIP_TRY(upload(d.grp_end, grp_end, d.stream));
            NRA_HIP_TRY(upload(d.tile_first, tile_first, d.stream));
            NRA_HIP_TRY(d.sketch.alloc((size_t)sk_off[n_seqs]));
            NRA_HIP_TRY(d.sk_len.alloc((size_t)n_seqs));
            NRA_HIP_TRY(d.n_valid.alloc((size_t)n_seqs));
            NRA_HIP_TRY(hipStreamSynchronize(d.stream));
            st.upload_ms = ms_since(t_up);

            NRA_HIP_TRY(hipEventRecord(d.ev0, d.stream));
            int e = nra_launch_sketch(d.stream, n_seqs, d.seqs.p, d.seq_base.p, d.seq_len.p, k, d.sk_off.p, d.sketch.p,
                                      d.sk_len.p, d.n_valid.p);
            if (e != 0) return fail(NRA_E_DEVICE, std::string("k_sketch: ") + hipGetErrorString((hipError_t)e));
            NRA_HIP_TRY(hipEventRecord(d.ev1, d.stream));

            // the number of pairs does not depend on the order the workgroups arrive in: a list that proves too small
            // is grown to the number the kernel reported and the launches repeated once
            size_t cap = (size_t)test_bytes("NRA_TEST_SKETCH_PAIR_CAP", 0);
            if (!cap)
                cap = std::min<size_t>(std::max<size_t>(size_t(32) * order.size(), size_t(1) << 16), size_t(1) << 25);
            NRA_HIP_TRY(d.pairs.ensure(cap));
            unsigned long long got = 0;
            for (int attempt = 0;; ++attempt) {
                NRA_HIP_TRY(hipMemsetAsync(d.count.p, 0, sizeof(got), d.stream));
                if (attempt) NRA_HIP_TRY(hipEventRecord(d.ev1, d.stream));
                for (int64_t t0 = 0; t0 < st.n_tiles; t0 += kTilesPerLaunch) {
                    e = nra_launch_sketch_pairs(d.stream, t0, std::min(kTilesPerLaunch, st.n_tiles - t0),
                                                (int32_t)order.size(), d.tile_first.p, d.order.p, d.grp_end.p,
                                                d.sk_off.p, d.sketch.p, d.sk_len.p, min_shared, d.pairs.p,
                                                d.pairs.cap, d.count.p);
                    if (e != 0)
                        return fail(NRA_E_DEVICE, std::string("k_sketch_pairs: ") + hipGetErrorString((hipError_t)e));
                }
                NRA_HIP_TRY(hipEventRecord(d.ev2, d.stream));
                NRA_HIP_TRY(hipMemcpyAsync(&got, d.count.p, sizeof(got), hipMemcpyDeviceToHost, d.stream));
                NRA_HIP_TRY(hipStreamSynchronize(d.stream));
                float ms = 0.f;
                if (!attempt) {
                    NRA_HIP_TRY(hipEventElapsedTime(&ms, d.ev0, d.ev1));
                    st.sketch_ms = ms;
                }
                NRA_HIP_TRY(hipEventElapsedTime(&ms, d.ev1, d.ev2));
                st.pairs_ms += ms;
                if (debug)
                    fprintf(stderr, "nra_sketch_pairs: %d sequence(s), %lld tile(s), %llu pair(s)\n", (int)n_seqs,
                            (long long)st.n_tiles, got);
                if (got <= d.pairs.cap) break;
                if (attempt) return fail(NRA_E_DEVICE, "k_sketch_pairs: the pair count changed between two launches");
                if (debug) fprintf(stderr, "nra_sketch_pairs: pair list grows from %zu to %llu\n", d.pairs.cap, got);
                NRA_HIP_TRY(d.pairs.ensure((size_t)got));
            }
            st.kernel_ms = st.sketch_ms + st.pairs_ms;
            pairs.resize((size_t)got);
            if (got)
                NRA_HIP_TRY(hipMemcpy(pairs.data(), d.pairs.p, (size_t)got * sizeof(NraSketchPair),
                                      hipMemcpyDeviceToHost));
            std::vector<int32_t> n_valid(n_seqs);
            sk_len.resize(n_seqs);
            NRA_HIP_TRY(hipMemcpy(sk_len.data(), d.sk_len.p, (size_t)n_seqs * sizeof(int32_t), hipMemcpyDeviceToHost));
            NRA_HIP_TRY(hipMemcpy(n_valid.data(), d.n_valid.p, (size_t)n_seqs * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int32_t s = 0; s < n_seqs; ++s) {
                st.n_kmers += sk_len[s];
                st.n_windows += n_valid[s];
            }
            const auto t_sort = std::chrono::steady_clock::now();
            std::sort(pairs.begin(), pairs.end(), [](const NraSketchPair& x, const NraSketchPair& y) {
                return x.a != y.a ? x.a < y.a : x.b < y.b;
            });
            st.sort_ms = ms_since(t_sort);
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "sketch pairs: host allocation failed");
    }
    const int64_t cap = *n_pairs;
    *n_pairs = (int64_t)pairs.size();
    if (stats) *stats = st;
    if ((int64_t)pairs.size() > cap)
        return fail(NRA_E_RANGE, "more pairs (" + std::to_string(pairs.size()) + ") than the capacity (" +
                                     std::to_string(cap) + ")");
    if (sketch_size) std::copy(sk_len.begin(), sk_len.end(), sketch_size);
    for (size_t q = 0; q < pairs.size(); ++q) {
        pair_a[q] = pairs[q].a; pair_b[q] = pairs[q].b; pair_shared[q] = pairs[q].shared;
    }
    return NRA_OK;
}

}  // extern "C"
