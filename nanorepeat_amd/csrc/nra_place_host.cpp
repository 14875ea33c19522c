// nra_place_host.cpp -- C ABI of the placement (nra_place_*): the index build on the host, the launches of k_place_hits
// (nra_place.hip) over the chunks of the target, and the reduction of the kept target windows to votes per
// (query, contig, strand, diagonal bin).  The rule is DESIGN.md section 31.
#include "nra_host_util.h"

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const size_t kPad = 64;                           // bytes after a chunk's copy: the kernel's last 16-byte load stays inside
const int kPosBits = 11, kQueryShift = 12;        // a posting: query << 12 | position << 1 | forward bit
const int64_t kBinBias = 4096;                    // a diagonal is at least -NRA_PLACE_MAX_QUERY: bin - 1 + kBinBias >= 0

static_assert(NRA_PLACE_MAX_QUERY <= (1 << kPosBits) && NRA_PLACE_MAX_QUERIES <= (1 << (32 - kQueryShift)),
              "a posting fits 32 bits");
static_assert(NRA_PLACE_MAX_POS <= (1 << 30), "position << 1 | forward bit fits 32 bits");
static_assert(NRA_PLACE_MAX_QUERY < kBinBias && (int64_t)NRA_PLACE_MAX_POS + NRA_PLACE_MAX_QUERY + kBinBias < (int64_t(1) << 31),
              "a biased diagonal bin fits 31 bits");
static_assert(NRA_PLACE_OCC_CEILING <= 65535, "the ceiling is a legal max_target_occ");

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct nra_place {
    int device = 0;
    int k = 13;
    int log2_slots = 0;
    bool broken = false;               // a scan ran into NRA_PLACE_MAX_HITS
    bool occ_stale = false;            // scans since the counters were last copied back
    int64_t max_hits = NRA_PLACE_MAX_HITS;
    nra_place_stats_t st{};
    std::vector<int32_t> query_len;
    std::vector<uint64_t> table;       // the host's copy: number of postings and first posting of a slot
    std::vector<uint32_t> postings;
    std::vector<uint32_t> occ;         // the counters as of the last copy back
    std::vector<NraPlaceRecord> records;
    struct Cand { int32_t q, t, s, b, v; };
    std::vector<Cand> cands;           // the result of the last nra_place_candidates, and what it was asked
    bool cand_valid = false;
    int32_t cand_bin = 0, cand_occ = 0, cand_votes = 0;
    size_t cand_records = 0;
    uint64_t* d_table = nullptr;
    uint32_t* d_occ = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<uint8_t> seqs;              // these grow and are reused across scans
    DevBuf<NraPlaceRecord> list;
    DevBuf<unsigned long long> counters;   // [0] records of the launch, [1] valid windows of the handle

    ~nra_place()
    {
        if (d_table) (void)hipFree(d_table);
        if (d_occ) (void)hipFree(d_occ);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// key << 32 | posting for every valid, non-periodic window of query q; the periodic windows' keys to `periodic`
void query_postings(const char* s, int64_t n, int k, uint32_t q, std::vector<uint64_t>& pairs,
                    std::vector<uint32_t>& periodic)
{
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    uint32_t fwd = 0, rev = 0;
    int run = 0;
    for (int64_t e = 0; e < n; ++e) {
        const int c = kBase.of[(unsigned char)s[e]];
        if (c > 3) { run = 0; continue; }
        fwd = ((fwd << 2) | (uint32_t)c) & kmask;
        rev = (rev >> 2) | ((uint32_t)(3 - c) << (2 * (k - 1)));
        if (++run < k) continue;
        bool per = false;
        for (int p = 1; p <= 6 && !per; ++p)     // w[i] == w[i + p] for every i: the first k - p bases equal the last k - p
            per = (fwd >> (2 * p)) == (fwd & ((1u << (2 * (k - p))) - 1u));
        const uint32_t key = std::min(fwd, rev);
        if (per) { periodic.push_back(key); continue; }
        const uint32_t j = (uint32_t)(e - (k - 1));
        pairs.push_back((uint64_t)key << 32 | (uint64_t)(q << kQueryShift | j << 1 | (fwd < rev ? 1u : 0u)));
    }
}

int build_index(nra_place* h, int32_t n_queries, const char* seqs, const int64_t* seq_off, int max_occ)
{
    std::vector<uint64_t> pairs;
    std::vector<uint32_t> periodic;
    h->query_len.resize((size_t)n_queries);
    for (int32_t q = 0; q < n_queries; ++q) {
        const int64_t len = seq_off[q + 1] - seq_off[q];
        h->query_len[(size_t)q] = (int32_t)len;
        if (len >= h->k) query_postings(seqs + seq_off[q], len, h->k, (uint32_t)q, pairs, periodic);
    }
    std::sort(periodic.begin(), periodic.end());
    h->st.n_masked_periodic = (int64_t)(std::unique(periodic.begin(), periodic.end()) - periodic.begin());
    std::vector<uint32_t>().swap(periodic);
    std::sort(pairs.begin(), pairs.end());

    std::vector<uint64_t> slots;                   // key | count << 30 | first << 38, before hashing
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        const uint32_t key = (uint32_t)(pairs[i] >> 32);
        while (j < pairs.size() && (uint32_t)(pairs[j] >> 32) == key) ++j;
        if ((int64_t)(j - i) > max_occ) {
            ++h->st.n_masked_max_occ;
        } else {
            if (h->postings.size() + (j - i) >= (size_t(1) << NRA_SCREEN_START_BITS))
                return fail(NRA_E_RANGE, "placement index: more than 2^26 postings");
            slots.push_back((uint64_t)key | (uint64_t)(j - i) << NRA_SCREEN_KEY_BITS |
                            (uint64_t)h->postings.size() << (NRA_SCREEN_KEY_BITS + NRA_SCREEN_CNT_BITS));
            for (size_t p = i; p < j; ++p) h->postings.push_back((uint32_t)pairs[p]);
        }
        i = j;
    }
    std::vector<uint64_t>().swap(pairs);

    // open addressing at load factor <= 0.5
    int log2_slots = 10;
    while ((size_t(1) << log2_slots) < 2 * slots.size()) ++log2_slots;
    const size_t n_slots = size_t(1) << log2_slots;
    h->table.assign(n_slots, NRA_SCREEN_EMPTY);
    for (uint64_t v : slots) {
        const uint64_t key = v & ((1ull << NRA_SCREEN_KEY_BITS) - 1);
        uint64_t at = (key * NRA_SCREEN_HASH_MUL) >> (64 - log2_slots);
        while (h->table[at] != NRA_SCREEN_EMPTY) at = (at + 1) & (n_slots - 1);
        h->table[at] = v;
    }
    h->log2_slots = log2_slots;
    h->occ.assign(n_slots, 0);
    h->st.n_keys = (int64_t)slots.size();
    h->st.n_postings = (int64_t)h->postings.size();
    h->st.index_bytes = (int64_t)(n_slots * (8 + 4));
    h->st.tile_windows = NRA_PLACE_TILE;

    NRA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_table), n_slots * 8));
    NRA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_occ), n_slots * 4));
    NRA_HIP_TRY(h->counters.alloc(2));
    NRA_HIP_TRY(hipMemcpy(h->d_table, h->table.data(), n_slots * 8, hipMemcpyHostToDevice));
    NRA_HIP_TRY(hipMemset(h->d_occ, 0, n_slots * 4));
    NRA_HIP_TRY(hipMemset(h->counters.p, 0, 2 * sizeof(unsigned long long)));
    return NRA_OK;
}

// the counters and the valid-window count as the device has them now, and what follows from them alone
int fetch_counters(nra_place* h)
{
    if (!h->occ_stale) return NRA_OK;
    NRA_HIP_TRY(hipSetDevice(h->device));
    unsigned long long c[2] = {0, 0};
    NRA_HIP_TRY(hipMemcpy(h->occ.data(), h->d_occ, h->occ.size() * 4, hipMemcpyDeviceToHost));
    NRA_HIP_TRY(hipMemcpy(c, h->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    h->st.n_target_windows = (int64_t)c[1];
    int64_t kept = 0;
    for (size_t at = 0; at < h->table.size(); ++at)
        if (h->occ[at] != 0 && h->occ[at] <= NRA_PLACE_OCC_CEILING)
            kept += (int64_t)h->occ[at] * (int64_t)((h->table[at] >> NRA_SCREEN_KEY_BITS) & ((1u << NRA_SCREEN_CNT_BITS) - 1));
    h->st.n_hits_kept = kept;
    h->occ_stale = false;
    return NRA_OK;
}

int check_handle(const nra_place* h)
{
    if (!h) return fail(NRA_E_ARG, "placement handle is NULL");
    if (h->broken)
        return fail(NRA_E_STATE, "the placement handle ran over its kept hits in an earlier scan: create a new one");
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_place_create(int device, int32_t n_queries, const char* seqs, const int64_t* seq_off, int32_t k,
                     int32_t max_occ, nra_place_t** out)
{
    if (!out) return fail(NRA_E_ARG, "out is NULL");
    *out = nullptr;
    if (n_queries < 0) return fail(NRA_E_ARG, "negative query count");
    if (k < 11 || k > 15 || k % 2 == 0) return fail(NRA_E_ARG, "k must be odd, 11..15");
    if (max_occ < 1 || max_occ > 255) return fail(NRA_E_ARG, "max_occ must be in 1..255");
    if (n_queries > 0 && !seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
    if (n_queries > NRA_PLACE_MAX_QUERIES)
        return fail(NRA_E_RANGE, "more than " + std::to_string(NRA_PLACE_MAX_QUERIES) + " queries");
    if (n_queries > 0) {
        if (int rc = check_tract_offsets(n_queries, seq_off, NRA_PLACE_MAX_QUERY, "query", "query")) return rc;
        if (seq_off[n_queries] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device)) return rc;
    nra_place* h = new (std::nothrow) nra_place;
    if (!h) return fail(NRA_E_NOMEM, "placement handle");
    h->device = device;
    h->k = k;
    h->max_hits = test_bytes("NRA_TEST_PLACE_MAX_HITS", NRA_PLACE_MAX_HITS);
    int rc = NRA_OK;
    try {
        const auto t0 = std::chrono::steady_clock::now();
        rc = build_index(h, n_queries, seqs, seq_off, max_occ);
        h->st.build_ms = ms_since(t0);
    } catch (const std::bad_alloc&) {
        rc = fail(NRA_E_NOMEM, "placement index: host allocation failed");
    }
    if (rc == NRA_OK) {
        hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&h->ev0);
        if (e == hipSuccess) e = hipEventCreate(&h->ev1);
        if (e != hipSuccess) rc = fail(NRA_E_DEVICE, std::string("placement stream: ") + hipGetErrorString(e));
    }
    if (rc != NRA_OK) { delete h; return rc; }
    *out = h;
    return NRA_OK;
}

int nra_place_scan(nra_place_t* h, int32_t contig, int64_t pos0, const char* bases, int64_t n)
{
    if (int rc = check_handle(h)) return rc;
    if (contig < 0) return fail(NRA_E_ARG, "negative contig label");
    if (pos0 < 0 || n < 0) return fail(NRA_E_ARG, "negative chunk position or size");
    if (n > 0 && !bases) return fail(NRA_E_ARG, "bases is NULL");
    if (pos0 > NRA_PLACE_MAX_POS || n > NRA_PLACE_MAX_POS - pos0)
        return fail(NRA_E_RANGE, "a chunk ends beyond contig position 2^30");
    const int64_t n_win = n >= h->k ? n - h->k + 1 : 0;
    if (n_win > 0 && h->st.n_keys > 0) {
        NRA_HIP_TRY(hipSetDevice(h->device));
        try {
            // launches of at most NRA_PLACE_LAUNCH_WINDOWS windows, each with a list of one record per window
            for (int64_t w0 = 0; w0 < n_win; w0 += NRA_PLACE_LAUNCH_WINDOWS) {
                const int64_t wins = std::min<int64_t>(NRA_PLACE_LAUNCH_WINDOWS, n_win - w0);
                const size_t bytes = (size_t)(wins + h->k - 1);
                NRA_HIP_TRY(h->seqs.ensure(bytes + kPad));
                NRA_HIP_TRY(h->list.ensure((size_t)wins));
                const auto t0 = std::chrono::steady_clock::now();
                NRA_HIP_TRY(hipMemcpyAsync(h->seqs.p, bases + w0, bytes, hipMemcpyHostToDevice, h->stream));
                NRA_HIP_TRY(hipMemsetAsync(h->seqs.p + bytes, 0, kPad, h->stream));
                NRA_HIP_TRY(hipMemsetAsync(h->counters.p, 0, sizeof(unsigned long long), h->stream));
                NRA_HIP_TRY(hipStreamSynchronize(h->stream));
                h->st.upload_ms += ms_since(t0);
                NRA_HIP_TRY(hipEventRecord(h->ev0, h->stream));
                h->occ_stale = true;
                const int e = nra_launch_place_hits(h->stream, wins, h->seqs.p, h->k, h->d_table, h->log2_slots, h->d_occ,
                                                    NRA_PLACE_OCC_CEILING, contig, pos0 + w0, h->list.p, h->counters.p,
                                                    h->counters.p + 1);
                if (e != 0) {
                    h->broken = true;
                    return fail(NRA_E_DEVICE, std::string("k_place_hits: ") + hipGetErrorString((hipError_t)e));
                }
                NRA_HIP_TRY(hipEventRecord(h->ev1, h->stream));
                unsigned long long got = 0;
                NRA_HIP_TRY(hipMemcpyAsync(&got, h->counters.p, sizeof(got), hipMemcpyDeviceToHost, h->stream));
                NRA_HIP_TRY(hipStreamSynchronize(h->stream));
                float ms = 0.f;
                NRA_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
                h->st.kernel_ms += ms;
                if ((int64_t)(h->records.size() + got) > h->max_hits) {
                    h->broken = true;
                    return fail(NRA_E_RANGE, "the handle would keep more than " + std::to_string(h->max_hits) +
                                                 " target windows: lower max_occ, so that fewer repeated k-mers stay in "
                                                 "the index, or raise k");
                }
                const size_t at = h->records.size();
                h->records.resize(at + (size_t)got);
                if (got)
                    NRA_HIP_TRY(hipMemcpy(h->records.data() + at, h->list.p, (size_t)got * sizeof(NraPlaceRecord),
                                          hipMemcpyDeviceToHost));
            }
        } catch (const std::bad_alloc&) {
            h->broken = true;
            return fail(NRA_E_NOMEM, "placement scan: host allocation failed");
        }
    } else if (n_win > 0) {
        // an empty index: the valid windows are still counted, on the host
        int64_t valid = 0;
        int run = 0;
        for (int64_t e = 0; e < n; ++e) {
            run = kBase.of[(unsigned char)bases[e]] > 3 ? 0 : run + 1;
            valid += run >= h->k;
        }
        h->st.n_target_windows += valid;
    }
    h->st.target_bases += n;
    h->st.n_chunks += 1;
    return NRA_OK;
}

int nra_place_candidates(nra_place_t* h, int32_t bin, int32_t max_target_occ, int32_t min_votes, int64_t* n_cand,
                         int32_t* cand_query, int32_t* cand_contig, int32_t* cand_strand, int32_t* cand_bin,
                         int32_t* cand_votes)
{
    if (int rc = check_handle(h)) return rc;
    if (!n_cand) return fail(NRA_E_ARG, "n_cand is NULL");
    if (bin < 1 || bin > 4096) return fail(NRA_E_ARG, "bin must be in 1..4096");
    if (max_target_occ < 1 || max_target_occ > 65535) return fail(NRA_E_ARG, "max_target_occ must be in 1..65535");
    if (min_votes < 1) return fail(NRA_E_ARG, "min_votes must be >= 1");
    if (*n_cand < 0) return fail(NRA_E_ARG, "negative candidate capacity");
    if (*n_cand > 0 && (!cand_query || !cand_contig || !cand_strand || !cand_bin || !cand_votes))
        return fail(NRA_E_ARG, "NULL output array");
    if (max_target_occ > NRA_PLACE_OCC_CEILING)
        return fail(NRA_E_RANGE, "max_target_occ is above " + std::to_string(NRA_PLACE_OCC_CEILING) +
                                     ", the ceiling the handle keeps target windows up to");
    try {
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = fetch_counters(h)) return rc;
        int64_t over = 0;
        for (size_t at = 0; at < h->occ.size(); ++at) over += h->occ[at] > (uint32_t)max_target_occ;
        h->st.n_keys_over = over;

        // the candidates of these values on these records are kept: the call that follows a too small capacity is free
        const bool cached = h->cand_valid && h->cand_bin == bin && h->cand_occ == max_target_occ &&
                            h->cand_votes == min_votes && h->cand_records == h->records.size();
        std::vector<nra_place::Cand>& cands = h->cands;
        if (!cached) {
            h->cand_valid = false;
            cands.clear();
            // the counting hits, sorted by query with a counting sort, then by (contig, strand, diagonal bin) inside a
            // query: contig << 32 | strand << 31 | bin + kBinBias
            const int64_t k = h->k;
            const size_t nq = h->query_len.size();
            std::vector<uint64_t> first(nq + 1, 0), hit_key, keys;
            std::vector<uint32_t> hit_query;
            hit_key.reserve(h->records.size());
            hit_query.reserve(h->records.size());
            for (const NraPlaceRecord& r : h->records) {
                if (h->occ[r.slot] > (uint32_t)max_target_occ) continue;
                const uint64_t slot = h->table[r.slot];
                const uint32_t n = (uint32_t)(slot >> NRA_SCREEN_KEY_BITS) & ((1u << NRA_SCREEN_CNT_BITS) - 1);
                const uint32_t at = (uint32_t)(slot >> (NRA_SCREEN_KEY_BITS + NRA_SCREEN_CNT_BITS));
                const int64_t i = r.pos_fwd >> 1;
                const uint32_t g = r.pos_fwd & 1u;
                for (uint32_t p = 0; p < n; ++p) {
                    const uint32_t post = h->postings[at + p];
                    const uint32_t q = post >> kQueryShift;
                    const int64_t j = (post >> 1) & ((1u << kPosBits) - 1);
                    const uint64_t s = (post & 1u) == g ? 0 : 1;
                    const int64_t d = s == 0 ? i - j : i + j + k - h->query_len[q];
                    const int64_t b = d >= 0 ? d / bin : -((-d + bin - 1) / bin);
                    hit_query.push_back(q);
                    hit_key.push_back((uint64_t)(uint32_t)r.contig << 32 | s << 31 | (uint64_t)(b + kBinBias));
                    ++first[q + 1];
                }
            }
            for (size_t q = 0; q < nq; ++q) first[q + 1] += first[q];
            keys.resize(hit_key.size());
            {
                std::vector<uint64_t> cursor(first.begin(), first.end() - 1);
                for (size_t x = 0; x < hit_key.size(); ++x) keys[cursor[hit_query[x]]++] = hit_key[x];
            }
            std::vector<uint64_t>().swap(hit_key);
            std::vector<uint32_t>().swap(hit_query);

            // bins with hits, ascending within a (query, contig, strand): v(b) = c(b) + c(b + 1), so a bin with hits
            // makes the candidates b - 1 (unless the bin before it has hits and makes it) and b
            for (size_t q = 0; q < nq; ++q) {
                uint64_t* lo = keys.data() + first[q];
                uint64_t* hi = keys.data() + first[q + 1];
                std::sort(lo, hi);
                auto emit = [&](uint64_t key, int64_t b, int64_t v) {
                    if (v >= min_votes)
                        cands.push_back(nra_place::Cand{(int32_t)q, (int32_t)(key >> 32), (int32_t)(key >> 31 & 1),
                                                        (int32_t)b, (int32_t)v});
                };
                const uint64_t* prev = nullptr;
                for (uint64_t* x = lo; x < hi;) {
                    uint64_t* y = x;
                    while (y < hi && *y == *x) ++y;
                    const int64_t b = (int64_t)(*x & 0x7fffffffu) - kBinBias;
                    if (!(prev && *prev + 1 == *x)) emit(*x, b - 1, y - x);       // the same (contig, strand), bin b - 1
                    uint64_t* z = y;
                    if (y < hi && *y == *x + 1)
                        while (z < hi && *z == *y) ++z;
                    emit(*x, b, (y - x) + (z - y));
                    prev = x;
                    x = y;
                }
            }
            h->cand_valid = true;
            h->cand_bin = bin; h->cand_occ = max_target_occ; h->cand_votes = min_votes;
            h->cand_records = h->records.size();
            h->st.reduce_ms = ms_since(t0);
        }

        const int64_t cap = *n_cand;
        *n_cand = (int64_t)cands.size();
        if ((int64_t)cands.size() > cap)
            return fail(NRA_E_RANGE, "more candidates (" + std::to_string(cands.size()) + ") than the capacity (" +
                                         std::to_string(cap) + ")");
        for (size_t x = 0; x < cands.size(); ++x) {
            cand_query[x] = cands[x].q; cand_contig[x] = cands[x].t; cand_strand[x] = cands[x].s;
            cand_bin[x] = cands[x].b; cand_votes[x] = cands[x].v;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "placement candidates: host allocation failed");
    }
    return NRA_OK;
}

int nra_place_stats(nra_place_t* h, nra_place_stats_t* st)
{
    if (!h || !st) return fail(NRA_E_ARG, "NULL argument");
    if (!h->broken)
        if (int rc = fetch_counters(h)) return rc;
    *st = h->st;
    return NRA_OK;
}

int nra_place_destroy(nra_place_t* h)
{
    if (!h) return NRA_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return NRA_OK;
}

}  // extern "C"
