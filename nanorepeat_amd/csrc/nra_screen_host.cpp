// nra_screen_host.cpp -- C ABI of the anchor k-mer screen (nra_screen_*): the index build on the host, the chunked
// launches of k_screen_hits (nra_screen.hip) and the per-(read, region) reduction with the pass rule; the motif classes,
// the launches of k_screen_motifs (nra_screen_motifs.hip) on the same chunk copy and the four kinds of
// nra_screen_reads_partial.
#include "nra_host_util.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const int64_t kSegmentBytes = int64_t(1) << 28;   // read bytes per launch (a longer read goes alone)
const size_t kPad = 64;                           // bytes after a chunk's copy: the kernel's last 16-byte load stays inside

}  // namespace

struct nra_screen {
    int device = 0;
    int k = 15;
    int32_t n_regions = 0;
    int log2_slots = 0;
    std::vector<int64_t> set_size;     // |K(g, s)| at 2g + s
    std::vector<int32_t> empty_regions;
    nra_screen_stats_t st{};
    uint64_t* table = nullptr;
    uint32_t* postings = nullptr;
    uint16_t* class_tab = nullptr;     // nra_screen_set_motifs: NRA_MOTIF_TAB_ENTRIES entries on the device
    std::vector<int32_t> class_of;     // region -> class, or -1
    std::vector<std::vector<int32_t>> class_regions;   // class -> its regions, ascending
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<uint8_t> seqs;              // these four grow and are reused across calls
    DevBuf<NraScreenTile> tiles;
    DevBuf<NraScreenEntry> entries;
    DevBuf<unsigned long long> count;

    ~nra_screen()
    {
        if (table) (void)hipFree(table);
        if (postings) (void)hipFree(postings);
        if (class_tab) (void)hipFree(class_tab);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// the canonical k-mers of one anchor's valid windows: non-periodic ones to `keys`, periodic ones to `periodic`
void anchor_kmers(const char* s, int64_t n, int k, std::vector<uint32_t>& keys, std::vector<uint32_t>& periodic)
{
    const uint32_t kmask = (1u << (2 * k)) - 1u;
    uint32_t fwd = 0, rev = 0;
    int run = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int c = kBase.of[(unsigned char)s[j]];
        if (c > 3) { run = 0; continue; }
        fwd = ((fwd << 2) | (uint32_t)c) & kmask;
        rev = (rev >> 2) | ((uint32_t)(3 - c) << (2 * (k - 1)));
        if (++run < k) continue;
        bool per = false;
        for (int p = 1; p <= 6 && !per; ++p)     // w[i] == w[i + p] for every i: the first k - p bases equal the last k - p
            per = (fwd >> (2 * p)) == (fwd & ((1u << (2 * (k - p))) - 1u));
        (per ? periodic : keys).push_back(std::min(fwd, rev));
    }
}

int build_index(nra_screen* s, const char* anchors, const int64_t* anchor_off, int max_occ)
{
    const int64_t n_sets = 2 * (int64_t)s->n_regions;
    std::vector<uint64_t> pairs;                   // canonical k-mer << 32 | set, each (k-mer, set) once
    std::vector<uint32_t> keys, periodic;
    s->set_size.assign((size_t)n_sets, 0);
    for (int64_t g = 0; g < n_sets; ++g) {
        keys.clear();
        anchor_kmers(anchors + anchor_off[g], anchor_off[g + 1] - anchor_off[g], s->k, keys, periodic);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        s->set_size[(size_t)g] = (int64_t)keys.size();
        for (uint32_t key : keys) pairs.push_back((uint64_t)key << 32 | (uint64_t)g);
    }
    std::sort(periodic.begin(), periodic.end());
    s->st.n_masked_periodic = (int64_t)(std::unique(periodic.begin(), periodic.end()) - periodic.begin());
    std::sort(pairs.begin(), pairs.end());

    // one slot per k-mer in at most max_occ sets; the others leave every set they are in
    std::vector<uint64_t> slots;                   // key | count << 30 | first << 38, before hashing
    std::vector<uint32_t> post;
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        const uint32_t key = (uint32_t)(pairs[i] >> 32);
        while (j < pairs.size() && (uint32_t)(pairs[j] >> 32) == key) ++j;
        if ((int64_t)(j - i) > max_occ) {
            for (size_t q = i; q < j; ++q) --s->set_size[(size_t)(uint32_t)pairs[q]];
            ++s->st.n_masked_max_occ;
        } else {
            if (post.size() + (j - i) >= (size_t(1) << NRA_SCREEN_START_BITS))
                return fail(NRA_E_RANGE, "anchor index: more than 2^26 postings");
            slots.push_back((uint64_t)key | (uint64_t)(j - i) << NRA_SCREEN_KEY_BITS |
                            (uint64_t)post.size() << (NRA_SCREEN_KEY_BITS + NRA_SCREEN_CNT_BITS));
            for (size_t q = i; q < j; ++q) post.push_back((uint32_t)pairs[q]);
        }
        i = j;
    }
    std::vector<uint64_t>().swap(pairs);
    for (int32_t g = 0; g < s->n_regions; ++g)
        if (s->set_size[2 * (size_t)g] == 0 && s->set_size[2 * (size_t)g + 1] == 0) s->empty_regions.push_back(g);

    // open addressing at load factor <= 0.5
    int log2_slots = 10;
    while ((size_t(1) << log2_slots) < 2 * slots.size()) ++log2_slots;
    const size_t n_slots = size_t(1) << log2_slots;
    std::vector<uint64_t> table(n_slots, NRA_SCREEN_EMPTY);
    for (uint64_t v : slots) {
        const uint64_t key = v & ((1ull << NRA_SCREEN_KEY_BITS) - 1);
        uint64_t h = (key * NRA_SCREEN_HASH_MUL) >> (64 - log2_slots);
        while (table[h] != NRA_SCREEN_EMPTY) h = (h + 1) & (n_slots - 1);
        table[h] = v;
    }
    s->log2_slots = log2_slots;
    s->st.n_keys = (int64_t)slots.size();
    s->st.n_postings = (int64_t)post.size();
    s->st.n_empty_regions = (int64_t)s->empty_regions.size();
    s->st.index_bytes = (int64_t)(n_slots * 8 + post.size() * 4);

    NRA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->table), n_slots * 8));
    NRA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->postings), std::max<size_t>(post.size(), 1) * 4));
    NRA_HIP_TRY(hipMemcpy(s->table, table.data(), n_slots * 8, hipMemcpyHostToDevice));
    if (!post.empty()) NRA_HIP_TRY(hipMemcpy(s->postings, post.data(), post.size() * 4, hipMemcpyHostToDevice));
    return NRA_OK;
}

// one kernel over the uploaded tiles -> its entries appended to `out`.  Overflowing LDS maps can make more entries than
// the list holds: it is grown and the kernel run again (how many overflow depends on the order the lanes arrive in,
// hence the margin)
template <class Launch>
int run_kernel(nra_screen* s, const char* what, Launch launch, std::vector<NraScreenEntry>& out, double& kernel_ms)
{
    for (;;) {
        unsigned long long wanted = 0;
        NRA_HIP_TRY(hipMemsetAsync(s->count.p, 0, sizeof(unsigned long long), s->stream));
        NRA_HIP_TRY(hipEventRecord(s->ev0, s->stream));
        const int e = launch();
        if (e != 0) return fail(NRA_E_DEVICE, std::string(what) + ": " + hipGetErrorString((hipError_t)e));
        NRA_HIP_TRY(hipEventRecord(s->ev1, s->stream));
        NRA_HIP_TRY(hipMemcpyAsync(&wanted, s->count.p, sizeof(wanted), hipMemcpyDeviceToHost, s->stream));
        NRA_HIP_TRY(hipStreamSynchronize(s->stream));
        float ms = 0.f;
        NRA_HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        kernel_ms += ms;
        if (wanted <= s->entries.cap) {
            const size_t at = out.size();
            out.resize(at + (size_t)wanted);
            if (wanted)
                NRA_HIP_TRY(hipMemcpy(out.data() + at, s->entries.p, (size_t)wanted * sizeof(NraScreenEntry),
                                         hipMemcpyDeviceToHost));
            return NRA_OK;
        }
        NRA_HIP_TRY(s->entries.ensure((size_t)wanted * 2));
    }
}

// hits of reads [r0, r1) -> entries appended to `out`; with `classes`, their class windows -> entries appended to it,
// from the same upload
int screen_segment(nra_screen* s, int32_t r0, int32_t r1, const char* seqs, const int64_t* seq_off,
                   std::vector<NraScreenEntry>& out, double& kernel_ms, std::vector<NraScreenEntry>* classes = nullptr,
                   double* motif_ms = nullptr)
{
    const int64_t b0 = seq_off[r0], bytes = seq_off[r1] - b0;
    std::vector<NraScreenTile> tiles;
    for (int32_t r = r0; r < r1; ++r) {
        const int64_t len = seq_off[r + 1] - seq_off[r];
        const int64_t n_win = len >= s->k ? len - s->k + 1 : 0;
        for (int64_t w = 0; w < n_win; w += NRA_SCREEN_TILE)
            tiles.push_back(NraScreenTile{seq_off[r] - b0 + w, r, (int32_t)std::min<int64_t>(NRA_SCREEN_TILE, n_win - w)});
    }
    if (tiles.empty()) return NRA_OK;
    NRA_HIP_TRY(s->seqs.ensure((size_t)bytes + kPad));
    NRA_HIP_TRY(s->tiles.ensure(tiles.size()));
    NRA_HIP_TRY(s->count.ensure(1));
    NRA_HIP_TRY(s->entries.ensure(std::max<size_t>(tiles.size() * 16, size_t(1) << 16)));
    NRA_HIP_TRY(hipMemcpyAsync(s->seqs.p, seqs + b0, (size_t)bytes, hipMemcpyHostToDevice, s->stream));
    NRA_HIP_TRY(hipMemsetAsync(s->seqs.p + bytes, 0, kPad, s->stream));
    NRA_HIP_TRY(hipMemcpyAsync(s->tiles.p, tiles.data(), tiles.size() * sizeof(NraScreenTile), hipMemcpyHostToDevice,
                                  s->stream));
    int rc = run_kernel(s, "k_screen_hits", [&] {
        return nra_launch_screen_hits(s->stream, (int64_t)tiles.size(), s->tiles.p, s->seqs.p, s->k, s->table,
                                      s->log2_slots, s->postings, s->entries.p, s->entries.cap, s->count.p);
    }, out, kernel_ms);
    if (rc != NRA_OK || !classes) return rc;
    return run_kernel(s, "k_screen_motifs", [&] {
        return nra_launch_screen_motifs(s->stream, (int64_t)tiles.size(), s->tiles.p, s->seqs.p, s->k, s->class_tab,
                                        s->entries.p, s->entries.cap, s->count.p);
    }, *classes, *motif_ms);
}

int check_reads_args(const nra_screen* s, int32_t n_reads, int32_t min_hits, const int64_t* n_pairs)
{
    if (!s) return fail(NRA_E_ARG, "screen handle is NULL");
    if (!n_pairs) return fail(NRA_E_ARG, "n_pairs is NULL");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (min_hits < 1) return fail(NRA_E_ARG, "min_hits must be >= 1");
    if (*n_pairs < 0) return fail(NRA_E_ARG, "negative pair capacity");
    return NRA_OK;
}

int check_read_offsets(int32_t n_reads, const char* seqs, const int64_t* seq_off)
{
    if (n_reads > 0 && !seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
    if (n_reads > 0) {
        if (seq_off[0] < 0) return fail(NRA_E_ARG, "negative read offset");
        for (int32_t r = 0; r < n_reads; ++r)
            if (seq_off[r + 1] < seq_off[r]) return fail(NRA_E_ARG, "read offsets must not decrease");
        if (seq_off[n_reads] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    return NRA_OK;
}

bool by_read_then_set(const NraScreenEntry& a, const NraScreenEntry& b)
{
    return a.read != b.read ? a.read < b.read : a.set < b.set;
}

// the smallest rotation of a root or of its reverse complement: the name of its class
std::string class_name(const std::string& root)
{
    std::string rc(root.rbegin(), root.rend());
    for (char& c : rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    std::string best = root;
    for (const std::string& w : {root, rc})
        for (size_t i = 0; i < w.size(); ++i) best = std::min(best, w.substr(i) + w.substr(0, i));
    return best;
}

// every rotation of `root` -> class + 1 in the table
void fill_rotations(std::vector<uint16_t>& tab, const std::string& root, int32_t cls)
{
    const size_t p = root.size();
    for (size_t i = 0; i < p; ++i) {
        uint32_t code = 0;
        for (size_t j = 0; j < p; ++j) code = code << 2 | (uint32_t)kBase.of[(unsigned char)root[(i + j) % p]];
        tab[NRA_MOTIF_TAB_OFF(p) + code] = (uint16_t)(cls + 1);
    }
}

}  // namespace

extern "C" {

int nra_screen_create(int device, int32_t n_regions, const char* anchors, const int64_t* anchor_off, int32_t k,
                      int32_t max_occ, nra_screen_t** out)
{
    if (!out) return fail(NRA_E_ARG, "out is NULL");
    *out = nullptr;
    if (n_regions <= 0 || n_regions > (1 << 30)) return fail(NRA_E_ARG, "bad region count");
    if (!anchor_off) return fail(NRA_E_ARG, "anchor_off is NULL");
    if (k < 11 || k > 15 || k % 2 == 0) return fail(NRA_E_ARG, "k must be odd, 11..15");
    if (max_occ < 1 || max_occ > 255) return fail(NRA_E_ARG, "max_occ must be in 1..255");
    if (anchor_off[0] < 0) return fail(NRA_E_ARG, "negative anchor offset");
    for (int64_t i = 0; i < 2 * (int64_t)n_regions; ++i)
        if (anchor_off[i + 1] < anchor_off[i]) return fail(NRA_E_ARG, "anchor offsets must not decrease");
    if (anchor_off[2 * (int64_t)n_regions] > 0 && !anchors) return fail(NRA_E_ARG, "anchors is NULL");
    if (int rc = use_device(device)) return rc;
    nra_screen* s = new (std::nothrow) nra_screen;
    if (!s) return fail(NRA_E_NOMEM, "screen handle");
    s->device = device;
    s->k = k;
    s->n_regions = n_regions;
    int rc = NRA_OK;
    try {
        const auto t0 = std::chrono::steady_clock::now();
        rc = build_index(s, anchors, anchor_off, max_occ);
        s->st.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } catch (const std::bad_alloc&) {
        rc = fail(NRA_E_NOMEM, "anchor index: host allocation failed");
    }
    if (rc == NRA_OK) {
        hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&s->ev0);
        if (e == hipSuccess) e = hipEventCreate(&s->ev1);
        if (e != hipSuccess) rc = fail(NRA_E_DEVICE, std::string("screen stream: ") + hipGetErrorString(e));
    }
    if (rc != NRA_OK) { delete s; return rc; }
    *out = s;
    return NRA_OK;
}

int nra_screen_reads(nra_screen_t* s, int32_t n_reads, const char* seqs, const int64_t* seq_off, int32_t min_hits,
                     int64_t* n_pairs, int32_t* pair_read, int32_t* pair_region, int32_t* hits_left,
                     int32_t* hits_right)
{
    if (int rc = check_reads_args(s, n_reads, min_hits, n_pairs)) return rc;
    if (*n_pairs > 0 && (!pair_read || !pair_region || !hits_left || !hits_right))
        return fail(NRA_E_ARG, "NULL output array");
    if (int rc = check_read_offsets(n_reads, seqs, seq_off)) return rc;
    NRA_HIP_TRY(hipSetDevice(s->device));
    try {
        std::vector<NraScreenEntry> entries;
        double kernel_ms = 0.0;
        for (int32_t r0 = 0; r0 < n_reads;) {
            int32_t r1 = r0 + 1;
            while (r1 < n_reads && seq_off[r1 + 1] - seq_off[r0] <= kSegmentBytes) ++r1;
            const int rc = screen_segment(s, r0, r1, seqs, seq_off, entries, kernel_ms);
            if (rc != NRA_OK) return rc;
            r0 = r1;
        }
        // sum per (read, set), then per (read, region) with the pass rule; regions with two empty sets take every read
        std::sort(entries.begin(), entries.end(), by_read_then_set);
        struct Pair { int32_t read, region, left, right; };
        std::vector<Pair> pairs;
        const auto& empty = s->empty_regions;
        size_t i = 0;
        for (int32_t r = 0; r < n_reads; ++r) {
            size_t e = 0;
            auto flush_empty_below = [&](int32_t region) {
                for (; e < empty.size() && empty[e] < region; ++e) pairs.push_back(Pair{r, empty[e], 0, 0});
            };
            while (i < entries.size() && entries[i].read == r) {
                const int32_t g = entries[i].set >> 1;
                int64_t c[2] = {0, 0};
                for (; i < entries.size() && entries[i].read == r && (entries[i].set >> 1) == g; ++i)
                    c[entries[i].set & 1] += entries[i].count;
                const int64_t need_l = std::min<int64_t>(min_hits, s->set_size[2 * (size_t)g]);
                const int64_t need_r = std::min<int64_t>(min_hits, s->set_size[2 * (size_t)g + 1]);
                if (c[0] >= need_l && c[1] >= need_r) {
                    flush_empty_below(g);
                    pairs.push_back(Pair{r, g, (int32_t)c[0], (int32_t)c[1]});
                }
            }
            flush_empty_below(s->n_regions);
        }
        const int64_t cap = *n_pairs;
        *n_pairs = (int64_t)pairs.size();
        if ((int64_t)pairs.size() > cap)
            return fail(NRA_E_RANGE, "more passing pairs (" + std::to_string(pairs.size()) + ") than the capacity (" +
                                         std::to_string(cap) + ")");
        for (size_t q = 0; q < pairs.size(); ++q) {
            pair_read[q] = pairs[q].read; pair_region[q] = pairs[q].region;
            hits_left[q] = pairs[q].left; hits_right[q] = pairs[q].right;
        }
        s->st.bases_screened += n_reads > 0 ? seq_off[n_reads] - seq_off[0] : 0;
        s->st.kernel_ms = kernel_ms;
        s->st.sum_kernel_ms += kernel_ms;
        s->st.n_calls += 1;
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "screen: host allocation failed");
    }
    return NRA_OK;
}

int nra_screen_set_motifs(nra_screen_t* s, int32_t n_regions, const char* motifs, const int64_t* motif_off)
{
    if (!s) return fail(NRA_E_ARG, "screen handle is NULL");
    if (n_regions != s->n_regions) return fail(NRA_E_ARG, "the region count differs from the handle's");
    if (!motifs || !motif_off) return fail(NRA_E_ARG, "NULL argument");
    if (motif_off[0] < 0) return fail(NRA_E_ARG, "negative motif offset");
    for (int32_t g = 0; g < n_regions; ++g) {
        const int64_t len = motif_off[g + 1] - motif_off[g];
        if (len <= 0) return fail(NRA_E_ARG, "region " + std::to_string(g) + ": empty motif");
        for (int64_t i = 0; i < len; ++i)
            if (kBase.of[(unsigned char)motifs[motif_off[g] + i]] > 3)
                return fail(NRA_E_ARG, "region " + std::to_string(g) + ": motif byte other than ACGT");
        if (len > NRA_MOTIF_MAX_LEN) return fail(NRA_E_RANGE, "region " + std::to_string(g) + ": motif over 64 bases");
    }
    NRA_HIP_TRY(hipSetDevice(s->device));
    try {
        std::vector<uint16_t> tab(NRA_MOTIF_TAB_ENTRIES, 0);
        std::vector<int32_t> class_of((size_t)n_regions, -1);
        std::vector<std::vector<int32_t>> class_regions;
        std::map<std::string, int32_t> ids;
        for (int32_t g = 0; g < n_regions; ++g) {
            std::string m(motifs + motif_off[g], (size_t)(motif_off[g + 1] - motif_off[g]));
            for (char& c : m) c = "ACGT"[kBase.of[(unsigned char)c]];
            size_t p = 1;                          // the root: the shortest w with m = w^j
            for (; p < m.size(); ++p)
                if (m.size() % p == 0 && m.compare(p, m.size() - p, m, 0, m.size() - p) == 0) break;
            if (p > NRA_MOTIF_MAX_ROOT) continue;
            const std::string root = m.substr(0, p), name = class_name(root);
            auto it = ids.find(name);
            if (it == ids.end()) {
                it = ids.emplace(name, (int32_t)class_regions.size()).first;
                class_regions.emplace_back();
                std::string rc(root.rbegin(), root.rend());
                for (char& c : rc) c = "TGCA"[kBase.of[(unsigned char)c]];
                fill_rotations(tab, root, it->second);
                fill_rotations(tab, rc, it->second);
            }
            class_of[(size_t)g] = it->second;
            class_regions[(size_t)it->second].push_back(g);
        }
        if (!s->class_tab) NRA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s->class_tab), tab.size() * sizeof(uint16_t)));
        NRA_HIP_TRY(hipMemcpy(s->class_tab, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        s->class_of.swap(class_of);
        s->class_regions.swap(class_regions);
        s->st.n_classes = (int64_t)s->class_regions.size();
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "motif classes: host allocation failed");
    }
    return NRA_OK;
}

int nra_screen_reads_partial(nra_screen_t* s, int32_t n_reads, const char* seqs, const int64_t* seq_off,
                             int32_t min_hits, int32_t motif_share_pct, int64_t* n_pairs, int32_t* pair_read,
                             int32_t* pair_region, int32_t* hits_left, int32_t* hits_right, int32_t* motif_windows,
                             uint8_t* kind)
{
    if (int rc = check_reads_args(s, n_reads, min_hits, n_pairs)) return rc;
    if (motif_share_pct < 1 || motif_share_pct > 100) return fail(NRA_E_ARG, "motif_share_pct must be in 1..100");
    if (*n_pairs > 0 && (!pair_read || !pair_region || !hits_left || !hits_right || !motif_windows || !kind))
        return fail(NRA_E_ARG, "NULL output array");
    if (int rc = check_read_offsets(n_reads, seqs, seq_off)) return rc;
    NRA_HIP_TRY(hipSetDevice(s->device));
    try {
        const bool with_motifs = !s->class_regions.empty();
        std::vector<NraScreenEntry> entries, classes;
        double kernel_ms = 0.0, motif_ms = 0.0;
        for (int32_t r0 = 0; r0 < n_reads;) {
            int32_t r1 = r0 + 1;
            while (r1 < n_reads && seq_off[r1 + 1] - seq_off[r0] <= kSegmentBytes) ++r1;
            const int rc = screen_segment(s, r0, r1, seqs, seq_off, entries, kernel_ms, with_motifs ? &classes : nullptr,
                                          &motif_ms);
            if (rc != NRA_OK) return rc;
            r0 = r1;
        }
        std::sort(entries.begin(), entries.end(), by_read_then_set);
        std::sort(classes.begin(), classes.end(), by_read_then_set);

        struct Pair { int32_t read, region, left, right, windows; uint8_t kind; };
        std::vector<Pair> pairs;
        std::vector<Pair> mine;                    // one read's pairs, and its regions with hits that are none (kind 255)
        std::vector<int64_t> m(s->class_regions.size(), 0);
        std::vector<int32_t> seen;                 // the classes with windows in this read
        const auto& empty = s->empty_regions;
        size_t i = 0, ci = 0;
        for (int32_t r = 0; r < n_reads; ++r) {
            mine.clear();
            for (; ci < classes.size() && classes[ci].read == r; ++ci) {
                if (m[(size_t)classes[ci].set] == 0) seen.push_back(classes[ci].set);
                m[(size_t)classes[ci].set] += classes[ci].count;
            }
            const int64_t len = seq_off[r + 1] - seq_off[r];
            const int64_t n_win = len >= s->k ? len - s->k + 1 : 0;
            const int64_t need_m = std::max<int64_t>(min_hits, ((int64_t)motif_share_pct * n_win + 99) / 100);
            auto windows_of = [&](int32_t g) {
                const int32_t c = s->class_of.empty() ? -1 : s->class_of[(size_t)g];
                return c < 0 ? int64_t(0) : m[(size_t)c];
            };
            auto in_repeat = [&](int32_t g) {
                return n_win >= 1 && !s->class_of.empty() && s->class_of[(size_t)g] >= 0 && windows_of(g) >= need_m;
            };
            while (i < entries.size() && entries[i].read == r) {
                const int32_t g = entries[i].set >> 1;
                int64_t c[2] = {0, 0};
                for (; i < entries.size() && entries[i].read == r && (entries[i].set >> 1) == g; ++i)
                    c[entries[i].set & 1] += entries[i].count;
                const int64_t size_l = s->set_size[2 * (size_t)g], size_r = s->set_size[2 * (size_t)g + 1];
                const bool ok_l = c[0] >= std::min<int64_t>(min_hits, size_l);   // nra_screen_reads' rule: an empty set passes
                const bool ok_r = c[1] >= std::min<int64_t>(min_hits, size_r);
                uint8_t kd = 255;
                if (ok_l && ok_r) kd = 0;
                else if (ok_l && size_l > 0 && size_r > 0) kd = 1;
                else if (ok_r && size_r > 0 && size_l > 0) kd = 2;
                else if (in_repeat(g)) kd = 3;
                mine.push_back(Pair{r, g, (int32_t)c[0], (int32_t)c[1], (int32_t)windows_of(g), kd});
            }
            // regions without a hit: those with two empty sets (kind 0), and those of a class the read is made of
            const size_t n_hit = mine.size();
            auto has_hits = [&](int32_t g) {
                auto it = std::lower_bound(mine.begin(), mine.begin() + (std::ptrdiff_t)n_hit, g,
                                           [](const Pair& a, int32_t b) { return a.region < b; });
                return it != mine.begin() + (std::ptrdiff_t)n_hit && it->region == g;
            };
            for (int32_t g : empty) mine.push_back(Pair{r, g, 0, 0, (int32_t)windows_of(g), 0});
            for (int32_t c : seen) {
                if (n_win >= 1 && m[(size_t)c] >= need_m)
                    for (int32_t g : s->class_regions[(size_t)c]) {
                        const bool is_empty = s->set_size[2 * (size_t)g] == 0 && s->set_size[2 * (size_t)g + 1] == 0;
                        if (!is_empty && !has_hits(g)) mine.push_back(Pair{r, g, 0, 0, (int32_t)m[(size_t)c], 3});
                    }
            }
            std::sort(mine.begin(), mine.end(), [](const Pair& a, const Pair& b) { return a.region < b.region; });
            for (const Pair& p : mine)
                if (p.kind != 255) pairs.push_back(p);
            for (int32_t c : seen) m[(size_t)c] = 0;
            seen.clear();
        }
        const int64_t cap = *n_pairs;
        *n_pairs = (int64_t)pairs.size();
        if ((int64_t)pairs.size() > cap)
            return fail(NRA_E_RANGE, "more pairs (" + std::to_string(pairs.size()) + ") than the capacity (" +
                                         std::to_string(cap) + ")");
        for (size_t q = 0; q < pairs.size(); ++q) {
            pair_read[q] = pairs[q].read; pair_region[q] = pairs[q].region;
            hits_left[q] = pairs[q].left; hits_right[q] = pairs[q].right;
            motif_windows[q] = pairs[q].windows; kind[q] = pairs[q].kind;
        }
        s->st.bases_screened += n_reads > 0 ? seq_off[n_reads] - seq_off[0] : 0;
        s->st.kernel_ms = kernel_ms;
        s->st.sum_kernel_ms += kernel_ms;
        s->st.motif_kernel_ms = motif_ms;
        s->st.sum_motif_kernel_ms += motif_ms;
        s->st.n_calls += 1;
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "screen: host allocation failed");
    }
    return NRA_OK;
}

int nra_screen_stats(const nra_screen_t* s, nra_screen_stats_t* st)
{
    if (!s || !st) return fail(NRA_E_ARG, "NULL argument");
    *st = s->st;
    return NRA_OK;
}

int nra_screen_destroy(nra_screen_t* s)
{
    if (!s) return NRA_OK;
    (void)hipSetDevice(s->device);
    delete s;
    return NRA_OK;
}

}  // extern "C"
