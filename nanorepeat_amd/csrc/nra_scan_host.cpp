// nra_scan_host.cpp -- C ABI of the repeat scan (nra_scan_repeats): argument checks, the table of every primitive
// p-mer, the chunks of reads, the launches of k_scan_repeats (nra_scan.hip) with the segment list that grows once, and
// the islands formed from the segments.  NRA_DEBUG in the environment traces every chunk and regrowth on stderr.
#include "nra_host_util.h"

#include <algorithm>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const int64_t kChunkBytes = int64_t(1) << 28;   // read bytes per launch (a longer read goes alone)
const size_t kPad = 64;                         // bytes after a chunk's copy: the kernel's last 16-byte load stays inside

struct Run {
    int32_t read, start, end, cls, windows, fwd;
};

// (class id + 1) << 1 | reverse for every primitive p-mer, p = 1..6, at NRA_MOTIF_TAB_OFF(p) + its code; 0 elsewhere
std::vector<uint16_t> build_table()
{
    std::vector<uint16_t> tab(NRA_MOTIF_TAB_ENTRIES, 0);
    for (int p = 1; p <= NRA_MOTIF_MAX_ROOT; ++p) {
        const uint32_t n = 1u << (2 * p), mask = n - 1u;
        auto rotate = [&](uint32_t w) { return ((w << 2) | (w >> (2 * (p - 1)))) & mask; };
        for (uint32_t w = 0; w < n; ++w) {
            uint32_t rc = 0;
            for (int i = 0; i < p; ++i) rc = rc << 2 | (3u - ((w >> (2 * i)) & 3u));
            uint32_t best = w, best_rc = rc, x = w, y = rc;
            bool primitive = true;
            for (int i = 1; i < p; ++i) {
                x = rotate(x);
                y = rotate(y);
                if (x == w) primitive = false;
                best = std::min(best, x);
                best_rc = std::min(best_rc, y);
            }
            if (!primitive) continue;
            const uint32_t canon = std::min(best, best_rc);
            tab[NRA_MOTIF_TAB_OFF(p) + w] = (uint16_t)((NRA_MOTIF_TAB_OFF(p) + canon + 1u) << 1 | (best != canon ? 1u : 0u));
        }
    }
    return tab;
}

struct Device {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<uint8_t> seqs;
    DevBuf<NraScanTile> tiles;
    DevBuf<NraScanSegment> segments;
    DevBuf<unsigned long long> count;
    DevBuf<uint32_t> tile_valid;
    DevBuf<uint16_t> tab;
    ~Device()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// reads [r0, r1) through the kernel -> their segments in `seg`
int scan_chunk(Device& d, int32_t r0, int32_t r1, const char* seqs, const int64_t* seq_off, int k, size_t first_cap,
               std::vector<NraScanSegment>& seg, nra_scan_stats_t& st)
{
    const bool debug = getenv("NRA_DEBUG") != nullptr;
    const int64_t b0 = seq_off[r0], bytes = seq_off[r1] - b0;
    std::vector<NraScanTile> tiles;
    for (int32_t r = r0; r < r1; ++r) {
        const int64_t len = seq_off[r + 1] - seq_off[r];
        const int64_t n_win = len >= k ? len - k + 1 : 0;
        for (int64_t w = 0; w < n_win; w += NRA_SCREEN_TILE)
            tiles.push_back(NraScanTile{seq_off[r] - b0 + w, r, (int32_t)std::min<int64_t>(NRA_SCREEN_TILE, n_win - w),
                                        (int32_t)w, 0});
    }
    seg.clear();
    if (debug)
        fprintf(stderr, "nra_scan_repeats: chunk of %d read(s), %lld base(s), %zu tile(s)\n", (int)(r1 - r0),
                (long long)bytes, tiles.size());
    st.n_chunks += 1;
    if (tiles.empty()) return NRA_OK;
    NRA_HIP_TRY(d.seqs.ensure((size_t)bytes + kPad));
    NRA_HIP_TRY(d.tiles.ensure(tiles.size()));
    NRA_HIP_TRY(d.tile_valid.ensure(tiles.size()));
    NRA_HIP_TRY(d.segments.ensure(first_cap ? first_cap : std::max<size_t>(tiles.size() * 16, size_t(1) << 16)));
    NRA_HIP_TRY(hipMemcpyAsync(d.seqs.p, seqs + b0, (size_t)bytes, hipMemcpyHostToDevice, d.stream));
    NRA_HIP_TRY(hipMemsetAsync(d.seqs.p + bytes, 0, kPad, d.stream));
    NRA_HIP_TRY(hipMemcpyAsync(d.tiles.p, tiles.data(), tiles.size() * sizeof(NraScanTile), hipMemcpyHostToDevice,
                                  d.stream));
    // the number of segments does not depend on the order the lanes arrive in: a list that proves too small is grown
    // to the number the kernel reported and the launch repeated once
    for (int attempt = 0;; ++attempt) {
        unsigned long long got = 0;
        NRA_HIP_TRY(hipMemsetAsync(d.count.p, 0, sizeof(got), d.stream));
        NRA_HIP_TRY(hipEventRecord(d.ev0, d.stream));
        const int e = nra_launch_scan_repeats(d.stream, (int64_t)tiles.size(), d.tiles.p, d.seqs.p, k, d.tab.p,
                                              d.segments.p, d.segments.cap, d.count.p, d.tile_valid.p);
        if (e != 0) return fail(NRA_E_DEVICE, std::string("k_scan_repeats: ") + hipGetErrorString((hipError_t)e));
        NRA_HIP_TRY(hipEventRecord(d.ev1, d.stream));
        NRA_HIP_TRY(hipMemcpyAsync(&got, d.count.p, sizeof(got), hipMemcpyDeviceToHost, d.stream));
        NRA_HIP_TRY(hipStreamSynchronize(d.stream));
        float ms = 0.f;
        NRA_HIP_TRY(hipEventElapsedTime(&ms, d.ev0, d.ev1));
        st.kernel_ms += ms;
        if (got <= d.segments.cap) {
            seg.resize((size_t)got);
            if (got)
                NRA_HIP_TRY(hipMemcpy(seg.data(), d.segments.p, (size_t)got * sizeof(NraScanSegment),
                                         hipMemcpyDeviceToHost));
            std::vector<uint32_t> valid(tiles.size());
            NRA_HIP_TRY(hipMemcpy(valid.data(), d.tile_valid.p, valid.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t v : valid) st.n_windows += v;
            st.n_segments += (int64_t)got;
            return NRA_OK;
        }
        if (attempt) return fail(NRA_E_DEVICE, "k_scan_repeats: the segment count changed between two launches");
        if (debug)
            fprintf(stderr, "nra_scan_repeats: segment list grows from %zu to %llu\n", d.segments.cap, got);
        NRA_HIP_TRY(d.segments.ensure((size_t)got));
    }
}

// the segments of a chunk -> its islands of at least min_span bases, appended to `runs` in the order of the result
void form_islands(std::vector<NraScanSegment>& seg, int k, int max_gap, int min_span, std::vector<Run>& runs,
                  nra_scan_stats_t& st)
{
    auto cls = [](const NraScanSegment& s) { return (s.entry >> 1) - 1; };
    std::sort(seg.begin(), seg.end(), [&](const NraScanSegment& a, const NraScanSegment& b) {
        if (a.read != b.read) return a.read < b.read;
        if (cls(a) != cls(b)) return cls(a) < cls(b);
        return a.start < b.start;
    });
    const size_t first = runs.size();
    for (size_t i = 0; i < seg.size();) {
        Run r{seg[i].read, seg[i].start, 0, cls(seg[i]), 0, 0};
        int32_t last = seg[i].start;               // the island's last window position so far
        for (; i < seg.size() && seg[i].read == r.read && cls(seg[i]) == r.cls &&
               (int64_t)seg[i].start - last <= max_gap; ++i) {
            last = seg[i].start + seg[i].len - 1;
            r.windows += seg[i].len;
            if (!(seg[i].entry & 1)) r.fwd += seg[i].len;
        }
        st.n_periodic += r.windows;
        r.end = last + k;
        if (r.end - r.start >= min_span) runs.push_back(r);
    }
    std::sort(runs.begin() + (std::ptrdiff_t)first, runs.end(), [](const Run& a, const Run& b) {
        if (a.read != b.read) return a.read < b.read;
        if (a.start != b.start) return a.start < b.start;
        if (a.end != b.end) return a.end < b.end;
        return a.cls < b.cls;
    });
}

}  // namespace

extern "C" {

int nra_scan_repeats(int device, int32_t n_reads, const char* seqs, const int64_t* seq_off, int32_t k, int32_t max_gap,
                     int32_t min_span, int64_t* n_runs, int32_t* run_read, int32_t* run_start, int32_t* run_end,
                     int32_t* run_class, int32_t* run_windows, int32_t* run_fwd_windows, nra_scan_stats_t* stats)
{
    if (k < 8 || k > 15) return fail(NRA_E_ARG, "k must be in 8..15");
    if (max_gap < 1 || max_gap > NRA_SCAN_MAX_GAP) return fail(NRA_E_ARG, "max_gap must be in 1..100000");
    if (min_span < k) return fail(NRA_E_ARG, "min_span must be at least k");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (!n_runs) return fail(NRA_E_ARG, "n_runs is NULL");
    if (*n_runs < 0) return fail(NRA_E_ARG, "negative run capacity");
    if (*n_runs > 0 && (!run_read || !run_start || !run_end || !run_class || !run_windows || !run_fwd_windows))
        return fail(NRA_E_ARG, "NULL output array");
    if (n_reads > 0) {
        if (!seq_off) return fail(NRA_E_ARG, "seq_off is NULL");
        if (int rc = check_tract_offsets(n_reads, seq_off, NRA_SCAN_MAX_N, "read", "read")) return rc;
        if (seq_off[n_reads] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
    }
    if (int rc = use_device(device, n_reads > 0)) return rc;
    nra_scan_stats_t st{};
    std::vector<Run> runs;
    try {
        if (n_reads > 0) {
            static const std::vector<uint16_t> table = build_table();
            Device d;
            NRA_HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
            NRA_HIP_TRY(hipEventCreate(&d.ev0));
            NRA_HIP_TRY(hipEventCreate(&d.ev1));
            NRA_HIP_TRY(d.count.alloc(1));
            NRA_HIP_TRY(d.tab.alloc(table.size()));
            NRA_HIP_TRY(hipMemcpy(d.tab.p, table.data(), table.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            const int64_t chunk_bytes = test_bytes("NRA_TEST_SCAN_CHUNK_BYTES", kChunkBytes);
            const size_t first_cap = (size_t)test_bytes("NRA_TEST_SCAN_SEG_CAP", 0);
            std::vector<NraScanSegment> seg;
            for (int32_t r0 = 0; r0 < n_reads;) {
                int32_t r1 = r0 + 1;
                while (r1 < n_reads && seq_off[r1 + 1] - seq_off[r0] <= chunk_bytes) ++r1;
                if (int rc = scan_chunk(d, r0, r1, seqs, seq_off, k, first_cap, seg, st)) return rc;
                form_islands(seg, k, max_gap, min_span, runs, st);
                r0 = r1;
            }
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "repeat scan: host allocation failed");
    }
    const int64_t cap = *n_runs;
    *n_runs = (int64_t)runs.size();
    if (stats) *stats = st;
    if ((int64_t)runs.size() > cap)
        return fail(NRA_E_RANGE, "more runs (" + std::to_string(runs.size()) + ") than the capacity (" +
                                     std::to_string(cap) + ")");
    for (size_t q = 0; q < runs.size(); ++q) {
        run_read[q] = runs[q].read; run_start[q] = runs[q].start; run_end[q] = runs[q].end;
        run_class[q] = runs[q].cls; run_windows[q] = runs[q].windows; run_fwd_windows[q] = runs[q].fwd;
    }
    return NRA_OK;
}

}  // extern "C"
