// nra_host.cpp -- host side of the C ABI (include/nanorepeat_amd.h): encoding, 2-bit
// packing, task bucketing, kernel sequencing on a private HIP stream, HIP-event timing.
//
// Replaces, in the reference, the per-read `pymm2.main(...)` loop of round3_align
// (nanoRepeat_bam.py:452-500) + its selector (:408-450), and the per-grid-cell loop +
// selector of the joint rounds (nanoRepeat_joint.py:315-347, 397-421, 427-478).
// No CPU fallback exists: without a HIP device every compute entry point fails.
#include "nanorepeat_amd.h"
#include "nra_internal.h"
#include "nra_plan1d.h"
#include "nra_plan2d.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define NRA_VERSION_STR "nanorepeat_amd 0.1.0 (gfx950)"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? NRA_E_NOMEM : NRA_E_DEVICE,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

// NRA_DEBUG=1 in the environment: synchronise after every launch and trace it on stderr
static const bool g_debug = getenv("NRA_DEBUG") != nullptr;
// NRA_DEBUG_PHASES=1: the phase marks alone (no synchronisation: the times are the host's)
static const bool g_debug_phases = g_debug || getenv("NRA_DEBUG_PHASES") != nullptr;

#define LAUNCH_TRY(expr)                                                                         \
    do {                                                                                         \
        if (g_debug) fprintf(stderr, "[nra] launch %.60s ...\n", #expr);                         \
        int e_ = (expr);                                                                         \
        if (e_ != 0)                                                                             \
            return fail(NRA_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString((hipError_t)e_)); \
        if (g_debug) {                                                                           \
            hipError_t s_ = hipDeviceSynchronize();                                              \
            fprintf(stderr, "[nra]   done: %s\n", hipGetErrorString(s_));                        \
        }                                                                                        \
    } while (0)

// ASCII -> code table for the bulk encoder (same mapping as encode_base)
struct BaseCodeTable {
    uint8_t v[256];
    BaseCodeTable()
    {
        for (int i = 0; i < 256; ++i) v[i] = NRA_CODE_N;
        v['A'] = v['a'] = 0; v['C'] = v['c'] = 1; v['G'] = v['g'] = 2;
        v['T'] = v['t'] = v['U'] = v['u'] = 3;
    }
    uint8_t operator[](uint8_t c) const { return v[c]; }
};
static const BaseCodeTable kBaseCode;

// Device memory of one call or batch: hipMalloc costs ~0.3 ms per call, a batch has ~25 buffers, so
// they are carved out of a few large chunks.  While an Arena is "current" on this thread, DevBuf
// allocations come from it (and are released with it); otherwise a DevBuf owns its allocation.
// chunks come from / go back to a small per-device cache (HandlePool below)
hipError_t device_chunk_get(int device, size_t bytes, char** out, size_t* got);
void device_chunk_put(int device, char* p, size_t bytes);
// Copies between pageable host memory and the device (defined behind HandlePool): from kStagedFrom bytes on they go
// through a pinned buffer of the calling thread instead of straight into hipMemcpy.
hipError_t copy_h2d(void* dst, const void* src, size_t bytes);
hipError_t copy_d2h(void* dst, const void* src, size_t bytes);
// Between upload_batch_begin() and upload_batch_end() the calling thread's copy_h2d calls of any size only copy into the
// pinned stage and enqueue the transfer; _end waits for all of them once.  (A create call makes some sixteen uploads: as
// synchronous copies ~15 us each, a sixth of a small call's time.)  Nothing may use the destinations before _end.
void upload_batch_begin();
hipError_t upload_batch_end();
struct UploadBatchScope {            // ends the batch on every way out of a function; the normal path calls upload_batch_end() itself
    UploadBatchScope() { upload_batch_begin(); }
    ~UploadBatchScope() { (void)upload_batch_end(); }
};

struct Arena {
    struct Chunk { char* p; size_t size, used; };
    std::vector<Chunk> chunks;
    size_t next_chunk = 1 << 20;
    int device = 0;            // set before the first allocation; the work using the chunks is over when it dies
    ~Arena() { for (Chunk& c : chunks) device_chunk_put(device, c.p, c.size); }
    void expect(size_t bytes) { next_chunk = std::max(next_chunk, bytes); }
    void reset() { for (Chunk& c : chunks) c.used = 0; }        // keep the memory, hand it out again
    void release() { for (Chunk& c : chunks) device_chunk_put(device, c.p, c.size); chunks.clear(); }    // give it back
    size_t capacity() const { size_t n = 0; for (const Chunk& c : chunks) n += c.size; return n; }
    hipError_t alloc(size_t bytes, void** out)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        for (Chunk& c : chunks)
            if (c.size - c.used >= bytes) { *out = c.p + c.used; c.used += bytes; return hipSuccess; }
        Chunk c{nullptr, std::max(bytes, next_chunk), 0};
        hipError_t e = device_chunk_get(device, c.size, &c.p, &c.size);
        if (e != hipSuccess) return e;
        c.used = bytes;
        *out = c.p;
        chunks.push_back(c);
        return hipSuccess;
    }
};
thread_local Arena* g_arena = nullptr;
struct ArenaScope {
    Arena* prev;
    explicit ArenaScope(Arena* a) : prev(g_arena) { g_arena = a; }
    ~ArenaScope() { g_arena = prev; }
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    bool owned = false;
    ~DevBuf() { if (p && owned) (void)hipFree(p); }
    hipError_t alloc(size_t count)
    {
        n = count;
        if (count == 0) count = 1;
        if (g_arena) { owned = false; return g_arena->alloc(count * sizeof(T), (void**)&p); }
        owned = true;
        return hipMalloc((void**)&p, count * sizeof(T));      // (outside an arena: small, short-lived buffers only)
    }
    hipError_t upload(const std::vector<T>& v)
    {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return copy_h2d(p, v.data(), v.size() * sizeof(T));
    }
};

// Streams and events are expensive to create (~2 ms a stream) and a batch needs a handful: they
// are handed back to a per-device pool when a batch is destroyed and reused by the next one.
struct HandlePool {
    std::mutex mu;
    std::vector<std::vector<hipStream_t>> streams;      // [device]
    std::vector<std::vector<hipEvent_t>> timed, untimed;
    template <class V> static V& at(std::vector<V>& v, int device)
    {
        if ((int)v.size() <= device) v.resize((size_t)device + 1);
        return v[(size_t)device];
    }
    hipError_t stream(int device, hipStream_t* out)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = at(streams, device);
            if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
        }
        return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    }
    hipError_t event(int device, bool timing, hipEvent_t* out)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = at(timing ? timed : untimed, device);
            if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
        }
        return timing ? hipEventCreate(out) : hipEventCreateWithFlags(out, hipEventDisableTiming);
    }
    // device chunks of destroyed arenas (hipMalloc + hipFree cost ~0.5 ms per one-shot call): a few are kept,
    // per device at most kMaxCachedChunks / kMaxCachedBytes; when an allocation fails they are given back first
    std::vector<std::vector<std::pair<char*, size_t>>> chunks;      // [device]
    std::vector<size_t> cached_bytes;                                // [device]
    static constexpr size_t kMaxCachedBytes = (size_t)2 << 30;
    static constexpr size_t kMaxCachedChunks = 6;
    void chunks_trim(int device)        // give every cached chunk of the device back to the runtime
    {
        std::vector<std::pair<char*, size_t>> mine;
        {
            std::lock_guard<std::mutex> lk(mu);
            mine.swap(at(chunks, device));
            at(cached_bytes, device) = 0;
        }
        for (auto& c : mine) (void)hipFree(c.first);
    }
    hipError_t chunk_get(int device, size_t bytes, char** out, size_t* got)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = at(chunks, device);
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].second >= bytes && v[i].second <= 2 * bytes + ((size_t)16 << 20)) {
                    *out = v[i].first; *got = v[i].second;
                    at(cached_bytes, device) -= v[i].second;
                    v.erase(v.begin() + (long)i);
                    return hipSuccess;
                }
        }
        *got = bytes;
        hipError_t e = hipMalloc((void**)out, bytes);
        if (e == hipErrorOutOfMemory) {          // idle cached chunks may be what is missing: release them, try once more
            (void)hipGetLastError();
            chunks_trim(device);
            e = hipMalloc((void**)out, bytes);
        }
        return e;
    }
    void chunk_put(int device, char* p, size_t bytes)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = at(chunks, device);
            size_t& held = at(cached_bytes, device);
            if (v.size() < kMaxCachedChunks && held + bytes <= kMaxCachedBytes) {
                v.push_back({p, bytes});
                held += bytes;
                return;
            }
        }
        (void)hipFree(p);
    }
    // pinned staging buffers (hipHostMalloc costs ~0.2 ms): reused like the streams
    std::vector<std::pair<void*, size_t>> pinned;
    hipError_t pinned_get(size_t bytes, void** out, size_t* got)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < pinned.size(); ++i)
                if (pinned[i].second >= bytes && pinned[i].second <= 4 * bytes + (1u << 20)) {
                    *out = pinned[i].first; *got = pinned[i].second;
                    pinned.erase(pinned.begin() + (long)i);
                    return hipSuccess;
                }
        }
        *got = bytes;
        return hipHostMalloc(out, bytes, hipHostMallocDefault);
    }
    void pinned_trim()
    {
        std::vector<std::pair<void*, size_t>> mine;
        { std::lock_guard<std::mutex> lk(mu); mine.swap(pinned); }
        for (auto& c : mine) (void)hipHostFree(c.first);
    }
    void pinned_put(void* p, size_t bytes)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (pinned.size() < 8) pinned.push_back({p, bytes});
        else (void)hipHostFree(p);
    }
    void put_stream(int device, hipStream_t q)
    {
        std::lock_guard<std::mutex> lk(mu);
        at(streams, device).push_back(q);
    }
    void put_event(int device, bool timing, hipEvent_t e)
    {
        std::lock_guard<std::mutex> lk(mu);
        at(timing ? timed : untimed, device).push_back(e);
    }
};
HandlePool g_handles;

// (A batch runs every rows-per-lane bucket's kernels on streams of its own, the joint mode two batches at a time:
// with HIP's default of 4 hardware queues, copies and short kernels wait behind another stream's long sweeps.
// GPU_MAX_HW_QUEUES=8 helps -- config 3: 25.6 -> 19.2 ms per run -- but the environment belongs to the host
// process: the library does not touch it; see nanorepeat_amd.apply_recommended_env and INTEGRATION.md.)
hipError_t device_chunk_get(int device, size_t bytes, char** out, size_t* got) { return g_handles.chunk_get(device, bytes, out, got); }
void device_chunk_put(int device, char* p, size_t bytes) { g_handles.chunk_put(device, p, bytes); }

// hipMemcpy on pageable memory of 1 MB or more pins the caller's pages for the transfer and unpins them after it
// (the runtime's GPU_PINNED_MIN_XFER_SIZE).  With kernels of the same process running meanwhile that is not harmless on
// this platform: measured on the joint path with >= 29 000 reads (the first task array to reach 1 MB), the device drops
// into a state in which every running kernel takes 2-3 x as long (GPU busy 95 -> 55 %, 32 -> 60 ms per step, for
// seconds; 5 of 9 runs against 1 of 9 with the runtime's threshold lifted -- DESIGN.md 9(2b), profiles/r04_keep_cliff*).
// So the library never hands the runtime a large pageable buffer: it copies through a pinned stage of its own, in
// pieces, synchronously as before.
// (from 896 KB: below the runtime's 1 MB it stages the copy itself, faster than this file can -- config 3 at 5000 reads, whose
// task arrays are 300-400 KB: 6.15 ms per step, 6.55 with everything from 256 KB on going through the stage below)
constexpr size_t kStagedFrom = 896u << 10, kStageBytes = 4u << 20;
struct CopyStage {
    void* p = nullptr;
    size_t cap = 0;
    bool deferred = false;              // upload_batch_begin .. _end: transfers are enqueued, not waited for
    size_t used = 0;                    // ... bytes of the stage they hold
    ~CopyStage() { if (p) g_handles.pinned_put(p, cap); }
    hipError_t ensure() { return p ? hipSuccess : g_handles.pinned_get(kStageBytes, &p, &cap); }
};
thread_local CopyStage g_copy_stage;
// (The transfers go to the null stream: a stream of the stage's own would be one more for the runtime to map onto its
// GPU_MAX_HW_QUEUES hardware queues, and two of a batch's streams that end up sharing a queue run one behind the other --
// measured: config 3 6.15 -> 6.6 ms per step with a stream held by the stage.  The batches' streams are non-blocking, so
// the null stream orders nothing against them.)
void upload_batch_begin() { g_copy_stage.deferred = true; g_copy_stage.used = 0; }
hipError_t upload_batch_end()
{
    CopyStage& st = g_copy_stage;
    if (!st.deferred) return hipSuccess;
    st.deferred = false;
    st.used = 0;
    return st.p ? hipStreamSynchronize(nullptr) : hipSuccess;
}
hipError_t copy_h2d(void* dst, const void* src, size_t bytes)
{
    CopyStage& st = g_copy_stage;
    if (st.deferred) {
        if (bytes == 0) return hipSuccess;
        hipError_t e = st.ensure();
        if (e != hipSuccess) return e;
        for (size_t off = 0; off < bytes;) {
            if (st.cap - st.used < std::min<size_t>(bytes - off, 64u << 10)) {      // the stage is full: wait for what it holds
                if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return e;
                st.used = 0;
            }
            const size_t n = std::min(bytes - off, st.cap - st.used);
            memcpy((char*)st.p + st.used, (const char*)src + off, n);
            if ((e = hipMemcpyAsync((char*)dst + off, (char*)st.p + st.used, n, hipMemcpyHostToDevice, nullptr)) != hipSuccess) return e;
            st.used += (n + 255) & ~(size_t)255;
            off += n;
        }
        return hipSuccess;
    }
    if (bytes < kStagedFrom) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    hipError_t e = st.ensure();
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < bytes; off += st.cap) {
        const size_t n = std::min(st.cap, bytes - off);
        memcpy(st.p, (const char*)src + off, n);
        if ((e = hipMemcpy((char*)dst + off, st.p, n, hipMemcpyHostToDevice)) != hipSuccess) return e;      // (pinned source: no pinning by the runtime)
    }
    return hipSuccess;
}
hipError_t copy_d2h(void* dst, const void* src, size_t bytes)
{
    if (bytes < kStagedFrom) return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    CopyStage& st = g_copy_stage;
    hipError_t e = st.ensure();
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < bytes; off += st.cap) {
        const size_t n = std::min(st.cap, bytes - off);
        if ((e = hipMemcpy(st.p, (const char*)src + off, n, hipMemcpyDeviceToHost)) != hipSuccess) return e;
        memcpy((char*)dst + off, st.p, n);
    }
    return hipSuccess;
}

NraScoreParams to_params(const nra_scoring_t& sc)
{
    NraScoreParams p;
    p.match = sc.match; p.mismatch = sc.mismatch;
    p.open1 = sc.gap_open1 + sc.gap_ext1; p.ext1 = sc.gap_ext1;
    p.open2 = sc.gap_open2 + sc.gap_ext2; p.ext2 = sc.gap_ext2;
    p.ambi = sc.sc_ambi; p.min_score = sc.min_dp_score;
    return p;
}

bool scoring_ok(const nra_scoring_t* sc)
{
    if (!sc) return false;
    if (sc->match <= 0 || sc->match > 64 || sc->mismatch < 0 || sc->mismatch > 64) return false;
    if (sc->gap_ext1 <= 0 || sc->gap_ext2 <= 0 || sc->gap_open1 < 0 || sc->gap_open2 < 0) return false;
    if (sc->gap_open1 + sc->gap_ext1 > 1024 || sc->gap_open2 + sc->gap_ext2 > 1024) return false;
    if (sc->sc_ambi < 0 || sc->sc_ambi > 64) return false;
    return true;
}

// SIMDs of a device (4 per compute unit; 1024 on MI355X)
int device_simds(int device)
{
    static std::mutex mu;
    static std::vector<int> cache;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)cache.size() <= device) cache.resize((size_t)device + 1, 0);
    if (cache[(size_t)device] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        cache[(size_t)device] = 4 * cus;
    }
    return cache[(size_t)device];
}

// Every launch of the concurrent-block sweeps (k_sweep_ringmt) tags the granules it publishes with an epoch of its own:
// process-wide, never 0 (a zeroed strip carries none).
uint32_t next_epoch()
{
    static std::atomic<uint32_t> counter{0};
    uint32_t e = ++counter;
    if (e == 0) e = ++counter;
    return e;
}

}  // namespace

extern "C" int nra_copy_h2d(void* dst, const void* src, size_t bytes) { return (int)copy_h2d(dst, src, bytes); }
extern "C" int nra_copy_d2h(void* dst, const void* src, size_t bytes) { return (int)copy_d2h(dst, src, bytes); }

struct nra_batch {
    Arena arena;               // declared first: released after every DevBuf below
    Arena cell_arena;          // 2D: buffers that depend on the cell list; reset by nra_batch2d_set_cells
    Arena keep_arena;          // 2D: column states kept from one routed grid for the next
    // 2D: what nra_batch2d_set_cells needs from the reads part
    std::vector<NraDevRead> host_reads;
    Region2D jr;
    nra_scoring_t scoring{};
    size_t n_q2bit_words = 0;
    bool reads_have_n = false;
    // 2D: what is fixed when the reads are packed, what the batch carries from one cell list to the next, and what the
    // next run makes valid (nra_plan2d.h)
    Reads2D r2;
    Carried2D carried;
    Pending2D pending;
    DevBuf<int32_t> jlstate, jrstate;            // packed wave states at the end of L / of rev(R) outside the window
    DevBuf<NraJointPairTask> jlpk_tasks, jrpk_tasks;
    int kind = 0;              // 1 = 1D, 2 = 2D
    int device = 0;
    int flags = 0;
    int has_n = 0;
    hipStream_t stream = nullptr;
    NraScoreParams sp{};
    int n_reads = 0, n_regions = 0;
    int64_t n_cands = 0;       // 1D candidates or 2D cells
    std::vector<Bucket> buckets;

    DevBuf<uint8_t> pool;
    DevBuf<uint32_t> q2bit, qnmask;
    DevBuf<NraDevRegion> regions;
    DevBuf<NraDevRead> reads, reads_init;
    DevBuf<NraPairTask> pair_tasks;
    DevBuf<NraSweepTask> sweep_tasks;
    DevBuf<int32_t> snap;                      // R side of the junction: per sweep task 3 planes of R x 64 (both reads packed)
    DevBuf<int32_t> read_a1d;                  // A per read: best alignment inside R (origin-bit scheme)
    int relax_c = 0;                           // the taint scheme's margin (bases of an anchor next to the junction swept exactly); 0: off
    DevBuf<int32_t> redo;                      // ... per sweep task: a relaxed cell may have reached an output, swept again exactly
    std::vector<uint8_t> task_reads;           // ... per sweep task: its reads (nra_batch1d_resweeps)
    DevBuf<uint8_t> cand_flag;                 // flank verdict per candidate
    bool brute = false;                        // K independent alignments instead of the sweeps
    DevBuf<int32_t> chain_sweep;                // scratch strips of the chained row blocks (int32 sweep cells)
    DevBuf<int64_t> chain_payload;              // ... and of the chained payload kernels (int32 or int64 cells)
    DevBuf<NraJointTask> jbwd_tasks, jpre_tasks, jtail_tasks; // 2D decomposition: per read / per read / per (read, k1) run
    DevBuf<int32_t> jsnap, jread_a;             // R side of the junction (3 x int32 per base), A per read
    DevBuf<int32_t> jk1list, jstate;            // k1 values per read; wave states of the prefix sweeps
    // routed grids, junction at the end of mid: column states of the MID sweeps / the extended reverse sweeps,
    // B(k1) / A(k2), one combine task per read
    DevBuf<int32_t> jfs, jrs, jfb, jra;
    DevBuf<NraJointCombineTask> jcomb_tasks;
    bool joint_v2 = false;
    bool joint_chain = false;                   // ... with the MID part as column-parallel scans on column states (k_joint_midscan)
    std::vector<JointGroup> jgroups;
    bool all_strands_given = false;             // 2D: every read came with its strand, no probe needed
    int chain_cap = 0;
    int payload_strips = 0;                     // waves of a chained payload launch (strips in chain_payload)
    DevBuf<NraChainBlock> chain_blocks;         // k_sweep_ringmt: (task, row block) lists, launch group after launch group
    DevBuf<uint64_t> mt_strips;                 // ... the granule strips between consecutive blocks (zeroed at create)
    DevBuf<int32_t> mt_words;                   // ... [0], [1] unused (the give-up word is mt_giveup), [2 + bucket] that bucket's ticket
    // the sweeps in quanta (k_sweep_ringq): ticket order, the words of a run ([0] give-up word, [1 + bucket] that bucket's
    // ticket, then one arrival counter per task -- a view into run_words), the wave states at the cut
    DevBuf<uint32_t> q_list;
    DevBuf<int32_t> q_words, q_state;
    size_t q_words_n = 0, q_arrivals_off = 0;
    bool q_checked = true;
    DevBuf<NraTask> queue_tasks;
    DevBuf<int32_t> queue_count;   // per bucket: prebuilt queue length (constant)
    DevBuf<int32_t> tie_count;     // per bucket: tie queue length (device-written)
    // the saturation exit of the forward sweeps in quanta: per bucket four words of the run, [0] sweeps that
    // left, [2..3] the steps they skipped as one 64-bit word (8-byte aligned), read by nra_batch1d_saturation; sat_steps as
    // k_sweep_ringq takes it (< 0: no exit)
    DevBuf<int32_t> sat_count;
    int sat_steps = -1;
    // 1D: the small words a run starts from zero -- q_words, the row blocks' give-up word, tie_count, redo -- are views
    // into ONE allocation, cleared by one memset per run
    DevBuf<int32_t> run_words;
    int32_t* mt_giveup = nullptr;  // ... the launch-wide give-up word of the row blocks (k_sweep_ringmt)
    // 1D: the forward sweeps of this batch write cand_score and cand_flag of every candidate, so a run clears neither
    bool sweeps_write_all = false;
    int32_t* giveup_out = nullptr; // 1D: two trailing words of the result block: the run's give-up words (quanta, row blocks)
    bool results_staged = false;   // 1D: the pinned mirror holds the result block of the last run
    DevBuf<uint32_t> bucket_task_base;
    // 1D
    DevBuf<int32_t> kmin, kmax, read_bucket;
    DevBuf<uint32_t> coff;
    DevBuf<int32_t> cand_score, cand_tstart, cand_tend, best_score, n_ties;
    DevBuf<int64_t> sum_k, sum_k2;
    DevBuf<uint8_t> status;
    // the per-read results above are views into ONE block [sum_k | sum_k2 | best_score | n_ties | status(+strand)],
    // so that a fetch is one D2H copy into a pinned staging buffer instead of four or six pageable ones
    DevBuf<uint8_t> result_block;
    void* result_stage = nullptr;      // pinned host mirror (from the handle pool)
    size_t result_bytes = 0, result_stage_bytes = 0;
    // 2D
    DevBuf<int32_t> probe_score, probe_dummy, cell_k1, cell_k2;
    DevBuf<NraGridRow> grid_rows;               // a routed grid instead of cell_k1 / cell_k2 (grid_step1 > 0)
    int32_t grid_step1 = 0, grid_step2 = 0;
    DevBuf<NraTask> probe_tasks;                // chained 2D reads: (read, first cell) in both orientations
    DevBuf<int32_t> probe_count;
    DevBuf<uint32_t> cell_first, cell_cnt;
    DevBuf<int8_t> strand_in, strand_out;
    bool have_strand_in = false;
    bool keep_off = false;                      // set for one retry: this cell list keeps nothing (the kept states did not fit)
    int joint_keep = 0;                         // this cell list: 0 = nothing kept, 1 = sweeps that keep, 2 = no sweeps, kept states
    // 2D: flank sweeps enqueued ahead of the cell list (nra_batch2d_sweep_flanks): buffers of their own, alive as long as
    // the batch (the cell list's pool / reads / task arrays are rebuilt in place while these kernels run)
    DevBuf<uint8_t> warm_pool;
    DevBuf<NraDevRegion> warm_region;
    DevBuf<NraDevRead> warm_reads;
    DevBuf<NraJointPairTask> warm_tasks;
    std::vector<hipEvent_t> warm_ev;            // end of the ahead-of-time sweeps: [2 i] rev(R) side, [2 i + 1] L side of part i
    std::vector<int> warm_R;                    // rows per lane of part i
    int warm_has_n = 0;
    int64_t warm_cells = 0;                     // cells those sweeps execute (added to the statistics of the run they belong to)
    bool warm_built = false, warm_pending = false;   // pending: enqueued, the next run's streams have not waited for them yet
    // 2D: a refinement enqueued behind the run of a routed grid (nra_batch2d_refine): its routing happens on the device
    DevBuf<double> rf_bounds;                   // lo1 | hi1 | lo2 | hi2, n_reads each
    DevBuf<NraGridRow> rf_rows, rf_keep;        // the refinement's rows (device-written); the kept ranges
    DevBuf<uint32_t> rf_first, rf_cnt;          // cells of a read: at read * cap; how many (device-written)
    DevBuf<int64_t> rf_words;                   // [0] cells, [1] rows outside the kept ranges, [2] executed, [3] algorithmic cells
    DevBuf<int32_t> rf_rowspad;                 // 64 * rows per lane of a read's bucket (0: not swept)
    DevBuf<NraJointTask> rf_mid_tasks;
    DevBuf<NraJointCombineTask> rf_comb_tasks;
    DevBuf<int32_t> rf_fs, rf_fb;
    DevBuf<int32_t> rf_cell_score, rf_cell_wscore;   // the refinement's cells (the grid's own stay where they are: the grid may run again)
    int64_t rf_n_cands = 0;
    bool refined = false, refine_read = false;  // this run carries a refinement; its counters have been read back
    int64_t refine_bad_rows = 0;
    bool cells_need_clear = true;               // 2D: some cells are written by no kernel unless found

    std::vector<hipStream_t> bstreams;   // one per bucket: the sweep chains of different buckets overlap
    hipEvent_t mt_rev_ev = nullptr;      // end of the row blocks' reverse launches: buckets of quanta may wait for it (run_1d)
    std::vector<hipEvent_t> bdone;       // bucket chain finished
    hipEvent_t fork_ev = nullptr, fork2_ev = nullptr;
    hipEvent_t phase_ev[2] = {nullptr, nullptr};   // scoring phase start / end (timing)
    std::vector<hipEvent_t> ev;    // [0]=run start, [1]=run end, then pairs per dominant launch
    int n_score_ev = 0, n_ext_ev = 0;
    bool ran = false, accounted = false;
    bool have_cells = false;   // 2D: nra_batch2d_set_cells has run
    bool mt_checked = true;         // 1D: the give-up word of the concurrent-block sweeps has been read after this run
    bool flanks_enqueued = false;   // 2D: the strand-only kernels of this cell list are on their streams already
    int ev_next = 2;                // 2D: next free timing-event pair (the run is enqueued in two parts)
    nra_stats_t stats{};

    ~nra_batch()
    {
        // all work of the batch has to be over before its handles serve another batch
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipStream_t q : bstreams) if (q) (void)hipStreamSynchronize(q);
        for (hipEvent_t e : ev) if (e) g_handles.put_event(device, true, e);
        for (hipEvent_t e : phase_ev) if (e) g_handles.put_event(device, true, e);
        for (hipEvent_t e : bdone) if (e) g_handles.put_event(device, false, e);
        for (hipEvent_t e : warm_ev) if (e) g_handles.put_event(device, false, e);
        if (fork_ev) g_handles.put_event(device, false, fork_ev);
        if (mt_rev_ev) g_handles.put_event(device, false, mt_rev_ev);
        if (fork2_ev) g_handles.put_event(device, false, fork2_ev);
        for (hipStream_t q : bstreams) if (q) g_handles.put_stream(device, q);
        if (stream) g_handles.put_stream(device, stream);
        if (result_stage) g_handles.pinned_put(result_stage, result_stage_bytes);
    }
};

// The kernels' shared arguments from the batch's buffers as they are now.  Built at the top of a run function, never
// kept: the 2D batch reallocates pool and regions with every cell list.
static inline NraSeqArgs seq_args(const nra_batch* b)
{
    return NraSeqArgs{b->reads.p, b->regions.p, b->pool.p, b->q2bit.p, b->qnmask.p, b->sp};
}
static inline NraSweepArgs sweep_args(const nra_batch* b)
{
    return NraSweepArgs{seq_args(b), b->kmin.p, b->kmax.p, b->coff.p, b->snap.p, b->read_a1d.p, b->cand_score.p, b->cand_flag.p};
}

namespace {

// ---- host worker threads --------------------------------------------------------------
// Starting a thread costs ~50 us and a one-shot call has ~1 ms of packing to spread: the workers are
// started once and woken per job.  run(n, fn) runs fn(0..n-1) on the caller and n-1 workers and returns
// when all are done.  One job at a time (callers from several threads take turns).
class HostWorkers {
    std::mutex job_mu, mu;
    std::condition_variable wake, done;
    std::vector<std::thread> threads;
    const std::function<void(int)>* fn = nullptr;
    int n_jobs = 0, next = 0, pending = 0;
    uint64_t generation = 0;

    void loop()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            wake.wait(lk, [&] { return generation != seen; });
            seen = generation;
            while (next < n_jobs) {
                const int i = next++;
                lk.unlock();
                (*fn)(i);
                lk.lock();
                if (--pending == 0) done.notify_all();
            }
        }
    }

public:
    void run(int n, const std::function<void(int)>& f)
    {
        if (n <= 1) { if (n == 1) f(0); return; }
        std::lock_guard<std::mutex> one_job(job_mu);
        std::unique_lock<std::mutex> lk(mu);
        while ((int)threads.size() < n - 1) { threads.emplace_back([this] { loop(); }); threads.back().detach(); }
        fn = &f; n_jobs = n; next = 0; pending = n;
        ++generation;
        wake.notify_all();
        while (next < n_jobs) {            // the caller works too
            const int i = next++;
            lk.unlock();
            f(i);
            lk.lock();
            --pending;
        }
        done.wait(lk, [&] { return pending == 0; });
        fn = nullptr;
    }

    // The same job in two halves: start() hands the n pieces to the workers and returns, finish() -- same thread --
    // takes what is left of them and waits for the rest.  `f` has to stay alive in between.
    void start(int n, const std::function<void(int)>& f)
    {
        job_mu.lock();
        std::unique_lock<std::mutex> lk(mu);
        while ((int)threads.size() < n) { threads.emplace_back([this] { loop(); }); threads.back().detach(); }
        fn = &f; n_jobs = n; next = 0; pending = n;
        ++generation;
        wake.notify_all();
    }
    void finish()
    {
        std::unique_lock<std::mutex> lk(mu);
        while (next < n_jobs) {
            const int i = next++;
            lk.unlock();
            (*fn)(i);
            lk.lock();
            --pending;
        }
        done.wait(lk, [&] { return pending == 0; });
        fn = nullptr;
        lk.unlock();
        job_mu.unlock();
    }
};
// never destroyed: the workers wait on its condition variable for the life of the process, and destroying
// a condition variable that has waiters blocks (glibc) -- at exit that is a hang
HostWorkers& g_workers = *new HostWorkers;

// ---- sequence packing ---------------------------------------------------------------
struct PackedReads {
    std::vector<uint32_t> q2bit, nmask;
    std::vector<NraDevRead> reads;
    bool has_n = false;
};

// Layout of the packed reads (offsets, lengths, regions) and the zeroed word arrays; the words themselves are
// written by PackJob below.
int pack_layout(int32_t n_reads, const int64_t* seq_off, const int32_t* read_region,
                int32_t n_regions, PackedReads& out, int64_t max_len = NRA_MAX_QLEN_1BLOCK)
{
    out.reads.resize((size_t)n_reads);
    uint64_t base = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        int64_t len = seq_off[r + 1] - seq_off[r];
        if (len < 0) return fail(NRA_E_ARG, "seq_off must be non-decreasing");
        if (len > max_len)
            return fail(NRA_E_RANGE, "read " + std::to_string(r) + " has " + std::to_string(len) +
                                         " bases; this entry point holds at most " + std::to_string(max_len));
        int32_t g = read_region ? read_region[r] : 0;
        if (g < 0 || g >= n_regions) return fail(NRA_E_ARG, "read_region out of range");
        out.reads[r].qoff = (uint32_t)base;
        out.reads[r].qlen = (int32_t)len;
        out.reads[r].region = g;
        out.reads[r].rc = 0;
        base += ((uint64_t)len + 31) / 32 * 32;
        if (base > 0xfff00000ull) return fail(NRA_E_RANGE, "read pool exceeds 4G bases");
    }
    out.q2bit.assign((size_t)(base / 16) + 1, 0);
    out.nmask.assign((size_t)(base / 32) + 1, 0);
    return NRA_OK;
}

// The 2-bit packing itself, on the worker pool.  Every read starts on a 32-base boundary, so reads write disjoint
// words: one piece per ~256 k bases, each a contiguous run of reads.  The constructor starts the workers and
// returns -- the caller goes on with whatever needs the layout only (buckets, tasks) -- and join() (or the
// destructor, on an early return) takes the pieces that are left and waits; `has_n` is known after that.
class PackJob {
    PackedReads& out;
    const char* seqs;
    const int64_t* seq_off;
    int32_t n_reads;
    int nthreads = 1;
    std::vector<uint8_t> saw_n;
    std::function<void(int)> work;
    bool running = false;

public:
    PackJob(int32_t n_reads_, const char* seqs_, const int64_t* seq_off_, PackedReads& out_)
        : out(out_), seqs(seqs_), seq_off(seq_off_), n_reads(n_reads_)
    {
        const uint64_t base = (uint64_t)(out.q2bit.size() - 1) * 16;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        nthreads = (int)std::max<uint64_t>(1, std::min<uint64_t>(std::min<unsigned>(hw, 16), base >> 18));
        saw_n.assign((size_t)nthreads, 0);
        work = [this](int t) {
            uint32_t any_n = 0;
            const int32_t r0 = (int32_t)((int64_t)n_reads * t / nthreads), r1 = (int32_t)((int64_t)n_reads * (t + 1) / nthreads);
            for (int32_t r = r0; r < r1; ++r) {
                const uint8_t* s = reinterpret_cast<const uint8_t*>(seqs + seq_off[r]);
                const int32_t len = out.reads[r].qlen;
                uint32_t* q2 = out.q2bit.data() + (out.reads[r].qoff >> 4);
                uint32_t* nm = out.nmask.data() + (out.reads[r].qoff >> 5);
                for (int32_t i = 0; i < len; i += 32) {
                    const int32_t n = std::min(32, len - i);
                    uint64_t w = 0;                    // 32 bases x 2 bits; an N keeps code 0 and sets its mask bit
                    uint32_t mask = 0;
                    for (int32_t j = 0; j < n; ++j) {  // branch-free: code 4 (N) = 0b100 -> bits 0..1 = 0, bit 2 = the mask
                        const uint32_t c = kBaseCode[s[i + j]];
                        w |= (uint64_t)(c & 3u) << (2 * j);
                        mask |= (c >> 2) << j;
                    }
                    q2[(i >> 4)] = (uint32_t)w;
                    if (n > 16) q2[(i >> 4) + 1] = (uint32_t)(w >> 32);
                    nm[i >> 5] = mask;
                    any_n |= mask;
                }
            }
            saw_n[(size_t)t] = any_n ? 1 : 0;
        };
        if (nthreads > 1) { g_workers.start(nthreads, work); running = true; }
        else work(0);
    }
    void join()
    {
        if (running) { g_workers.finish(); running = false; }
        for (uint8_t v : saw_n) out.has_n |= v != 0;
    }
    ~PackJob() { if (running) g_workers.finish(); }
    PackJob(const PackJob&) = delete;
    PackJob& operator=(const PackJob&) = delete;
};

int pack_reads(int32_t n_reads, const char* seqs, const int64_t* seq_off, const int32_t* read_region,
               int32_t n_regions, PackedReads& out, int64_t max_len = NRA_MAX_QLEN_1BLOCK)
{
    const int rc = pack_layout(n_reads, seq_off, read_region, n_regions, out, max_len);
    if (rc) return rc;
    PackJob job(n_reads, seqs, seq_off, out);
    job.join();
    return NRA_OK;
}

int common_init(nra_batch* b, int device, const nra_scoring_t* sc, int flags)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    b->device = device;
    b->arena.device = device;
    b->cell_arena.device = device;
    b->keep_arena.device = device;
    b->flags = flags;
    b->sp = to_params(*sc);
    HIP_TRY(g_handles.stream(device, &b->stream));
    return NRA_OK;
}

// one device block (+ pinned host mirror) for the per-read results; n8 = int64 arrays, strand: 2D only
int alloc_results(nra_batch* b, size_t n, bool two_d)
{
    const size_t n8 = two_d ? 2 : 1;
    const size_t np = (n + 7) & ~(size_t)7;                 // keeps every sub-array 8-byte aligned
    b->result_bytes = np * (8 * n8 + 4 + 4 + 1 + (two_d ? 1 : 0)) + (two_d ? 0 : 8);
    HIP_TRY(b->result_block.alloc(b->result_bytes));
    HIP_TRY(g_handles.pinned_get(std::max<size_t>(b->result_bytes, 8), &b->result_stage, &b->result_stage_bytes));
    uint8_t* p = b->result_block.p;
    auto view = [&](auto& buf, size_t bytes) {
        buf.p = reinterpret_cast<decltype(buf.p)>(p); buf.n = n; buf.owned = false; p += bytes;
    };
    view(b->sum_k, np * 8);
    if (two_d) view(b->sum_k2, np * 8);
    view(b->best_score, np * 4);
    view(b->n_ties, np * 4);
    view(b->status, np);
    if (two_d) view(b->strand_out, np);
    else b->giveup_out = reinterpret_cast<int32_t*>(p);     // 1D: the run's give-up words, written by k_select_final_1d
    return NRA_OK;
}

// the results block -> the pinned mirror (one copy); returns host pointers through `at`
int fetch_results(nra_batch* b)
{
    if (b->result_bytes)
        HIP_TRY(hipMemcpy(b->result_stage, b->result_block.p, b->result_bytes, hipMemcpyDeviceToHost));
    return NRA_OK;
}
template <class T> const T* staged(const nra_batch* b, const DevBuf<T>& buf)
{
    return reinterpret_cast<const T*>(static_cast<const uint8_t*>(b->result_stage) +
                                      (reinterpret_cast<const uint8_t*>(buf.p) - b->result_block.p));
}

int make_events(nra_batch* b, int n)
{
    b->ev.assign((size_t)n, nullptr);
    for (int i = 0; i < n; ++i) HIP_TRY(g_handles.event(b->device, true, &b->ev[i]));
    for (int i = 0; i < 2; ++i) HIP_TRY(g_handles.event(b->device, true, &b->phase_ev[i]));
    return NRA_OK;
}

// ---- 1D: around the plan (nra_plan1d.h) -----------------------------------------------
int check_batch1d_args(const nra_region_t* regions, int32_t n_regions, int32_t n_reads, const char* seqs,
                       const int64_t* seq_off, const int32_t* read_region, const int32_t* kmin, const int32_t* kmax,
                       const nra_scoring_t* sc)
{
    if (!regions || n_regions <= 0 || n_reads < 0) return fail(NRA_E_ARG, "bad region / read count");
    if (n_reads > 0 && (!seqs || !seq_off || !kmin || !kmax)) return fail(NRA_E_ARG, "NULL input array");
    if (n_regions > 1 && n_reads > 0 && !read_region) return fail(NRA_E_ARG, "read_region required when n_regions > 1");
    if (!scoring_ok(sc)) return fail(NRA_E_ARG, "scoring parameters out of range");
    for (int32_t g = 0; g < n_regions; ++g) {
        const nra_region_t& rg = regions[g];
        if (rg.left_len < 0 || rg.right_len < 0 || rg.unit_len <= 0 || !rg.unit ||
            (rg.left_len > 0 && !rg.left) || (rg.right_len > 0 && !rg.right))
            return fail(NRA_E_ARG, "bad region " + std::to_string(g));
    }
    return NRA_OK;
}

// the environment knobs of a 1D plan, as they stand at this call (the plan itself reads no environment)
Plan1DKnobs plan1d_knobs()
{
    Plan1DKnobs k;
    auto knob = [](const char* name, bool& has, int& value) {
        if (const char* e = getenv(name)) { has = true; value = atoi(e); }
    };
    knob("NRA_RELAX_C", k.has_relax_c, k.relax_c);
    knob("NRA_CHAIN_FROM", k.has_chain_from, k.chain_from);
    knob("NRA_TEST_QSTEPS", k.has_qsteps, k.qsteps);
    knob("NRA_TEST_SAT", k.has_sat, k.sat);
    knob("NRA_TEST_SAT_STEPS", k.has_sat_steps, k.sat_steps);
    return k;
}

// The device side of a 1D plan: the batch's buffers out of one arena chunk and their uploads, enqueued and waited for
// once.  The order of the allocations is part of the contract: device addresses and the one-chunk sizing follow it.
int upload_plan_1d(nra_batch* b, const Plan1D& plan, const PackedReads& pr, const int32_t* kmin, const int32_t* kmax)
{
    const int32_t n_reads = b->n_reads;
    const int64_t total = plan.n_cands;
    const bool brute = plan.brute, all_ext = (b->flags & NRA_F_ALL_EXTENTS) != 0;
    const size_t nb = b->buckets.size();
    // one chunk for everything: ~7 B per read base, ~40 B per candidate, the tasks, the chain strips
    b->arena.expect(pr.q2bit.size() * 16 * 2 + (size_t)plan.snap_total * 4 + (size_t)total * 40 + plan.pool.size() + plan.sweep_tasks.size() * sizeof(NraSweepTask) +
                    plan.pair_tasks.size() * sizeof(NraPairTask) + (size_t)n_reads * 64 + (4u << 20));
    // (the chain strips get chunks of their own: they can be GBs)
    UploadBatchScope uploads;            // every upload below is enqueued; one wait behind the last of them
    HIP_TRY(b->pool.upload(plan.pool));
    HIP_TRY(b->q2bit.upload(pr.q2bit));
    HIP_TRY(b->qnmask.upload(pr.nmask));
    HIP_TRY(b->regions.upload(plan.dregs));
    HIP_TRY(b->reads.upload(pr.reads));
    HIP_TRY(b->pair_tasks.upload(plan.pair_tasks));
    HIP_TRY(b->sweep_tasks.upload(plan.sweep_tasks));
    if (!brute) {
        HIP_TRY(b->snap.alloc((size_t)plan.snap_total));
        HIP_TRY(b->read_a1d.alloc((size_t)n_reads));
        bool any_taint = false;
        for (const Bucket& bk : b->buckets) any_taint = any_taint || bk.taint;
        if (any_taint) b->redo.n = std::max<size_t>(plan.sweep_tasks.size(), 1);        // (a view into run_words, below)
        if (!plan.qlist.empty()) {
            HIP_TRY(b->q_list.upload(plan.qlist));
            b->q_arrivals_off = (1 + b->buckets.size() + 3) / 4 * 4;
            b->q_words_n = b->q_arrivals_off + plan.q_tasks;            // (a view into run_words, below)
            HIP_TRY(b->q_state.alloc(plan.q_state));
        }
    }
    HIP_TRY(b->cand_flag.alloc((size_t)total));
    if (!plan.chain_blocks.empty()) {
        HIP_TRY(b->chain_blocks.upload(plan.chain_blocks));
        const size_t granules = std::max<size_t>(plan.mt_strip_total, 1) * 5 * (size_t)b->chain_cap;
        HIP_TRY(b->mt_strips.alloc(granules));
        // (on the batch's own stream: the bucket streams are ordered behind it by fork_ev; a null-stream memset is not
        // ordered with these non-blocking streams at all)
        HIP_TRY(hipMemsetAsync(b->mt_strips.p, 0, granules * 8, b->stream));       // no granule carries an epoch yet (epochs are never 0)
        HIP_TRY(b->mt_words.alloc(2 + b->buckets.size()));
        HIP_TRY(hipMemsetAsync(b->mt_words.p, 0, (2 + b->buckets.size()) * 4, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    if (plan.strip_total || !plan.chain_blocks.empty()) {
        if (plan.strip_total) HIP_TRY(b->chain_sweep.alloc(plan.strip_total));
        // the chained buckets' extents launches run in turn and share these strips (int64 cells)
        b->payload_strips = chain_strips(plan.chain_queue_cap, NRA_CHAIN_STRIPS, (size_t)6 * 8 * (size_t)b->chain_cap);
        HIP_TRY(b->chain_payload.alloc((size_t)b->payload_strips * 6 * (size_t)b->chain_cap));
    }
    if (all_ext) HIP_TRY(b->queue_tasks.upload(plan.queue_tasks));
    else HIP_TRY(b->queue_tasks.alloc(plan.queue_total));
    HIP_TRY(b->queue_count.upload(plan.queue_count));
    {
        // the words of a run: [q_words | the row blocks' give-up word | tie_count | sat_count | redo], zero before any run too
        // (so that nra_batch1d_resweeps and nra_batch1d_saturation read nothing of a run that has not happened)
        const size_t n_redo = b->redo.n, n_words = b->q_words_n + 1 + 5 * std::max<size_t>(nb, 1) + 1 + n_redo;
        HIP_TRY(b->run_words.alloc(n_words));
        int32_t* w = b->run_words.p;
        auto view = [&](DevBuf<int32_t>& buf, size_t n) { buf.p = w; buf.n = n; buf.owned = false; w += n; };
        view(b->q_words, b->q_words_n);
        b->mt_giveup = w++;
        view(b->tie_count, std::max<size_t>(nb, 1));
        if (reinterpret_cast<uintptr_t>(w) & 7) ++w;                     // (the 64-bit step counts of sat_count: 8-byte aligned)
        view(b->sat_count, 4 * std::max<size_t>(nb, 1));
        view(b->redo, n_redo);
        HIP_TRY(hipMemsetAsync(b->run_words.p, 0, n_words * 4, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    HIP_TRY(b->bucket_task_base.upload(plan.task_base));
    {
        std::vector<int32_t> v(kmin, kmin + n_reads); HIP_TRY(b->kmin.upload(v));
        std::vector<int32_t> w(kmax, kmax + n_reads); HIP_TRY(b->kmax.upload(w));
    }
    HIP_TRY(b->read_bucket.upload(plan.read_bucket));
    HIP_TRY(b->coff.upload(plan.coff));
    HIP_TRY(b->cand_score.alloc((size_t)total));
    HIP_TRY(b->cand_tstart.alloc((size_t)total));
    HIP_TRY(b->cand_tend.alloc((size_t)total));
    const int rc = alloc_results(b, (size_t)n_reads, false);
    if (rc) return rc;
    HIP_TRY(upload_batch_end());
    return NRA_OK;
}

}  // namespace

// =====================================================================================
extern "C" {

int nra_set_error(int code, const char* msg) { return fail(code, msg ? msg : ""); }

int nra_abi_version(void) { return NRA_ABI_VERSION; }
const char* nra_version(void) { return NRA_VERSION_STR; }
const char* nra_last_error(void) { return g_err.c_str(); }

int nra_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_err = hipGetErrorString(e); return NRA_E_DEVICE; }
    return n;
}

int nra_release_cached_memory(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NRA_E_DEVICE, "no HIP device");
    if (device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (int d = device < 0 ? 0 : device; d < (device < 0 ? ndev : device + 1); ++d) {
        (void)hipSetDevice(d);
        g_handles.chunks_trim(d);
    }
    g_handles.pinned_trim();
    (void)hipSetDevice(prev);
    return NRA_OK;
}

void nra_default_scoring(nra_scoring_t* sc)
{
    if (!sc) return;
    sc->match = 2; sc->mismatch = 4;
    sc->gap_open1 = 4; sc->gap_ext1 = 2;
    sc->gap_open2 = 24; sc->gap_ext2 = 1;
    sc->sc_ambi = 1; sc->min_dp_score = 80;
}

// ---- 1D -----------------------------------------------------------------------------
int nra_batch1d_create(int device, const nra_region_t* regions, int32_t n_regions,
                       int32_t n_reads, const char* seqs, const int64_t* seq_off,
                       const int32_t* read_region, const int32_t* kmin, const int32_t* kmax,
                       const nra_scoring_t* sc, int32_t flags, nra_batch_t** out)
{
    if (!out) return fail(NRA_E_ARG, "out is NULL");
    *out = nullptr;
    int rc = check_batch1d_args(regions, n_regions, n_reads, seqs, seq_off, read_region, kmin, kmax, sc);
    if (rc) return rc;

    nra_batch* b = new nra_batch();
    std::unique_ptr<nra_batch> guard(b);
    ArenaScope arena_scope(&b->arena);
    b->kind = 1; b->n_reads = n_reads; b->n_regions = n_regions;
    rc = common_init(b, device, sc, flags);
    if (rc) return rc;

    PhaseClock clk(g_debug_phases);
    clk.mark("device, stream");
    // the workers pack the reads while this thread builds templates, buckets and tasks from the layout
    PackedReads pr;
    rc = pack_layout(n_reads, seq_off, read_region, n_regions, pr, NRA_MAX_QLEN);
    if (rc) return rc;
    PackJob packing(n_reads, seqs, seq_off, pr);
    clk.mark("read layout, packing started");

    // (the plan reads the layout alone -- pr.reads -- not the words the workers are writing)
    Plan1D plan;
    rc = plan_1d(regions, n_regions, pr.reads, kmin, kmax, sc, flags, plan1d_knobs(), device_simds(device), clk, plan);
    if (rc) return rc;
    packing.join();
    b->has_n = (plan.has_n || pr.has_n) ? 1 : 0;
    clk.mark("2-bit packing (rest)");

    b->n_cands = plan.n_cands;
    b->brute = plan.brute;
    b->relax_c = plan.relax_c;
    b->chain_cap = plan.chain_cap;
    b->sat_steps = plan.sat_steps;
    b->sweeps_write_all = plan.sweeps_write_all;
    b->buckets = std::move(plan.buckets);
    b->task_reads = std::move(plan.task_reads);
    rc = upload_plan_1d(b, plan, pr, kmin, kmax);
    if (rc) return rc;
    clk.mark("device buffers, H2D");

    const size_t nb = b->buckets.size();
    rc = make_events(b, 2 + 6 * (int)nb + 2);
    if (rc) return rc;
    if (!plan.brute) {
        b->bstreams.assign(nb, nullptr); b->bdone.assign(nb, nullptr);
        for (size_t i = 0; i < nb; ++i) {
            HIP_TRY(g_handles.stream(b->device, &b->bstreams[i]));
            HIP_TRY(g_handles.event(b->device, false, &b->bdone[i]));
        }
        HIP_TRY(g_handles.event(b->device, false, &b->fork_ev));
    }

    clk.mark("events, streams");
    b->stats.n_alignments = plan.n_cands;
    b->stats.algorithmic_cells = plan.alg_cells;
    b->stats.executed_cells = plan.cells_pair + plan.cells_queue + plan.cells_sweep;
    b->stats.algorithmic_bytes = (int64_t)pr.q2bit.size() * 4 + (int64_t)plan.pool.size() + plan.n_cands * 4 + (int64_t)n_reads * 17;
    b->stats.intermediate_bytes = plan.brute ? 0 : 2 * ((int64_t)plan.snap_total + (int64_t)b->q_state.n) * 4;   // the junction snapshot and the wave states at the cut: written, then read
    *out = guard.release();
    return NRA_OK;
}

int64_t nra_plan1d_digest(const nra_region_t* regions, int32_t n_regions,
                          int32_t n_reads, const char* seqs, const int64_t* seq_off,
                          const int32_t* read_region, const int32_t* kmin, const int32_t* kmax,
                          const nra_scoring_t* sc, int32_t flags, int32_t simds, char* buf, int64_t cap)
{
    int rc = check_batch1d_args(regions, n_regions, n_reads, seqs, seq_off, read_region, kmin, kmax, sc);
    if (rc) return rc;
    if (simds <= 0 || cap < 0 || (cap > 0 && !buf)) return fail(NRA_E_ARG, "bad simds / buffer");
    PackedReads pr;
    rc = pack_layout(n_reads, seq_off, read_region, n_regions, pr, NRA_MAX_QLEN);
    if (rc) return rc;
    PhaseClock clk(false);
    Plan1D plan;
    rc = plan_1d(regions, n_regions, pr.reads, kmin, kmax, sc, flags, plan1d_knobs(), simds, clk, plan);
    if (rc) return rc;
    const std::string text = plan_1d_digest(plan);
    if (cap > 0) {
        const size_t n = std::min(text.size(), (size_t)cap - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size() + 1;
}

// what a run of a 1D batch clears first (run_1d; nra_batch1d_clears reports it)
static bool clears_scores_1d(const nra_batch* b) { return !(NRA_LEAN_CLEARS != 0 && b->sweeps_write_all); }
static bool clears_extents_1d(const nra_batch* b) { return NRA_LEAN_CLEARS == 0 || (b->flags & NRA_F_ALL_EXTENTS) != 0; }

static int run_1d(nra_batch* b)
{
    hipStream_t st = b->stream;
    const NraSweepArgs sw = sweep_args(b);
    const NraSeqArgs& seq = sw.seq;
    const size_t nb = b->buckets.size();
    const bool all_ext = (b->flags & NRA_F_ALL_EXTENTS) != 0;
    const size_t nc = (size_t)b->n_cands;
    HIP_TRY(hipEventRecord(b->ev[0], st));
    b->results_staged = false;
    // What a run clears.  cand_score (-1) and cand_flag (2 = "needs the extents DP") only where a kernel of the run may
    // leave a candidate unwritten: the forward sweeps of a batch with sweeps_write_all write both for every candidate.
    // cand_tstart / cand_tend read -1 where no extents were computed: k_select_best_1d writes that on its way through the
    // candidates, but with NRA_F_ALL_EXTENTS the extents kernel runs before it.
    // (NRA_TEST_POISON_OUTPUTS in the environment, tests only: every array that goes uncleared is filled with 0x5a instead,
    // so that a stale or uninitialised value that reached a result would show.)
    const bool clear_scores = clears_scores_1d(b), clear_extents = clears_extents_1d(b);
    const bool poison = getenv("NRA_TEST_POISON_OUTPUTS") != nullptr;
    if (clear_scores || poison) {
        HIP_TRY(hipMemsetAsync(b->cand_score.p, clear_scores ? 0xff : 0x5a, std::max<size_t>(nc, 1) * 4, st));
        HIP_TRY(hipMemsetAsync(b->cand_flag.p, clear_scores ? 2 : 0x5a, std::max<size_t>(nc, 1), st));
    }
    if (clear_extents || poison) {
        HIP_TRY(hipMemsetAsync(b->cand_tstart.p, clear_extents ? 0xff : 0x5a, std::max<size_t>(nc, 1) * 4, st));
        HIP_TRY(hipMemsetAsync(b->cand_tend.p, clear_extents ? 0xff : 0x5a, std::max<size_t>(nc, 1) * 4, st));
    }
    // the words of the run in one memset: the quanta's give-up word, tickets and arrival counters, the row blocks' give-up
    // word, the tie queues' lengths, the re-sweep flags
    HIP_TRY(hipMemsetAsync(b->run_words.p, 0, b->run_words.n * 4, st));
    // (NRA_TEST_MT_GIVEUP in the environment, tests only: the run starts with the give-up words set, as if a wave had
    // timed out -- every waiting wave leaves at its next look and the fetch reports NRA_E_DEVICE)
    const bool test_giveup = getenv("NRA_TEST_MT_GIVEUP") != nullptr;
    if (b->chain_blocks.n > 0) {
        // concurrent row blocks: every block adds its maximum to the read's A (atomicMax; A >= 0)
        HIP_TRY(hipMemsetAsync(b->read_a1d.p, 0, std::max<size_t>((size_t)b->n_reads, 1) * 4, st));
        if (test_giveup) HIP_TRY(hipMemsetAsync(b->mt_giveup, 1, 4, st));
        b->mt_checked = false;
    }
    if (b->q_words_n > 0) {
        if (test_giveup) HIP_TRY(hipMemsetAsync(b->q_words.p, 1, 4, st));
        b->q_checked = false;
    }
    int ev = 2;
    b->n_score_ev = 0; b->n_ext_ev = 0;
    const int max_waves = 256 * 16;
    const bool tie_ext = (b->flags & NRA_F_TIE_EXTENTS) != 0;
    HIP_TRY(hipEventRecord(b->phase_ev[0], st));
    if (!b->brute) {
        // junction decomposition: per bucket a chain reverse sweep -> forward sweep, each chain on
        // its own stream so that short buckets fill the SIMDs a long bucket's tail leaves idle
        HIP_TRY(hipEventRecord(b->fork_ev, st));
        // The exact re-sweep of a tainted bucket's flagged tasks: today's two launches, behind the tainted
        // sweeps on the bucket's stream; every other wave leaves at once.  It rewrites the tasks' R side, A and outputs.
        auto resweep = [&](const Bucket& bk, hipStream_t q, int32_t* redo) {
            int rc2 = nra_launch_sweep_ring_bwd(bk.R, b->has_n, bk.half, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw, 0, redo);
            if (rc2) return rc2;
            return nra_launch_sweep_ring_fwd(bk.R, b->has_n, bk.half, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw, 0, redo);
        };
        // (the order the buckets' chains are launched in makes no difference: 5.50 - 5.61 ms either way on config 2;
        // a bucket's tasks as 2 / 3 / 4 groups with chains of their own are slower: 5.65 -> 6.0 / 5.9 / 7.6 ms)
        std::vector<size_t> order;
        for (size_t i = 0; i < nb; ++i) if (b->buckets[i].mt) order.push_back(i);
        for (size_t i = 0; i < nb; ++i) if (!b->buckets[i].mt) order.push_back(i);
        bool mt_rev_recorded = false;
        // Row-block buckets beside quanta: the launch that is being dispatched keeps the slots its own waves free, so the
        // quanta, started together with the row blocks' reverse launch, kept the forward launch of the row blocks off the
        // device until they were through (config 5: it began at 5.7 of 17.7 ms and then ran alone).  Where the row blocks
        // are the larger share of the work the quanta wait for the reverse launch instead and share the device with the
        // forward one: 17.9 -> 17.35 ms per step.
        int64_t cells_mt = 0, cells_q = 0;
        for (const Bucket& bk : b->buckets) (bk.mt ? cells_mt : cells_q) += bk.quanta || bk.mt ? bk.cells_sweep : 0;
        const bool mt_first = cells_mt > 0 && cells_q > 0 && cells_mt >= cells_q;
        for (size_t oi = 0; oi < nb; ++oi) {
            const size_t i = order[oi];
            const Bucket& bk = b->buckets[i];
            hipStream_t q = b->bstreams[i];
            int32_t* redo = bk.taint ? b->redo.p + bk.sweep_off : nullptr;
            const int relax_c = bk.taint ? b->relax_c : 0;
            HIP_TRY(hipStreamWaitEvent(q, b->fork_ev, 0));
            if (mt_first && bk.quanta && mt_rev_recorded) HIP_TRY(hipStreamWaitEvent(q, b->mt_rev_ev, 0));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            int32_t* strips = bk.chain ? b->chain_sweep.p + bk.strip_off : nullptr;
            if (bk.quanta) {
                // one launch: the sweeps' parts, taken by ticket (two timing pairs like the two launches it replaces: the
                // second one is empty)
                LAUNCH_TRY(nra_launch_sweep_ringq(bk.R, b->has_n, bk.half, q, bk.n_quanta, b->q_list.p + bk.q_off, bk.q_steps, bk.n_sweep,
                                                  b->q_words.p + 1 + i, b->q_words.p + b->q_arrivals_off + bk.q_task_off, b->q_words.p,
                                                  b->q_state.p + bk.q_state_off, b->sweep_tasks.p + bk.sweep_off, sw,
                                                  bk.taint ? b->relax_c : 0, redo, b->sat_steps, b->sat_count.p + 4 * i));
                if (bk.taint) LAUNCH_TRY(resweep(bk, q, redo));
                HIP_TRY(hipEventRecord(b->ev[ev++], q));
                HIP_TRY(hipEventRecord(b->ev[ev++], q));
                HIP_TRY(hipEventRecord(b->ev[ev++], q));
                b->n_score_ev += 2;
                HIP_TRY(hipEventRecord(b->bdone[i], q));
                HIP_TRY(hipStreamWaitEvent(st, b->bdone[i], 0));
                continue;
            }
            if (bk.mt) {
                for (const auto& g : bk.mt_groups)
                    LAUNCH_TRY(nra_launch_sweep_ringmt_bwd(bk.R, b->has_n, bk.wide ? 1 : 0, q, g.second, b->chain_blocks.p + g.first,
                                                           b->mt_words.p + 2 + i, b->sweep_tasks.p + bk.sweep_off, sw,
                                                           b->mt_strips.p + bk.strip_off * 5 * (size_t)b->chain_cap, b->chain_cap,
                                                           next_epoch(), b->mt_giveup));
            } else if (bk.ring && bk.chain)
                LAUNCH_TRY(nra_launch_sweep_ringchain_bwd(bk.R, b->has_n, bk.wide ? 1 : 0, q, bk.n_sweep,
                                                          b->sweep_tasks.p + bk.sweep_off, sw, strips, b->chain_cap, bk.n_strips));
            else if (bk.ring)
                LAUNCH_TRY(nra_launch_sweep_ring_bwd(bk.R, b->has_n, bk.half, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw,
                                                     relax_c, redo));
            else
                LAUNCH_TRY(nra_launch_sweep_bwd(bk.R, b->has_n, bk.chain ? 1 : 0, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw,
                                                strips, b->chain_cap, bk.n_strips));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            if (bk.mt && mt_first) {
                if (!b->mt_rev_ev) HIP_TRY(g_handles.event(b->device, false, &b->mt_rev_ev));
                HIP_TRY(hipEventRecord(b->mt_rev_ev, q));
                mt_rev_recorded = true;
            }
            if (bk.mt) {
                for (const auto& g : bk.mt_groups)
                    LAUNCH_TRY(nra_launch_sweep_ringmt_fwd(bk.R, b->has_n, bk.wide ? 1 : 0, q, g.second, b->chain_blocks.p + g.first,
                                                           b->mt_words.p + 2 + i, b->sweep_tasks.p + bk.sweep_off, sw,
                                                           b->mt_strips.p + bk.strip_off * 5 * (size_t)b->chain_cap, b->chain_cap,
                                                           next_epoch(), b->mt_giveup));
            } else if (bk.ring && bk.chain)
                LAUNCH_TRY(nra_launch_sweep_ringchain_fwd(bk.R, b->has_n, bk.wide ? 1 : 0, q, bk.n_sweep,
                                                          b->sweep_tasks.p + bk.sweep_off, sw, strips, b->chain_cap, bk.n_strips));
            else if (bk.ring)
                LAUNCH_TRY(nra_launch_sweep_ring_fwd(bk.R, b->has_n, bk.half, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw,
                                                     relax_c, redo));
            else
                LAUNCH_TRY(nra_launch_sweep_fwd(bk.R, b->has_n, bk.chain ? 1 : 0, q, bk.n_sweep, b->sweep_tasks.p + bk.sweep_off, sw,
                                                strips, b->chain_cap, bk.n_strips));
            if (bk.taint) LAUNCH_TRY(resweep(bk, q, redo));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            b->n_score_ev += 2;
            HIP_TRY(hipEventRecord(b->bdone[i], q));
            HIP_TRY(hipStreamWaitEvent(st, b->bdone[i], 0));
        }
    } else {
        for (size_t i = 0; i < nb; ++i) {
            const Bucket& bk = b->buckets[i];
            HIP_TRY(hipEventRecord(b->ev[ev++], st));
            if (!all_ext) {
                LAUNCH_TRY(nra_launch_score_pk16(bk.R, b->has_n, st, bk.n_pair, b->pair_tasks.p + bk.pair_off, seq, b->cand_score.p));
            } else {
                LAUNCH_TRY(nra_launch_payload_origin(bk.R, b->has_n, st, std::min(bk.n_queue, max_waves),
                                                  b->queue_tasks.p + bk.queue_off, b->queue_count.p + i, seq, b->cand_score.p,
                                                  b->cand_tstart.p, b->cand_tend.p, nullptr, 0, 0));
            }
            HIP_TRY(hipEventRecord(b->ev[ev++], st));
            b->n_score_ev++;
        }
    }
    HIP_TRY(hipEventRecord(b->phase_ev[1], st));
    // ties that need the explicit extents DP: all of them (brute force / TIE_EXTENTS), or only those
    // whose three-score flank verdict is ambiguous
    const int append_mode = all_ext ? 0 : ((b->brute || tie_ext) ? 2 : 1);
    LAUNCH_TRY(nra_launch_select_best_1d(st, b->n_reads, b->kmin.p, b->kmax.p, b->coff.p, b->cand_score.p,
                                         b->cand_flag.p, b->read_bucket.p, b->bucket_task_base.p, append_mode,
                                         b->queue_tasks.p, b->tie_count.p, b->best_score.p,
                                         clear_extents ? nullptr : b->cand_tstart.p, clear_extents ? nullptr : b->cand_tend.p));
    if (!all_ext) {
        for (size_t i = 0; i < nb; ++i) {
            const Bucket& bk = b->buckets[i];
            HIP_TRY(hipEventRecord(b->ev[ev++], st));
            // chained reads: int64 cells (scores and extents of any size)
            LAUNCH_TRY(nra_launch_payload_origin(bk.chain ? bk.payload_R : bk.R, b->has_n, st,
                                              (int)std::min<size_t>(bk.queue_cap, bk.chain ? (size_t)b->payload_strips : (size_t)max_waves),
                                              b->queue_tasks.p + bk.queue_off, b->tie_count.p + i, seq, b->cand_score.p,
                                              b->cand_tstart.p, b->cand_tend.p,
                                              bk.chain ? b->chain_payload.p : nullptr, b->chain_cap, bk.chain ? 1 : 0));
            HIP_TRY(hipEventRecord(b->ev[ev++], st));
            b->n_ext_ev++;
        }
    }
    LAUNCH_TRY(nra_launch_select_final_1d(st, b->n_reads, b->kmin.p, b->kmax.p, b->coff.p, b->reads.p,
                                          b->regions.p, b->cand_score.p, b->cand_flag.p, b->cand_tstart.p,
                                          b->cand_tend.p, b->best_score.p, b->sum_k.p, b->n_ties.p, b->status.p,
                                          b->q_words_n > 0 ? b->q_words.p : nullptr,
                                          b->chain_blocks.n > 0 ? b->mt_giveup : nullptr, b->giveup_out));
    HIP_TRY(hipEventRecord(b->ev[1], st));
    return NRA_OK;
}

// After a run with concurrent-block sweeps: did a wave give up waiting for the block above it?  (A hang guard that
// should never fire; if it does the results of this run are not to be used.)
static int check_mt(nra_batch* b)
{
    if (!b->q_checked && b->q_words_n > 0) {
        int32_t gave_up = 0;
        HIP_TRY(hipMemcpy(&gave_up, b->q_words.p, 4, hipMemcpyDeviceToHost));
        b->q_checked = true;
        if (gave_up) return fail(NRA_E_DEVICE, "sweep in quanta: a second part timed out waiting for its reverse sweep / first part");
    }
    if (b->mt_checked || b->chain_blocks.n == 0) return NRA_OK;
    int32_t failed = 0;
    HIP_TRY(hipMemcpy(&failed, b->mt_giveup, 4, hipMemcpyDeviceToHost));
    b->mt_checked = true;
    if (failed) return fail(NRA_E_DEVICE, "chained sweep: a row block timed out waiting for the block above it");
    return NRA_OK;
}

// The same after a run of a 1D batch with reads, without a copy of its own: k_select_final_1d, the run's last kernel, left
// both give-up words behind the per-read results, and one copy brings the whole block to the pinned mirror.  The stream is
// idle.  nra_batch_sync stages the block and nra_batch1d_fetch finds it there; a fetch without a sync stages it itself.
static int stage_results_1d(nra_batch* b)
{
    if (!b->results_staged) {
        const int rc = fetch_results(b);
        if (rc) return rc;
        b->results_staged = true;
    }
    if (!b->ran) return NRA_OK;                             // (no run yet: nothing has written the words)
    int32_t words[2];
    memcpy(words, static_cast<const uint8_t*>(b->result_stage) + (reinterpret_cast<const uint8_t*>(b->giveup_out) - b->result_block.p), 8);
    b->q_checked = true; b->mt_checked = true;
    if (words[0]) return fail(NRA_E_DEVICE, "sweep in quanta: a second part timed out waiting for its reverse sweep / first part");
    if (words[1]) return fail(NRA_E_DEVICE, "chained sweep: a row block timed out waiting for the block above it");
    return NRA_OK;
}
static bool one_copy_1d(const nra_batch* b) { return NRA_FETCH_ONE_COPY != 0 && b->kind == 1 && b->n_reads > 0 && b->giveup_out; }

int nra_batch1d_fetch(nra_batch_t* b, int32_t* best_score, int64_t* sum_k, int32_t* n_ties,
                      uint8_t* status, int32_t* cand_score, int32_t* cand_tstart, int32_t* cand_tend)
{
    if (!b || b->kind != 1) return fail(NRA_E_ARG, "not a 1D batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    {
        const int rcm = one_copy_1d(b) ? stage_results_1d(b) : check_mt(b);
        if (rcm) return rcm;
    }
    // (after a refinement the per-cell arrays are the refinement's: (2 buf1)(2 buf2) entries a read)
    const size_t n = (size_t)b->n_reads, nc = (size_t)(b->refined ? b->rf_n_cands : b->n_cands);
    const int32_t* src_score = b->refined ? b->rf_cell_score.p : b->cand_score.p;
    const int32_t* src_wscore = b->refined ? b->rf_cell_wscore.p : b->cand_tstart.p;
    if (n) {
        if (!one_copy_1d(b)) {
            int rc = fetch_results(b);
            if (rc) return rc;
        }
        if (best_score) memcpy(best_score, staged(b, b->best_score), n * 4);
        if (sum_k) memcpy(sum_k, staged(b, b->sum_k), n * 8);
        if (n_ties) memcpy(n_ties, staged(b, b->n_ties), n * 4);
        if (status) memcpy(status, staged(b, b->status), n);
        if (best_score)
            for (size_t i = 0; i < n; ++i) if (best_score[i] < 0) best_score[i] = 0;
    }
    if (nc) {
        if (cand_score) HIP_TRY(copy_d2h(cand_score, b->cand_score.p, nc * 4));
        if (cand_tstart) HIP_TRY(copy_d2h(cand_tstart, b->cand_tstart.p, nc * 4));
        if (cand_tend) HIP_TRY(copy_d2h(cand_tend, b->cand_tend.p, nc * 4));
    }
    return NRA_OK;
}

// A large many-region call in region blocks: block i + 1 is packed, bucketed and uploaded (host work + H2D) while
// the kernels of block i run, so that the host's share of the call (config 4: ~90 of ~345 ms) hides behind the
// device's.  Reads of a region stay in one block (the sweeps pair two or four reads of a region per wave); needs
// the reads grouped by region (read_region non-decreasing), which is how the host mirror lists them.
#define NRA_STREAM_MIN_READS 131072
static int round3_1d_streamed(int device, const nra_region_t* regions, int32_t n_regions, int32_t n_reads,
                              const char* seqs, const int64_t* seq_off, const int32_t* read_region,
                              const int32_t* kmin, const int32_t* kmax, const nra_scoring_t* sc, int32_t flags,
                              int32_t* best_score, int64_t* sum_k, int32_t* n_ties, uint8_t* status,
                              int32_t* cand_score, int32_t* cand_tstart, int32_t* cand_tend)
{
    // Up to 8 blocks of equal size.  Measured on config 4 (1 M reads, one box, ms per call): 16 blocks 350 -- every launch a
    // sixteenth of its bucket --, 8 blocks 304-314, 4 blocks 300-312, 2 blocks 330-337 (the first block's host work is not
    // hidden), blocks of doubling size 353-359 (the last block's device chunk is too large for the chunk cache: a
    // hipMalloc / hipFree of several GB per call); the resident batch's step is 281.
    const int n_blocks = (int)std::min<int64_t>(8, std::max<int64_t>(2, n_reads / 120000));
    struct Block { int32_t r0, r1, g0, g1; int64_t c0; };
    std::vector<Block> blocks;
    {
        int64_t cands = 0;
        int32_t r = 0;
        for (int i = 0; i < n_blocks && r < n_reads; ++i) {
            Block bl{r, r, read_region[r], 0, cands};
            const int32_t want = (int32_t)((int64_t)n_reads * (i + 1) / n_blocks);
            while (r < n_reads && (r < want || read_region[r] == read_region[r - 1])) {      // whole regions only
                cands += std::max<int64_t>(0, (int64_t)kmax[r] - kmin[r] + 1);
                ++r;
            }
            if (i == n_blocks - 1) for (; r < n_reads; ++r) cands += std::max<int64_t>(0, (int64_t)kmax[r] - kmin[r] + 1);
            bl.r1 = r; bl.g1 = read_region[r - 1] + 1;
            if (bl.r1 > bl.r0) blocks.push_back(bl);
        }
    }
    std::vector<nra_batch_t*> live(blocks.size(), nullptr);
    std::vector<std::vector<int32_t>> local_region(blocks.size());
    int rc = NRA_OK;
    auto finish = [&](size_t i) {
        if (!live[i]) return;
        const Block& bl = blocks[i];
        if (!rc) rc = nra_batch_sync(live[i]);
        if (!rc) rc = nra_batch1d_fetch(live[i], best_score + bl.r0, sum_k + bl.r0, n_ties + bl.r0, status + bl.r0,
                                        cand_score ? cand_score + bl.c0 : nullptr, cand_tstart ? cand_tstart + bl.c0 : nullptr,
                                        cand_tend ? cand_tend + bl.c0 : nullptr);
        nra_batch_destroy(live[i]);
        live[i] = nullptr;
    };
    for (size_t i = 0; i < blocks.size() && !rc; ++i) {
        const Block& bl = blocks[i];
        std::vector<int32_t>& lr = local_region[i];
        lr.resize((size_t)(bl.r1 - bl.r0));
        for (int32_t r = bl.r0; r < bl.r1; ++r) lr[(size_t)(r - bl.r0)] = read_region[r] - bl.g0;
        rc = nra_batch1d_create(device, regions + bl.g0, bl.g1 - bl.g0, bl.r1 - bl.r0, seqs, seq_off + bl.r0, lr.data(),
                                kmin + bl.r0, kmax + bl.r0, sc, flags, &live[i]);
        if (!rc) rc = nra_batch_run(live[i]);
        if (i >= 2) finish(i - 2);              // at most three blocks alive: running, queued, being built
    }
    for (size_t i = 0; i < blocks.size(); ++i) finish(i);
    return rc;
}

int nra_round3_1d(int device, const nra_region_t* regions, int32_t n_regions, int32_t n_reads,
                  const char* seqs, const int64_t* seq_off, const int32_t* read_region,
                  const int32_t* kmin, const int32_t* kmax, const nra_scoring_t* sc, int32_t flags,
                  int32_t* best_score, int64_t* sum_k, int32_t* n_ties, uint8_t* status,
                  int32_t* cand_score, int32_t* cand_tstart, int32_t* cand_tend)
{
    if (n_reads > 0 && (!best_score || !sum_k || !n_ties || !status)) return fail(NRA_E_ARG, "NULL output array");
    nra_batch_t* b = nullptr;
    if (cand_tstart || cand_tend) flags |= NRA_F_TIE_EXTENTS;
    if (n_reads >= NRA_STREAM_MIN_READS && n_regions > 1 && read_region && regions && seqs && seq_off && kmin && kmax) {
        bool grouped = true;
        for (int32_t r = 0; r < n_reads && grouped; ++r)
            grouped = read_region[r] >= 0 && read_region[r] < n_regions && (r == 0 || read_region[r] >= read_region[r - 1]);
        if (grouped)
            return round3_1d_streamed(device, regions, n_regions, n_reads, seqs, seq_off, read_region, kmin, kmax, sc,
                                      flags, best_score, sum_k, n_ties, status, cand_score, cand_tstart, cand_tend);
    }
    int rc = nra_batch1d_create(device, regions, n_regions, n_reads, seqs, seq_off, read_region, kmin,
                                kmax, sc, flags, &b);
    if (rc) return rc;
    rc = nra_batch_run(b);
    if (!rc) rc = nra_batch_sync(b);
    if (!rc) rc = nra_batch1d_fetch(b, best_score, sum_k, n_ties, status, cand_score, cand_tstart, cand_tend);
    nra_batch_destroy(b);
    return rc;
}

// ---- 2D -----------------------------------------------------------------------------
static int account_run(nra_batch* b);
static int account_run_fwd(nra_batch* b) { return account_run(b); }

int nra_batch2d_create_reads(int device, const nra_joint_region_t* reg, int32_t n_reads, const char* seqs,
                             const int64_t* seq_off, const nra_scoring_t* sc, int32_t flags, nra_batch_t** out)
{
    if (!out) return fail(NRA_E_ARG, "out is NULL");
    *out = nullptr;
    if (!reg || n_reads < 0) return fail(NRA_E_ARG, "bad region / counts");
    if (n_reads > 0 && (!seqs || !seq_off)) return fail(NRA_E_ARG, "NULL input array");
    if (!scoring_ok(sc)) return fail(NRA_E_ARG, "scoring parameters out of range");
    if (reg->left_len < 0 || reg->right_len < 0 || reg->mid_len < 0 || reg->unit1_len <= 0 ||
        reg->unit2_len <= 0 || !reg->unit1 || !reg->unit2)
        return fail(NRA_E_ARG, "bad joint region");

    nra_batch* b = new nra_batch();
    std::unique_ptr<nra_batch> guard(b);
    ArenaScope arena_scope(&b->arena);
    b->kind = 2; b->n_reads = n_reads; b->n_regions = 1; b->n_cands = 0;
    int rc = common_init(b, device, sc, flags);
    if (rc) return rc;
    b->scoring = *sc;
    b->jr.left.assign(reg->left ? reg->left : "", (size_t)reg->left_len);
    b->jr.unit1.assign(reg->unit1, (size_t)reg->unit1_len);
    b->jr.mid.assign(reg->mid ? reg->mid : "", (size_t)reg->mid_len);
    b->jr.unit2.assign(reg->unit2, (size_t)reg->unit2_len);
    b->jr.right.assign(reg->right ? reg->right : "", (size_t)reg->right_len);

    PackedReads pr;
    rc = pack_reads(n_reads, seqs, seq_off, nullptr, 1, pr, NRA_MAX_QLEN);
    if (rc) return rc;
    plan_2d_reads(pr.reads, reg->left_len, reg->right_len, sc, flags, b->r2);
    b->carried.init(n_reads);
    const uint64_t jpack_ints = b->r2.jpack_ints;
    b->arena.expect(pr.q2bit.size() * 6 + (size_t)n_reads * 96 + (size_t)reg->left_len + (size_t)reg->right_len + (1u << 20) +
                    ((b->r2.jpack_l ? jpack_ints : 0) + (b->r2.jpack_r ? jpack_ints : 0)) * 4);
    HIP_TRY(b->q2bit.upload(pr.q2bit));
    HIP_TRY(b->qnmask.upload(pr.nmask));
    b->n_q2bit_words = pr.q2bit.size();
    b->reads_have_n = pr.has_n;
    b->host_reads = std::move(pr.reads);
    if (b->r2.jpack_l) HIP_TRY(b->jlstate.alloc((size_t)jpack_ints));
    if (b->r2.jpack_r) HIP_TRY(b->jrstate.alloc((size_t)jpack_ints));
    if ((b->r2.jpack_l || b->r2.jpack_r) && reg->left_len >= 1 && reg->right_len >= 2 && n_reads > 0) {
        // what flank sweeps ahead of a cell list read (nra_batch2d_sweep_flanks): L and rev(R) alone, the oriented reads,
        // the pair tasks -- buffers of the batch, not of a cell list
        std::vector<uint8_t> pool;
        bool has_n = b->reads_have_n;
        NraDevRegion d{};
        d.p1_off = pool_append(pool, b->jr.left.data(), reg->left_len, nullptr, 0, 0, has_n);
        std::string rr(b->jr.right);
        std::reverse(rr.begin(), rr.end());
        d.pr_off = pool_append(pool, rr.data(), reg->right_len, nullptr, 0, 0, has_n);
        d.p2_off = d.p3_off = (uint32_t)pool.size();
        d.l1 = reg->left_len; d.m1 = reg->unit1_len; d.l2 = reg->mid_len; d.m2 = reg->unit2_len; d.l3 = reg->right_len;
        pool.push_back(0);
        b->warm_has_n = has_n ? 1 : 0;
        HIP_TRY(b->warm_pool.upload(pool));
        HIP_TRY(b->warm_region.upload(std::vector<NraDevRegion>(1, d)));
        HIP_TRY(b->warm_reads.alloc((size_t)n_reads));
        HIP_TRY(b->warm_tasks.alloc(2 * b->r2.jpairs.size()));
        b->warm_built = true;
    }
    HIP_TRY(b->jsnap.alloc(b->n_q2bit_words * 16 * 3));    // R side of the junction per read base: kept across cell lists
    HIP_TRY(b->jread_a.alloc((size_t)n_reads));
    rc = alloc_results(b, (size_t)n_reads, true);      // best_wscore, n_ties, sum_k, sum_k2, status, strand_out
    if (rc) return rc;
    for (int i = 0; i < 2; ++i) HIP_TRY(g_handles.event(b->device, true, &b->phase_ev[i]));
    HIP_TRY(g_handles.event(b->device, false, &b->fork_ev));
    HIP_TRY(g_handles.event(b->device, false, &b->fork2_ev));
    *out = guard.release();
    return NRA_OK;
}

}  // extern "C"

namespace {

int set_cells_common(nra_batch* b, const int8_t* read_strand, int64_t n_cells, const int32_t* cell_read,
                     const int32_t* cell_k1, const int32_t* cell_k2, const JointGrid* grid);
int run_2d_flanks(nra_batch* b);

}  // namespace

extern "C" {

int64_t nra_joint_grid_cells(int32_t n_reads, int32_t start1, int32_t step1, int32_t count1, const double* lo1,
                             const double* hi1, int32_t start2, int32_t step2, int32_t count2, const double* lo2,
                             const double* hi2, int64_t cap, int32_t* cell_read, int32_t* cell_k1, int32_t* cell_k2)
{
    std::vector<GridRow> rows;
    int64_t n = 0;
    const int rc = route_grid(n_reads, start1, step1, count1, lo1, hi1, start2, step2, count2, lo2, hi2, rows, n);
    if (rc) return rc;
    if (!cell_read && !cell_k1 && !cell_k2) return n;
    if (!cell_read || !cell_k1 || !cell_k2) return fail(NRA_E_ARG, "all three cell arrays or none");
    if (cap < n) return fail(NRA_E_ARG, "cell arrays too small: " + std::to_string(n) + " cells");
    int64_t c = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        const GridRow& g = rows[(size_t)r];
        for (int32_t i = 0; i < g.n1; ++i)
            for (int32_t j = 0; j < g.n2; ++j, ++c) {
                cell_read[c] = r; cell_k1[c] = g.k1lo + i * step1; cell_k2[c] = g.k2lo + j * step2;
            }
    }
    return n;
}

// The cell list of one grid round.  May be called again on the same batch (the reads stay packed on the
// device; the buffers of the previous list are handed out again).
int nra_batch2d_set_cells(nra_batch_t* b, const int8_t* read_strand, int64_t n_cells, const int32_t* cell_read,
                          const int32_t* cell_k1, const int32_t* cell_k2)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    if (n_cells < 0) return fail(NRA_E_ARG, "bad cell count");
    if (n_cells > 0 && (!cell_read || !cell_k1 || !cell_k2)) return fail(NRA_E_ARG, "NULL cell array");
    return set_cells_common(b, read_strand, n_cells, cell_read, cell_k1, cell_k2, nullptr);
}

// The same for a whole routed grid: the library lists the cells itself (no per-cell arrays cross the boundary).
int nra_batch2d_set_grid(nra_batch_t* b, const int8_t* read_strand,
                         int32_t start1, int32_t step1, int32_t count1, const double* lo1, const double* hi1,
                         int32_t start2, int32_t step2, int32_t count2, const double* lo2, const double* hi2,
                         int64_t* n_cells_out)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    std::vector<GridRow> rows, keep;
    int64_t n = 0;
    int rc = route_grid(b->n_reads, start1, step1, count1, lo1, hi1, start2, step2, count2, lo2, hi2, rows, n, &keep);
    if (rc) return rc;
    if (n_cells_out) *n_cells_out = n;
    const JointGrid grid{step1, step2, rows.data(), keep.data()};
    // no per-cell arrays at all: the tasks come from the rows, the selector gets the rows (16 bytes a read)
    rc = set_cells_common(b, read_strand, n, nullptr, nullptr, nullptr, &grid);
    if (rc == NRA_E_NOMEM && b->joint_keep == 1) {
        // The kept column states did not fit after all (the check against the free memory races with other batches, ranks
        // and libraries on the device): give the arena back and set the grid again without keeping -- a later, finer grid
        // then sweeps again, nra_batch2d_refine says NRA_E_STATE, the results are the same.
        b->keep_arena.release();
        b->carried.keep_valid = false;
        b->keep_off = true;
        rc = set_cells_common(b, read_strand, n, nullptr, nullptr, nullptr, &grid);
        b->keep_off = false;
    }
    return rc;
}

}  // extern "C"

namespace {

// the budget of the kept column states, in bytes
// (NRA_JOINT_KEEP_BUDGET_GB in the environment overrides the built-in budget; 0 keeps nothing)
uint64_t joint_keep_budget()
{
    const char* budget_env = getenv("NRA_JOINT_KEEP_BUDGET_GB");
    return budget_env ? (uint64_t)(atof(budget_env) * (double)(1ull << 30)) : (uint64_t)NRA_JOINT_KEEP_BUDGET;
}

// The phases of a cell list in their fixed order: wait and account, reset, the strand-only plan (plan_2d_strands), its
// uploads, its kernels, the plan of the cells (plan_2d_cells), its uploads, the statistics.
int set_cells_common(nra_batch* b, const int8_t* read_strand, int64_t n_cells, const int32_t* cell_read,
                     const int32_t* cell_k1, const int32_t* cell_k2, const JointGrid* grid)
{
    if (!cells_2d_countable(n_cells)) return fail(NRA_E_RANGE, "too many cells");
    HIP_TRY(hipSetDevice(b->device));
    if (b->ran) HIP_TRY(hipStreamSynchronize(b->stream));      // the previous list's kernels own the buffers
    if (b->flanks_enqueued) {                                  // ... also when only its first part was enqueued
        for (hipStream_t q : b->bstreams) HIP_TRY(hipStreamSynchronize(q));
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->flanks_enqueued = false;
    }
    {
        int rc0 = account_run_fwd(b);
        if (rc0) return rc0;
    }
    b->have_cells = false;
    b->ran = false;
    const bool had_warm = b->warm_pending;                     // flank sweeps enqueued ahead of this list (nra_batch2d_sweep_flanks)
    b->cell_arena.reset();
    ArenaScope arena_scope(&b->cell_arena);
    b->buckets.clear();
    b->jgroups.clear();
    b->n_cands = n_cells;
    const int32_t n_reads = b->n_reads;
    PhaseClock clk(g_debug_phases);

    Cells2D cl;
    cl.read_strand = read_strand; cl.n_cells = n_cells; cl.grid = grid;
    cl.cell_read = cell_read; cl.cell_k1 = cell_k1; cl.cell_k2 = cell_k2;
    KeepInputs ki;
    ki.budget = joint_keep_budget();
    ki.keep_off = b->keep_off;
    for (const Arena::Chunk& c : b->keep_arena.chunks) ki.held += c.size;
    ki.device_free = [](uint64_t& free_b) {
        size_t f = 0, total_b = 0;
        if (hipMemGetInfo(&f, &total_b) != hipSuccess) return false;
        free_b = f;
        return true;
    };
    Plan2D plan;
    {
        const int rc1 = plan_2d_strands(b->jr, b->host_reads, b->reads_have_n, b->r2, b->flags, cl, ki, clk, b->carried,
                                        b->pending, plan);
        if (rc1) return rc1;
    }
    const int keep = plan.keep;
    b->joint_keep = keep;
    if (keep == 1) {
        // what the arena holds is handed out again; if it is too small it goes back BEFORE the larger chunk is asked for
        // (old and new together may not fit)
        if (g_debug_phases)
            fprintf(stderr, "[nra] kept column states: %.3f GB wanted, the arena holds %.3f GB in %zu chunks -> %s\n", (double)plan.keep_bytes / 1073741824.0,
                    (double)b->keep_arena.capacity() / 1073741824.0, b->keep_arena.chunks.size(),
                    b->keep_arena.capacity() < plan.keep_bytes + (2u << 20) ? "given back, asked for again" : "handed out again");
        if (b->keep_arena.capacity() < plan.keep_bytes + (2u << 20)) b->keep_arena.release();
        else b->keep_arena.reset();
    }
    b->has_n = plan.has_n ? 1 : 0;
    b->brute = plan.brute;
    b->joint_v2 = plan.joint_v2;
    b->joint_chain = plan.joint_chain;
    b->cells_need_clear = plan.cells_need_clear;
    b->all_strands_given = plan.all_strands_given;
    b->buckets = plan.buckets;                                 // (part 2 completes them, below)
    const size_t nb = b->buckets.size();
    clk.mark("2D cells: pool, strand-only tasks built");
    // one chunk for everything but the wave states, which get their own (all of it reused by the next cell list)
    b->cell_arena.expect(cell_arena_bytes(b->n_q2bit_words, n_cells, plan.pool.size(), n_reads));
    HIP_TRY(b->pool.upload(plan.pool));
    HIP_TRY(b->regions.upload(plan.dregs));
    HIP_TRY(b->reads.upload(plan.reads));
    HIP_TRY(b->reads_init.upload(plan.reads));
    HIP_TRY(b->pair_tasks.upload(plan.pair_tasks));
    HIP_TRY(b->probe_tasks.upload(plan.probe_tasks));
    HIP_TRY(b->probe_count.upload(plan.probe_count));
    HIP_TRY(b->probe_dummy.alloc(2 * (size_t)n_reads));
    HIP_TRY(b->probe_score.alloc(2 * (size_t)n_reads));
    b->have_strand_in = read_strand != nullptr;
    if (read_strand) {
        std::vector<int8_t> v(read_strand, read_strand + n_reads);
        HIP_TRY(b->strand_in.upload(v));
    }
    if (plan.chain_cap > 0) {                                  // chained reads are listed
        b->chain_cap = plan.chain_cap;
        b->payload_strips = plan.payload_strips;
        HIP_TRY(b->chain_payload.alloc((size_t)b->payload_strips * 6 * (size_t)b->chain_cap));
    }
    if (!b->brute) {
        HIP_TRY(b->jbwd_tasks.upload(plan.jbwd));
        HIP_TRY(b->jlpk_tasks.upload(plan.jlpk));
        HIP_TRY(b->jrpk_tasks.upload(plan.jrpk));
        if (b->joint_v2 && keep != 2) {
            ArenaScope kept(keep == 1 ? &b->keep_arena : &b->cell_arena);
            if (keep == 1) b->keep_arena.expect((size_t)plan.rs_total * 4 + (size_t)plan.ra_total * 4 + (1u << 20));
            HIP_TRY(b->jrs.alloc((size_t)plan.rs_total));
            HIP_TRY(b->jra.alloc((size_t)plan.ra_total));
        }
    }
    // events and streams: kept from one cell list to the next, more taken from the pool when needed
    auto ensure_handles = [&](size_t n_ev) -> int {
        while (b->ev.size() < n_ev) { hipEvent_t e; HIP_TRY(g_handles.event(b->device, true, &e)); b->ev.push_back(e); }
        // two streams per bucket: the buckets' chains overlap, and so do a bucket's reverse and prefix sweeps
        while (b->bstreams.size() < 2 * nb) { hipStream_t q; HIP_TRY(g_handles.stream(b->device, &q)); b->bstreams.push_back(q); }
        while (b->bdone.size() < 3 * nb) { hipEvent_t e; HIP_TRY(g_handles.event(b->device, false, &e)); b->bdone.push_back(e); }
        return NRA_OK;
    };
    {
        const int rc1 = ensure_handles((b->warm_pending ? (size_t)b->ev_next : 2) + 12 * nb + 2);
        if (rc1) return rc1;
    }
    clk.mark("2D cells: strand-only uploads, handles");
    b->flanks_enqueued = false;
    if (b->all_strands_given && !b->brute && n_cells > 0) {
        const int rc1 = run_2d_flanks(b);
        if (rc1) return rc1;
    }
    clk.mark("2D cells: strand-only kernels enqueued");

    plan_2d_cells(b->host_reads, b->r2, cl, b->n_q2bit_words, had_warm ? b->warm_cells : 0, b->carried, plan);
    b->buckets = std::move(plan.buckets);
    b->jgroups = std::move(plan.jgroups);

    clk.mark("2D cells: prefix and tail sweeps built");
    HIP_TRY(b->queue_tasks.upload(plan.queue_tasks));
    HIP_TRY(b->queue_count.upload(plan.queue_count));
    if (!b->brute) {
        HIP_TRY(b->jpre_tasks.upload(plan.jpre));
        HIP_TRY(b->jtail_tasks.upload(plan.jtail));
        HIP_TRY(b->jk1list.upload(plan.k1list));
        if (keep != 2) {
            ArenaScope kept(keep == 1 ? &b->keep_arena : &b->cell_arena);
            if (keep == 1) b->keep_arena.expect((size_t)plan.state_base * 4 + (1u << 20));
            HIP_TRY(b->jstate.alloc((size_t)plan.state_base));
        }
        if (b->joint_v2) {
            HIP_TRY(b->jfs.alloc((size_t)plan.fs_total));
            HIP_TRY(b->jfb.alloc((size_t)plan.fb_total));
            HIP_TRY(b->jcomb_tasks.upload(plan.jcomb));
        }
    }
    b->carried.set_current(grid, n_reads);
    b->grid_step1 = b->grid_step2 = 0;
    if (grid) {                                        // the selector computes k1 / k2 of a cell from the read's row
        std::vector<GridRow> rows(grid->rows, grid->rows + n_reads);
        HIP_TRY(b->grid_rows.upload(rows));
        b->grid_step1 = grid->step1; b->grid_step2 = grid->step2;
    } else {
        std::vector<int32_t> v(cell_k1, cell_k1 + n_cells); HIP_TRY(b->cell_k1.upload(v));
        std::vector<int32_t> w(cell_k2, cell_k2 + n_cells); HIP_TRY(b->cell_k2.upload(w));
    }
    HIP_TRY(b->cell_first.upload(plan.first));
    HIP_TRY(b->cell_cnt.upload(plan.cnt));
    HIP_TRY(b->cand_score.alloc((size_t)n_cells));     // cell_score
    HIP_TRY(b->cand_tstart.alloc((size_t)n_cells));    // cell_wscore
    clk.mark("2D cells: device buffers, H2D");
    {
        const int rc1 = ensure_handles((b->warm_pending || b->flanks_enqueued ? (size_t)b->ev_next : 2) + 12 * nb + 4 * b->jgroups.size() + 2);
        if (rc1) return rc1;
    }

    b->stats.n_alignments = plan.stats.n_alignments;
    b->stats.algorithmic_cells = plan.stats.algorithmic_cells;
    b->stats.executed_cells = plan.stats.executed_cells;
    b->stats.algorithmic_bytes = plan.stats.algorithmic_bytes;
    b->stats.intermediate_bytes = plan.stats.intermediate_bytes;
    b->have_cells = true;
    return NRA_OK;
}

}  // namespace

extern "C" {

// Forget what earlier cell lists left for later ones (the reverse sweeps): the next list starts like the first.
int nra_batch2d_invalidate(nra_batch_t* b)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    b->carried.invalidate();
    return NRA_OK;
}

// The flank sweeps of a joint run ahead of its cell list.  The packed sweeps of L and rev(R) outside the scoring window
// (k_joint_pk16) depend on the reads and their strands only -- not on ranges, grids or cells -- and are the first third
// of a round's device time: a caller that knows the strands (round 1 does) enqueues them HERE, before it derives step
// sizes, bounds and grids on the host, and the device works through that host time instead of idling.  The cell lists
// that follow find the flank states valid (like a later list of the same batch) and sweep no flank.
int nra_batch2d_sweep_flanks(nra_batch_t* b, const int8_t* read_strand)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    const int32_t n_reads = b->n_reads;
    if (n_reads > 0 && !read_strand) return fail(NRA_E_ARG, "NULL strand array");
    const int32_t left_len = (int32_t)b->jr.left.size(), right_len = (int32_t)b->jr.right.size();
    if (!sweeps_flanks_ahead(b->r2, b->flags, left_len, right_len, n_reads))
        return NRA_OK;                                         // nothing this batch sweeps ahead of time
    HIP_TRY(hipSetDevice(b->device));
    if (b->ran) HIP_TRY(hipStreamSynchronize(b->stream));      // an earlier list's kernels read the flank states
    if (b->flanks_enqueued || b->warm_pending) {
        for (hipStream_t q : b->bstreams) HIP_TRY(hipStreamSynchronize(q));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    {
        int rc0 = account_run_fwd(b);
        if (rc0) return rc0;
    }
    ArenaScope arena_scope(&b->arena);
    if (!b->warm_built) return NRA_OK;
    // the reads as the kernels orient them (what k_pick_strand leaves in the cell list's own copy)
    std::vector<NraDevRead> reads(b->host_reads.begin(), b->host_reads.begin() + n_reads);
    for (int32_t r = 0; r < n_reads; ++r) reads[(size_t)r].rc = read_strand[r] < 0 ? 1 : 0;
    FlankPlan fp;
    plan_2d_flanks(b->r2, b->carried, read_strand, left_len, right_len, fp);
    const std::vector<FlankPart>& parts = fp.parts;
    if (parts.empty()) return NRA_OK;
    HIP_TRY(copy_h2d(b->warm_reads.p, reads.data(), reads.size() * sizeof(NraDevRead)));
    HIP_TRY(copy_h2d(b->warm_tasks.p, fp.tasks.data(), fp.tasks.size() * sizeof(NraJointPairTask)));
    const size_t np = parts.size();
    while (b->bstreams.size() < 2 * np) { hipStream_t q; HIP_TRY(g_handles.stream(b->device, &q)); b->bstreams.push_back(q); }
    while (b->warm_ev.size() < 2 * np) { hipEvent_t e; HIP_TRY(g_handles.event(b->device, false, &e)); b->warm_ev.push_back(e); }
    while (b->ev.size() < 2 + 4 * np + 2) { hipEvent_t e; HIP_TRY(g_handles.event(b->device, true, &e)); b->ev.push_back(e); }
    hipStream_t st = b->stream;
    // these sweeps read buffers of their own: the cell list's are rebuilt while they run
    NraSeqArgs warm = seq_args(b);
    warm.reads = b->warm_reads.p; warm.regions = b->warm_region.p; warm.pool = b->warm_pool.p;
    HIP_TRY(hipEventRecord(b->ev[0], st));
    HIP_TRY(hipEventRecord(b->phase_ev[0], st));
    HIP_TRY(hipEventRecord(b->fork2_ev, st));
    int ev = 2;
    b->n_score_ev = 0; b->n_ext_ev = 0;
    for (size_t i = 0; i < np; ++i) {
        const FlankPart& pt = parts[i];
        hipStream_t qa = b->bstreams[2 * i], qb = b->bstreams[2 * i + 1];
        HIP_TRY(hipStreamWaitEvent(qa, b->fork2_ev, 0));
        HIP_TRY(hipStreamWaitEvent(qb, b->fork2_ev, 0));
        // both sides of a rows-per-lane class in ONE launch, L- and R-side tasks alternating: the two chains behind them
        // (prefix sweeps; extended reverse sweeps) carry about the same work and meet again in the cells, so neither side's
        // waves should be the older ones (two launches: the first one's waves issue first, its side finishes 1.4 ms ahead)
        HIP_TRY(hipEventRecord(b->ev[ev++], qa));
        LAUNCH_TRY(nra_launch_joint_pk16(pt.R, b->warm_has_n, qa, (int)(pt.n_l + pt.n_r), b->warm_tasks.p + pt.off, warm, -1,
                                         b->jrstate.p, b->jlstate.p));
        HIP_TRY(hipEventRecord(b->ev[ev++], qa));
        b->n_score_ev++;
        HIP_TRY(hipEventRecord(b->warm_ev[2 * i], qa));
        HIP_TRY(hipEventRecord(b->warm_ev[2 * i + 1], qa));
    }
    b->warm_R.clear();
    for (const FlankPart& pt : parts) b->warm_R.push_back(pt.R);
    b->ev_next = ev;
    b->warm_pending = true;
    b->warm_cells = fp.cells;
    commit_2d_flanks(b->carried, fp);
    return NRA_OK;
}

int nra_batch2d_create(int device, const nra_joint_region_t* reg, int32_t n_reads, const char* seqs,
                       const int64_t* seq_off, const int8_t* read_strand, int64_t n_cells,
                       const int32_t* cell_read, const int32_t* cell_k1, const int32_t* cell_k2,
                       const nra_scoring_t* sc, int32_t flags, nra_batch_t** out)
{
    if (!out) return fail(NRA_E_ARG, "out is NULL");
    *out = nullptr;
    if (n_cells < 0) return fail(NRA_E_ARG, "bad region / counts");
    if (n_cells > 0 && (!cell_read || !cell_k1 || !cell_k2)) return fail(NRA_E_ARG, "NULL cell array");
    nra_batch_t* b = nullptr;
    int rc = nra_batch2d_create_reads(device, reg, n_reads, seqs, seq_off, sc, flags, &b);
    if (rc) return rc;
    rc = nra_batch2d_set_cells(b, read_strand, n_cells, cell_read, cell_k1, cell_k2);
    if (rc) { nra_batch_destroy(b); return rc; }
    *out = b;
    return NRA_OK;
}

}  // extern "C"

namespace {

// The kernels of a 2D run come in two parts.  Part 1 -- strand probes, strand choice, and per bucket the packed
// sweeps of the flanks outside the scoring window and the reverse sweeps over R -- depends on the reads and their
// strands only; nra_batch2d_set_cells / _set_grid enqueue it themselves when every strand is given, before they
// build the rest of the cell list's tasks.  Part 2 -- prefix sweeps, tail sweeps, per-cell payload launches,
// the selector -- is enqueued by nra_batch_run.
int run_2d_flanks(nra_batch* b)
{
    hipStream_t st = b->stream;
    const NraSeqArgs seq = seq_args(b);
    const size_t nb = b->buckets.size();
    const size_t nr = std::max<size_t>((size_t)b->n_reads, 1);
    int ev = 2;
    const bool warm = b->warm_pending;           // flank sweeps of this run went out ahead of the cell list: the run began there
    if (warm) {
        // a bucket's two chains wait for the sweeps of its own rows-per-lane class only (the R side's for the reverse
        // chain, the L side's for the prefix chain): the classes overlap as they do within one run
        ev = b->ev_next;
        for (size_t i = 0; i < nb; ++i)
            for (size_t w = 0; w < b->warm_R.size(); ++w)
                if (b->warm_R[w] == b->buckets[i].R && !b->buckets[i].chain) {
                    HIP_TRY(hipStreamWaitEvent(b->bstreams[2 * i], b->warm_ev[2 * w], 0));
                    HIP_TRY(hipStreamWaitEvent(b->bstreams[2 * i + 1], b->warm_ev[2 * w + 1], 0));
                }
        b->warm_pending = false;
    } else {
        HIP_TRY(hipEventRecord(b->ev[0], st));
        b->n_score_ev = 0;
    }
    b->n_ext_ev = 0;
    HIP_TRY(hipMemcpyAsync(b->reads.p, b->reads_init.p, nr * sizeof(NraDevRead), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(b->probe_score.p, 0xff, 2 * nr * 4, st));
    if (!b->all_strands_given) {
        HIP_TRY(hipEventRecord(b->fork_ev, st));
        for (size_t i = 0; i < nb; ++i) {
            const Bucket& bk = b->buckets[i];
            hipStream_t q = b->bstreams[2 * i];
            HIP_TRY(hipStreamWaitEvent(q, b->fork_ev, 0));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            if (bk.chain) {
                NraSeqArgs raw = seq;
                raw.sp.min_score = 0;            // the probe compares raw scores
                LAUNCH_TRY(nra_launch_payload_origin(bk.R, b->has_n, q, std::min(bk.n_probe, b->payload_strips),
                                                     b->probe_tasks.p + bk.probe_off, b->probe_count.p + i,
                                                     raw, b->probe_score.p, b->probe_dummy.p, nullptr,
                                                     b->chain_payload.p, b->chain_cap, 1));
            } else
            LAUNCH_TRY(nra_launch_score_pk16(bk.R, b->has_n, q, bk.n_pair, b->pair_tasks.p + bk.pair_off, seq, b->probe_score.p));
            HIP_TRY(hipEventRecord(b->ev[ev++], q));
            b->n_ext_ev++;
            HIP_TRY(hipEventRecord(b->bdone[3 * i + 2], q));
            HIP_TRY(hipStreamWaitEvent(st, b->bdone[3 * i + 2], 0));
        }
    }
    LAUNCH_TRY(nra_launch_pick_strand(st, b->n_reads, b->probe_score.p,
                                      b->have_strand_in ? b->strand_in.p : nullptr, b->strand_out.p, b->reads.p));
    if (!warm) HIP_TRY(hipEventRecord(b->phase_ev[0], st));
    if (!b->brute) {
        // reverse sweeps over R (one per read) and the packed sweeps of both flanks (one per pair of reads)
        HIP_TRY(hipEventRecord(b->fork2_ev, st));
        for (size_t i = 0; i < nb; ++i) {
            const Bucket& bk = b->buckets[i];
            if (bk.chain) continue;
            hipStream_t qa = b->bstreams[2 * i], qb = b->bstreams[2 * i + 1];
            HIP_TRY(hipStreamWaitEvent(qa, b->fork2_ev, 0));
            HIP_TRY(hipStreamWaitEvent(qb, b->fork2_ev, 0));
            // the L side first: the older kernel's waves issue first, and the chain behind it (prefix sweep, MID scans,
            // combine) is the longer one (config 3: 7.3 -> 7.1 ms of device time against the R side first)
            if (bk.n_jlpk > 0) {
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                LAUNCH_TRY(nra_launch_joint_pk16(bk.R, b->has_n, qb, bk.n_jlpk, b->jlpk_tasks.p + bk.jlpk_off, seq, 1, b->jlstate.p, nullptr));
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                b->n_score_ev++;
            }
            if (bk.n_jrpk > 0) {
                HIP_TRY(hipEventRecord(b->ev[ev++], qa));
                LAUNCH_TRY(nra_launch_joint_pk16(bk.R, b->has_n, qa, bk.n_jrpk, b->jrpk_tasks.p + bk.jrpk_off, seq, 0, b->jrstate.p, nullptr));
                HIP_TRY(hipEventRecord(b->ev[ev++], qa));
                b->n_score_ev++;
            }
            HIP_TRY(hipEventRecord(b->ev[ev++], qa));
            if (b->joint_v2)
                LAUNCH_TRY(nra_launch_joint_bwd_ext(bk.R, b->has_n, qa, bk.n_jbwd, b->jbwd_tasks.p + bk.jbwd_off, seq, b->jrs.p, b->jra.p,
                                                    b->jrstate.p));
            else
            LAUNCH_TRY(nra_launch_joint_bwd(bk.R, b->has_n, qa, bk.n_jbwd, b->jbwd_tasks.p + bk.jbwd_off, seq, b->jsnap.p, b->jread_a.p,
                                            b->jrstate.p));
            HIP_TRY(hipEventRecord(b->ev[ev++], qa));
            b->n_score_ev++;
            HIP_TRY(hipEventRecord(b->bdone[3 * i], qa));
        }
    }
    b->ev_next = ev;
    b->flanks_enqueued = true;
    return NRA_OK;
}

int run_2d(nra_batch* b)
{
    if (!b->flanks_enqueued) {
        const int rc = run_2d_flanks(b);
        if (rc) return rc;
    }
    b->flanks_enqueued = false;          // (a second nra_batch_run of the same cell list starts over)
    hipStream_t st = b->stream;
    const NraSeqArgs seq = seq_args(b);
    const size_t nb = b->buckets.size();
    const size_t nc = std::max<size_t>((size_t)b->n_cands, 1);
    int ev = b->ev_next;
    const int max_waves = 256 * 16;
    if (b->cells_need_clear) {
        HIP_TRY(hipMemsetAsync(b->cand_score.p, 0xff, nc * 4, st));
        HIP_TRY(hipMemsetAsync(b->cand_tstart.p, 0, nc * 4, st));
        HIP_TRY(hipEventRecord(b->fork_ev, st));           // the cell arrays are cleared (the tails write them)
    }
    // buckets scored cell by cell: all of them in brute-force mode, else the chained (long) reads only
    for (size_t i = 0; i < nb; ++i) {
        const Bucket& bk = b->buckets[i];
        if (!b->brute && !bk.chain) continue;
        HIP_TRY(hipEventRecord(b->ev[ev++], st));
        LAUNCH_TRY(nra_launch_payload_window(bk.R, b->has_n, st, std::min(bk.n_queue, bk.chain ? b->payload_strips : max_waves),
                                          b->queue_tasks.p + bk.queue_off, b->queue_count.p + i, seq, b->cand_score.p,
                                          b->cand_tstart.p, nullptr, bk.chain ? b->chain_payload.p : nullptr,
                                          bk.chain ? b->chain_cap : 0, bk.chain ? 1 : 0));
        HIP_TRY(hipEventRecord(b->ev[ev++], st));
        b->n_score_ev++;
    }
    if (!b->brute) {
        // group by group, the prefix sweeps (one per read) that leave the wave states and the tail sweeps (one
        // per (read, k1) run of cells) that resume from them
        for (size_t i = 0; i < nb; ++i) {
            const Bucket& bk = b->buckets[i];
            if (bk.chain) continue;
            hipStream_t qb = b->bstreams[2 * i + 1];
            HIP_TRY(hipStreamWaitEvent(st, b->bdone[3 * i], 0));
            if (b->cells_need_clear) HIP_TRY(hipStreamWaitEvent(qb, b->fork_ev, 0));
            bool first = true;
            for (const JointGroup& g : b->jgroups) {
                if (g.bucket != (int)i) continue;
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                if (b->joint_chain)
                    LAUNCH_TRY(nra_launch_joint_prefix_cols(g.R, b->has_n, qb, g.n_pre, b->jpre_tasks.p + g.pre_off, seq, b->jk1list.p,
                                                            b->jstate.p, b->jlstate.p));
                else
                LAUNCH_TRY(nra_launch_joint_prefix(g.R, b->has_n, qb, g.n_pre, b->jpre_tasks.p + g.pre_off, seq, b->jk1list.p,
                                                   b->jstate.p, b->jlstate.p));
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                b->n_score_ev++;
                if (first && !b->joint_v2) HIP_TRY(hipStreamWaitEvent(qb, b->bdone[3 * i], 0));     // the tails read the R side
                first = false;
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                if (b->joint_chain)
                    LAUNCH_TRY(nra_launch_joint_midscan(g.R, b->has_n, qb, g.n_tail, b->jtail_tasks.p + g.tail_off, seq, b->jk1list.p,
                                                         b->jstate.p, b->jfs.p, b->jfb.p, nullptr));
                else if (b->joint_v2)
                    LAUNCH_TRY(nra_launch_joint_mid(g.R, b->has_n, qb, g.n_tail, b->jtail_tasks.p + g.tail_off, seq, b->jstate.p,
                                                    b->jfs.p, b->jfb.p));
                else
                LAUNCH_TRY(nra_launch_joint_tail(g.R, b->has_n, qb, g.n_tail, b->jtail_tasks.p + g.tail_off, seq, b->jstate.p,
                                                 b->jsnap.p, b->jread_a.p, b->cand_score.p, b->cand_tstart.p));
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                b->n_score_ev++;
            }
            if (b->joint_v2 && bk.n_comb > 0) {
                // every cell of the bucket's reads from the column states on either side of the junction
                HIP_TRY(hipStreamWaitEvent(qb, b->bdone[3 * i], 0));                // ... the extended reverse sweeps'
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                LAUNCH_TRY(nra_launch_joint_combine(qb, bk.n_comb, b->jcomb_tasks.p + bk.comb_off, b->reads.p, b->sp,
                                                    b->jfs.p, b->jrs.p, b->jfb.p, b->jra.p, b->cand_score.p, b->cand_tstart.p, nullptr));
                HIP_TRY(hipEventRecord(b->ev[ev++], qb));
                b->n_score_ev++;
            }
            HIP_TRY(hipEventRecord(b->bdone[3 * i + 1], qb));
            HIP_TRY(hipStreamWaitEvent(st, b->bdone[3 * i + 1], 0));
        }
    }
    // the reverse sweeps enqueued above stay valid for later cell lists of this batch (given strands only:
    // a probed strand is not known on the host)
    commit_2d(b->carried, b->pending);
    HIP_TRY(hipEventRecord(b->phase_ev[1], st));
    LAUNCH_TRY(nra_launch_select_2d(st, b->n_reads, b->cell_first.p, b->cell_cnt.p, b->cell_k1.p, b->cell_k2.p,
                                    b->grid_step1 > 0 ? b->grid_rows.p : nullptr, b->grid_step1, b->grid_step2,
                                    b->cand_score.p, b->cand_tstart.p, b->best_score.p, b->sum_k.p,
                                    b->sum_k2.p, b->n_ties.p, b->status.p));
    HIP_TRY(hipEventRecord(b->ev[1], st));
    b->ev_next = ev;
    b->refined = false; b->refine_read = false; b->refine_bad_rows = 0;
    return NRA_OK;
}

// the counters a refinement left on the device (after its stream is idle): cells scored, rows that were not routable
int finish_refine(nra_batch* b)
{
    if (!b->refined || b->refine_read) return NRA_OK;
    int64_t w[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(w, b->rf_words.p, sizeof(w), hipMemcpyDeviceToHost));
    b->stats.n_alignments += w[0];
    b->stats.executed_cells += w[2];
    b->stats.algorithmic_cells += w[3];
    b->refine_bad_rows = w[1];
    b->refine_read = true;
    return NRA_OK;
}

}  // namespace

extern "C" {

// The reference's round 3 (nanoRepeat_joint.py:275-349) as a refinement of the routed grid whose run has just been
// enqueued: routed on the device from that grid's per-read results, scored from the column states its sweeps kept.
int nra_batch2d_refine(nra_batch_t* b, int32_t buf1, int32_t buf2, const double* lo1, const double* hi1,
                       const double* lo2, const double* hi2)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    if (buf1 <= 0 || buf2 <= 0 || buf1 > 4096 || buf2 > 4096) return fail(NRA_E_ARG, "bad refinement buffers");
    const int32_t n_reads = b->n_reads;
    if (n_reads > 0 && (!lo1 || !hi1 || !lo2 || !hi2)) return fail(NRA_E_ARG, "NULL bound array");
    {
        const Forms2D forms{b->joint_keep, b->brute, b->joint_v2, b->joint_chain, b->all_strands_given};
        const int rc = check_2d_refine(b->ran && !b->accounted && !b->refined, forms, b->carried, b->buckets, n_reads, buf1, buf2,
                                       lo1, hi1, lo2, hi2);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(b->device));
    ArenaScope arena_scope(&b->cell_arena);
    const int cap1 = 2 * buf1, cap2 = 2 * buf2;
    const int64_t cap = (int64_t)cap1 * cap2;
    if (!cells_2d_countable(cap * n_reads)) return fail(NRA_E_RANGE, "too many cells");
    const size_t nb = b->buckets.size();
    RefinePlan rp;
    {
        const int rc = plan_2d_refine(b->host_reads, b->r2, b->carried, b->buckets, buf1, buf2, rp);
        if (rc) return rc;
    }
    std::vector<double> bounds((size_t)4 * (size_t)std::max(n_reads, 1), 0.0);
    for (int32_t r = 0; r < n_reads; ++r) {
        bounds[(size_t)r] = lo1[r]; bounds[(size_t)n_reads + r] = hi1[r];
        bounds[(size_t)2 * n_reads + r] = lo2[r]; bounds[(size_t)3 * n_reads + r] = hi2[r];
    }
    b->cell_arena.expect(refine_arena_bytes(rp.fs_total, cap, n_reads));
    HIP_TRY(b->rf_bounds.upload(bounds));
    HIP_TRY(b->rf_keep.upload(b->carried.keep_rows));
    HIP_TRY(b->rf_first.upload(rp.first));
    HIP_TRY(b->rf_rowspad.upload(rp.rowspad));
    HIP_TRY(b->rf_mid_tasks.upload(rp.mid));
    HIP_TRY(b->rf_comb_tasks.upload(rp.comb));
    HIP_TRY(b->rf_rows.alloc((size_t)std::max(n_reads, 1)));
    HIP_TRY(b->rf_cnt.alloc((size_t)std::max(n_reads, 1)));
    HIP_TRY(b->rf_words.alloc(4));
    HIP_TRY(b->rf_fs.alloc((size_t)rp.fs_total));
    HIP_TRY(b->rf_fb.alloc((size_t)rp.fb_total));
    // the refinement's cells: read-major, `cap` entries a read (its n1 x n2 cells first, k1-major)
    HIP_TRY(b->rf_cell_score.alloc((size_t)(cap * n_reads)));
    HIP_TRY(b->rf_cell_wscore.alloc((size_t)(cap * n_reads)));
    b->rf_n_cands = cap * n_reads;
    {
        const size_t need = (size_t)b->ev_next + 4 * nb + 4;
        while (b->ev.size() < need) { hipEvent_t e; HIP_TRY(g_handles.event(b->device, true, &e)); b->ev.push_back(e); }
    }

    hipStream_t st = b->stream;
    const NraSeqArgs seq = seq_args(b);
    int ev = b->ev_next;
    const size_t nc = (size_t)std::max<int64_t>(cap * n_reads, 1);
    HIP_TRY(hipMemsetAsync(b->rf_words.p, 0, 4 * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(b->rf_cell_score.p, 0xff, nc * 4, st));
    HIP_TRY(hipMemsetAsync(b->rf_cell_wscore.p, 0, nc * 4, st));
    const double* bd = b->rf_bounds.p;
    LAUNCH_TRY(nra_launch_joint_refine_route(st, n_reads, b->status.p, b->n_ties.p, b->sum_k.p, b->sum_k2.p, bd, bd + n_reads,
                                             bd + 2 * (size_t)n_reads, bd + 3 * (size_t)n_reads, buf1, buf2, b->rf_keep.p,
                                             b->rf_rows.p, b->rf_cnt.p, b->rf_rowspad.p, b->reads.p, b->regions.p,
                                             reinterpret_cast<unsigned long long*>(b->rf_words.p)));
    HIP_TRY(hipEventRecord(b->fork2_ev, st));
    for (size_t i = 0; i < nb; ++i) {
        const Bucket& bk = b->buckets[i];
        const int n_mid = (int)(rp.mid_off[i + 1] - rp.mid_off[i]), n_comb = (int)(rp.comb_off[i + 1] - rp.comb_off[i]);
        if (n_mid == 0) continue;
        hipStream_t qb = b->bstreams[2 * i + 1];
        HIP_TRY(hipStreamWaitEvent(qb, b->fork2_ev, 0));
        HIP_TRY(hipEventRecord(b->ev[ev++], qb));
        LAUNCH_TRY(nra_launch_joint_midscan(bk.R, b->has_n, qb, n_mid, b->rf_mid_tasks.p + rp.mid_off[i], seq, nullptr, b->jstate.p,
                                            b->rf_fs.p, b->rf_fb.p, b->rf_rows.p));
        HIP_TRY(hipEventRecord(b->ev[ev++], qb));
        b->n_score_ev++;
        HIP_TRY(hipEventRecord(b->ev[ev++], qb));
        LAUNCH_TRY(nra_launch_joint_combine(qb, n_comb, b->rf_comb_tasks.p + rp.comb_off[i], b->reads.p, b->sp, b->rf_fs.p, b->jrs.p,
                                            b->rf_fb.p, b->jra.p, b->rf_cell_score.p, b->rf_cell_wscore.p, b->rf_rows.p));
        HIP_TRY(hipEventRecord(b->ev[ev++], qb));
        b->n_score_ev++;
        HIP_TRY(hipEventRecord(b->bdone[3 * i + 1], qb));
        HIP_TRY(hipStreamWaitEvent(st, b->bdone[3 * i + 1], 0));
    }
    HIP_TRY(hipEventRecord(b->phase_ev[1], st));
    LAUNCH_TRY(nra_launch_select_2d(st, n_reads, b->rf_first.p, b->rf_cnt.p, nullptr, nullptr, b->rf_rows.p, 1, 1,
                                    b->rf_cell_score.p, b->rf_cell_wscore.p, b->best_score.p, b->sum_k.p, b->sum_k2.p, b->n_ties.p,
                                    b->status.p));
    HIP_TRY(hipEventRecord(b->ev[1], st));
    b->ev_next = ev;
    b->refined = true; b->refine_read = false;
    return NRA_OK;
}
int64_t nra_plan2d_digest(const nra_joint_region_t* reg, int32_t n_reads, const char* seqs, const int64_t* seq_off,
                          const nra_scoring_t* sc, int32_t flags, const nra_plan2d_step_t* steps, int32_t n_steps,
                          char* buf, int64_t cap)
{
    if (!reg || n_reads < 0 || n_steps < 0 || (n_steps > 0 && !steps)) return fail(NRA_E_ARG, "bad region / counts");
    if (n_reads > 0 && (!seqs || !seq_off)) return fail(NRA_E_ARG, "NULL input array");
    if (!scoring_ok(sc)) return fail(NRA_E_ARG, "scoring parameters out of range");
    if (reg->left_len < 0 || reg->right_len < 0 || reg->mid_len < 0 || reg->unit1_len <= 0 ||
        reg->unit2_len <= 0 || !reg->unit1 || !reg->unit2)
        return fail(NRA_E_ARG, "bad joint region");
    if (cap < 0 || (cap > 0 && !buf)) return fail(NRA_E_ARG, "bad buffer");
    PackedReads pr;
    const int rc = pack_reads(n_reads, seqs, seq_off, nullptr, 1, pr, NRA_MAX_QLEN);
    if (rc) return rc;
    const std::string text = plan_2d_digest(reg, pr.reads, pr.has_n, pr.q2bit.size(), sc, flags, steps, n_steps);
    if (cap > 0) {
        const size_t n = std::min(text.size(), (size_t)cap - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size() + 1;
}

int nra_batch2d_fetch(nra_batch_t* b, int8_t* read_strand, int32_t* cell_score, int32_t* cell_wscore,
                      int32_t* best_wscore, int64_t* sum_k1, int64_t* sum_k2, int32_t* n_ties, uint8_t* status)
{
    if (!b || b->kind != 2) return fail(NRA_E_ARG, "not a 2D batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    {
        int rc = finish_refine(b);
        if (rc) return rc;
        if (b->refine_bad_rows > 0)
            return fail(NRA_E_RANGE, std::to_string(b->refine_bad_rows) + " reads of the refinement ask for repeat counts outside the "
                                     "kept column states (bounds other than the grid's?)");
    }
    // (after a refinement the per-cell arrays are the refinement's: (2 buf1)(2 buf2) entries a read)
    const size_t n = (size_t)b->n_reads, nc = (size_t)(b->refined ? b->rf_n_cands : b->n_cands);
    const int32_t* src_score = b->refined ? b->rf_cell_score.p : b->cand_score.p;
    const int32_t* src_wscore = b->refined ? b->rf_cell_wscore.p : b->cand_tstart.p;
    if (n) {
        int rc = fetch_results(b);
        if (rc) return rc;
        if (read_strand) memcpy(read_strand, staged(b, b->strand_out), n);
        if (best_wscore) memcpy(best_wscore, staged(b, b->best_score), n * 4);
        if (sum_k1) memcpy(sum_k1, staged(b, b->sum_k), n * 8);
        if (sum_k2) memcpy(sum_k2, staged(b, b->sum_k2), n * 8);
        if (n_ties) memcpy(n_ties, staged(b, b->n_ties), n * 4);
        if (status) memcpy(status, staged(b, b->status), n);
    }
    if (nc) {
        if (cell_score) HIP_TRY(copy_d2h(cell_score, src_score, nc * 4));
        if (cell_wscore) HIP_TRY(copy_d2h(cell_wscore, src_wscore, nc * 4));
    }
    return NRA_OK;
}

int nra_joint_2d(int device, const nra_joint_region_t* region, int32_t n_reads, const char* seqs,
                 const int64_t* seq_off, int8_t* read_strand, int64_t n_cells, const int32_t* cell_read,
                 const int32_t* cell_k1, const int32_t* cell_k2, const nra_scoring_t* sc, int32_t flags,
                 int32_t* cell_score, int32_t* cell_wscore, int32_t* best_wscore, int64_t* sum_k1,
                 int64_t* sum_k2, int32_t* n_ties, uint8_t* status)
{
    if (n_reads > 0 && (!best_wscore || !sum_k1 || !sum_k2 || !n_ties || !status)) return fail(NRA_E_ARG, "NULL output array");
    nra_batch_t* b = nullptr;
    int rc = nra_batch2d_create(device, region, n_reads, seqs, seq_off, read_strand, n_cells, cell_read,
                                cell_k1, cell_k2, sc, flags, &b);
    if (rc) return rc;
    rc = nra_batch_run(b);
    if (!rc) rc = nra_batch_sync(b);
    if (!rc) rc = nra_batch2d_fetch(b, read_strand, cell_score, cell_wscore, best_wscore, sum_k1, sum_k2, n_ties, status);
    nra_batch_destroy(b);
    return rc;
}

// ---- generic pairs --------------------------------------------------------------------
namespace {

struct PairSetup {
    std::vector<uint8_t> pool;
    std::vector<NraDevRegion> dregs;
    std::vector<NraDevRead> dreads;
    std::vector<uint32_t> q2bit, nmask;
    std::vector<int32_t> as_query, as_target;   // sequence -> read / region index
    bool has_n = false;
};

int prepare_pairs(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, int64_t n_pairs,
                  const int32_t* pair_query, const int32_t* pair_target, const nra_scoring_t* sc, PairSetup& ps,
                  int64_t max_query, int64_t max_target, int64_t max_query_score)
{
    if (n_seqs < 0 || n_pairs < 0) return fail(NRA_E_ARG, "negative count");
    if (n_seqs > 0 && (!seqs || !seq_off)) return fail(NRA_E_ARG, "NULL sequence array");
    if (n_pairs > 0 && (!pair_query || !pair_target)) return fail(NRA_E_ARG, "NULL pair array");
    if (n_pairs > 0x7ff00000ll) return fail(NRA_E_RANGE, "too many pairs");
    if (!scoring_ok(sc)) return fail(NRA_E_ARG, "scoring parameters out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    // which sequences are queries (2-bit pool, one register block) / targets (byte pool, <= 65000)
    ps.as_query.assign((size_t)n_seqs, -1); ps.as_target.assign((size_t)n_seqs, -1);
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t q = pair_query[i], t = pair_target[i];
        if (q < 0 || q >= n_seqs || t < 0 || t >= n_seqs) return fail(NRA_E_ARG, "pair index out of range");
        ps.as_query[q] = 0; ps.as_target[t] = 0;
    }
    uint64_t base = 0;
    for (int32_t s = 0; s < n_seqs; ++s) {
        const int64_t len = seq_off[s + 1] - seq_off[s];
        if (len < 0) return fail(NRA_E_ARG, "seq_off must be non-decreasing");
        if (ps.as_target[s] == 0) {
            if (len > max_target) return fail(NRA_E_RANGE, "target longer than " + std::to_string(max_target));
            NraDevRegion d{};
            d.p1_off = pool_append(ps.pool, seqs + seq_off[s], (int32_t)len, nullptr, 0, 0, ps.has_n);
            d.p2_off = d.p3_off = d.pr_off = (uint32_t)ps.pool.size();
            d.l1 = (int32_t)len; d.m1 = 0; d.l2 = 0; d.m2 = 0; d.l3 = 0;
            ps.as_target[s] = (int32_t)ps.dregs.size();
            ps.dregs.push_back(d);
            if (ps.pool.size() > 0xfff00000ull) return fail(NRA_E_RANGE, "target pool exceeds 4 GB");
        }
        if (ps.as_query[s] == 0) {
            if (len > max_query) return fail(NRA_E_RANGE, "query longer than " + std::to_string(max_query));
            if (max_score(sc, len) > max_query_score)
                return fail(NRA_E_RANGE, "query " + std::to_string(s) + ": match score x length does not fit 16 bits");
            NraDevRead r{};
            r.qoff = (uint32_t)base; r.qlen = (int32_t)len; r.region = 0; r.rc = 0;
            ps.as_query[s] = (int32_t)ps.dreads.size();
            ps.dreads.push_back(r);
            base += ((uint64_t)len + 31) / 32 * 32;
            if (base > 0xfff00000ull) return fail(NRA_E_RANGE, "query pool exceeds 4G bases");
        }
    }
    ps.pool.push_back(0);
    ps.q2bit.assign((size_t)(base / 16) + 1, 0);
    ps.nmask.assign((size_t)(base / 32) + 1, 0);
    for (int32_t s = 0; s < n_seqs; ++s) {
        if (ps.as_query[s] < 0) continue;
        const NraDevRead& r = ps.dreads[ps.as_query[s]];
        const char* p = seqs + seq_off[s];
        for (int32_t i = 0; i < r.qlen; ++i) {
            uint8_t c = encode_base(p[i]);
            const uint32_t b = r.qoff + (uint32_t)i;
            if (c >= 4) { ps.nmask[b >> 5] |= 1u << (b & 31); ps.has_n = true; c = 0; }
            ps.q2bit[b >> 4] |= (uint32_t)c << ((b & 15) * 2);
        }
    }
    return NRA_OK;
}

}  // namespace

int nra_align_pairs(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, int64_t n_pairs,
                    const int32_t* pair_query, const int32_t* pair_target, const nra_scoring_t* sc,
                    int32_t flags, int32_t* score, int32_t* tstart, int32_t* tend)
{
    (void)flags;
    if (n_pairs > 0 && (!score || !tstart || !tend)) return fail(NRA_E_ARG, "NULL output array");
    PairSetup ps;
    int rc = prepare_pairs(device, n_seqs, seqs, seq_off, n_pairs, pair_query, pair_target, sc, ps, NRA_MAX_QLEN,
                           NRA_MAX_TLEN_WIDE, (int64_t)1 << 30);
    if (rc || n_pairs == 0) return rc;
    // Launch groups: int32 cells (score < 32768, target <= 65000 columns) in the rows-per-lane bucket of the
    // query, or -- queries longer than one register block -- chained row blocks; everything beyond that
    // (a long core's score, a whole long read as the target) in int64 cells, three row counts.
    struct Group { int R; bool chain, wide; std::vector<NraTask> tasks; };
    std::vector<Group> groups;
    auto group_of = [&](int R, bool chain, bool wide) -> Group& {
        for (Group& g : groups) if (g.R == R && g.chain == chain && g.wide == wide) return g;
        groups.push_back(Group{R, chain, wide, {}});
        return groups.back();
    };
    int chain_cols = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t qi = ps.as_query[pair_query[i]];
        const int32_t ti = ps.as_target[pair_target[i]];
        const int qlen = ps.dreads[qi].qlen, tlen = ps.dregs[ti].l1;
        if (qlen == 0) continue;
        const bool wide = tlen > NRA_MAX_TLEN || max_score(sc, qlen) > kScoreCapI32;
        const bool chain = qlen > NRA_MAX_QLEN_1BLOCK;
        if (chain) chain_cols = std::max(chain_cols, tlen);
        const int R = chain ? NRA_CHAIN_R
                            : wide ? (qlen <= 64 * NRA_WIDE_R_SMALL ? NRA_WIDE_R_SMALL : NRA_WIDE_R_LARGE)
                                   : kRList[rows_for_qlen(qlen)];
        group_of(R, chain, wide).tasks.push_back(NraTask{qi, ti, -1, (int32_t)i});
    }
    std::sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) {      // longest first
        return (int64_t)a.R * (a.chain ? 1000 : 1) > (int64_t)b.R * (b.chain ? 1000 : 1);
    });
    const int chain_cap = (chain_cols + 127) / 64 * 64 + 64;
    std::vector<NraTask> tasks;
    std::vector<int32_t> counts;
    std::vector<size_t> offs;
    bool any_chain = false;
    for (const Group& g : groups) {
        offs.push_back(tasks.size());
        counts.push_back((int32_t)g.tasks.size());
        tasks.insert(tasks.end(), g.tasks.begin(), g.tasks.end());
        any_chain |= g.chain;
    }
    Arena arena;                       // before the buffers: released after them
    arena.device = device;
    ArenaScope arena_scope(&arena);
    arena.expect(ps.pool.size() + ps.q2bit.size() * 6 + (size_t)n_pairs * 32 + (2u << 20));
    DevBuf<uint8_t> d_pool; DevBuf<uint32_t> d_q2, d_nm; DevBuf<NraDevRegion> d_regs; DevBuf<NraDevRead> d_reads;
    DevBuf<NraTask> d_tasks; DevBuf<int32_t> d_counts, d_score, d_ts, d_te; DevBuf<int64_t> d_chain;
    HIP_TRY(d_pool.upload(ps.pool)); HIP_TRY(d_q2.upload(ps.q2bit)); HIP_TRY(d_nm.upload(ps.nmask));
    HIP_TRY(d_regs.upload(ps.dregs)); HIP_TRY(d_reads.upload(ps.dreads)); HIP_TRY(d_tasks.upload(tasks));
    HIP_TRY(d_counts.upload(counts));
    HIP_TRY(d_score.alloc((size_t)n_pairs)); HIP_TRY(d_ts.alloc((size_t)n_pairs)); HIP_TRY(d_te.alloc((size_t)n_pairs));
    size_t chain_tasks = 0;
    for (size_t i = 0; i < groups.size(); ++i) if (groups[i].chain) chain_tasks = std::max(chain_tasks, groups[i].tasks.size());
    const int pair_strips = chain_strips(chain_tasks, NRA_CHAIN_STRIPS, (size_t)6 * 8 * (size_t)chain_cap);
    if (any_chain) HIP_TRY(d_chain.alloc((size_t)pair_strips * 6 * (size_t)chain_cap));
    HIP_TRY(hipMemset(d_score.p, 0xff, (size_t)n_pairs * 4));
    HIP_TRY(hipMemset(d_ts.p, 0xff, (size_t)n_pairs * 4));
    HIP_TRY(hipMemset(d_te.p, 0xff, (size_t)n_pairs * 4));
    const NraSeqArgs seq{d_reads.p, d_regs.p, d_pool.p, d_q2.p, d_nm.p, to_params(*sc)};     // this call's own buffers
    for (size_t i = 0; i < groups.size(); ++i) {
        const Group& g = groups[i];
        LAUNCH_TRY(nra_launch_payload_origin(g.R, ps.has_n ? 1 : 0, nullptr,
                                             std::min(counts[i], g.chain ? pair_strips : 256 * 16),
                                             d_tasks.p + offs[i], d_counts.p + i, seq, d_score.p, d_ts.p, d_te.p,
                                             g.chain ? d_chain.p : nullptr, g.chain ? chain_cap : 0, g.wide ? 1 : 0));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(copy_d2h(score, d_score.p, (size_t)n_pairs * 4));
    HIP_TRY(copy_d2h(tstart, d_ts.p, (size_t)n_pairs * 4));
    HIP_TRY(copy_d2h(tend, d_te.p, (size_t)n_pairs * 4));
    return NRA_OK;
}

namespace {

// nra_align_pairs_cigar and nra_align_paths: the trace of every pair, its best cell, the walk back and the CIGAR.
// paths = false: queries of one register block in int32 cells, a launch per rows-per-lane bucket (k_trace_fill).
// paths = true: those pairs the same way; a query beyond one register block, or a pair whose score outgrows the
// int32 cell, in row blocks of block_r rows per lane (k_trace_fill_mt), and with force_blocks every pair so.
int align_cigar_pairs(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, int64_t n_pairs,
                      const int32_t* pair_query, const int32_t* pair_target, const nra_scoring_t* sc, bool paths,
                      int block_r, bool force_blocks, int32_t* score, int32_t* tstart, int32_t* tend, int32_t* qstart,
                      int32_t* qend, char* cigar, int64_t cigar_cap, int64_t* cigar_off)
{
    if (n_pairs > 0 && (!score || !tstart || !tend || !qstart || !qend || !cigar || !cigar_off || cigar_cap < 1))
        return fail(NRA_E_ARG, "NULL output array");
    PairSetup ps;
    int rc = prepare_pairs(device, n_seqs, seqs, seq_off, n_pairs, pair_query, pair_target, sc, ps,
                           paths ? NRA_MAX_QLEN : NRA_MAX_QLEN_1BLOCK, NRA_MAX_TLEN,
                           paths ? (int64_t)1 << 40 : kScoreCapI32);
    if (rc) return rc;
    if (cigar_off) cigar_off[0] = 0;
    if (n_pairs == 0) return NRA_OK;

    // launch groups: row blocks in 64-bit cells, row blocks in int32 cells, then one per rows-per-lane bucket;
    // tasks keep their pair index through `order`
    std::vector<std::vector<int64_t>> by_bucket((size_t)kNumR);
    std::vector<int64_t> by_blocks[2];                 // [wide]
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t qi = ps.as_query[pair_query[i]];
        const int64_t ql = ps.dreads[qi].qlen, tl = ps.dregs[ps.as_target[pair_target[i]]].l1;
        if (ql == 0 || tl == 0) continue;
        const bool wide = paths && max_score(sc, std::min(ql, tl)) > kScoreCapI32;
        if (paths && (force_blocks || wide || ql > NRA_MAX_QLEN_1BLOCK)) by_blocks[wide ? 1 : 0].push_back(i);
        else by_bucket[rows_for_qlen((int)ql)].push_back(i);
    }
    struct Launch { int R; size_t off; int count; bool blocks, wide; size_t blk_off; int n_blocks; };
    std::vector<NraTraceTask> tasks;
    std::vector<int64_t> order;
    std::vector<Launch> launches;
    std::vector<NraTraceBlock> blocks;
    uint64_t trace_bytes = 0, ops_bytes = 0, strip_granules = 0;
    size_t n_blk_slots = 0;
    auto add_task = [&](int64_t i) {
        NraTraceTask t{};
        t.read = ps.as_query[pair_query[i]];
        t.region = ps.as_target[pair_target[i]];
        const uint64_t ql = (uint64_t)ps.dreads[t.read].qlen, tl = (uint64_t)ps.dregs[t.region].l1;
        t.ops_cap = (int32_t)(ql + tl);
        t.trace_off = trace_bytes; t.ops_off = ops_bytes;
        trace_bytes += ql * tl; ops_bytes += ql + tl;
        tasks.push_back(t); order.push_back(i);
    };
    const int block_rows = 64 * block_r;
    for (int w = 1; w >= 0; --w) {
        if (by_blocks[w].empty()) continue;
        Launch L{block_r, tasks.size(), (int)by_blocks[w].size(), true, w == 1, blocks.size(), 0};
        std::vector<uint64_t> strip0;                  // the strip under block 0 of each task of the launch
        int most = 0;
        for (int64_t i : by_blocks[w]) {
            add_task(i);
            NraTraceTask& t = tasks.back();
            const int nblk = (ps.dreads[t.read].qlen + block_rows - 1) / block_rows;
            t.blk0 = (int32_t)n_blk_slots;
            n_blk_slots += (size_t)nblk;
            strip0.push_back(strip_granules);
            strip_granules += (uint64_t)(nblk - 1) * (w ? 6 : 3) * (uint64_t)((ps.dregs[t.region].l1 + 63) & ~63);
            most = std::max(most, nblk);
        }
        // a producer precedes its consumer: the blocks 0 of every task, then the blocks 1, ...
        for (int b = 0; b < most; ++b)
            for (int k = 0; k < L.count; ++k) {
                const NraTraceTask& t = tasks[L.off + (size_t)k];
                const int nblk = (ps.dreads[t.read].qlen + block_rows - 1) / block_rows;
                if (b >= nblk) continue;
                const uint64_t per = (uint64_t)(w ? 6 : 3) * (uint64_t)((ps.dregs[t.region].l1 + 63) & ~63);
                NraTraceBlock nb{};
                nb.task = k; nb.blk = b; nb.nblk = nblk;
                nb.strip_in = b > 0 ? strip0[(size_t)k] + (uint64_t)(b - 1) * per : 0;
                nb.strip_out = b + 1 < nblk ? strip0[(size_t)k] + (uint64_t)b * per : 0;
                blocks.push_back(nb);
            }
        L.n_blocks = (int)(blocks.size() - L.blk_off);
        launches.push_back(L);
    }
    for (int bi = kNumR - 1; bi >= 0; --bi) {
        if (by_bucket[bi].empty()) continue;
        launches.push_back(Launch{kRList[bi], tasks.size(), (int)by_bucket[bi].size(), false, false, 0, 0});
        for (int64_t i : by_bucket[bi]) add_task(i);
    }
    if (trace_bytes > (8ull << 30)) return fail(NRA_E_RANGE, "trace needs more than 8 GiB: split the call");
    const size_t nt = tasks.size();
    Arena arena;                       // before the buffers: released after them
    arena.device = device;
    ArenaScope arena_scope(&arena);
    arena.expect(ps.pool.size() + ps.q2bit.size() * 6 + nt * 128 + (size_t)ops_bytes + blocks.size() * 48 + (2u << 20));
    DevBuf<uint8_t> d_pool, d_trace, d_ops; DevBuf<uint32_t> d_q2, d_nm; DevBuf<NraDevRegion> d_regs;
    DevBuf<NraDevRead> d_reads; DevBuf<NraTraceTask> d_tasks; DevBuf<int32_t> d_fill, d_back, d_best, d_words;
    DevBuf<NraTraceBlock> d_blocks; DevBuf<uint64_t> d_strips;
    HIP_TRY(d_pool.upload(ps.pool)); HIP_TRY(d_q2.upload(ps.q2bit)); HIP_TRY(d_nm.upload(ps.nmask));
    HIP_TRY(d_regs.upload(ps.dregs)); HIP_TRY(d_reads.upload(ps.dreads)); HIP_TRY(d_tasks.upload(tasks));
    HIP_TRY(d_trace.alloc((size_t)trace_bytes)); HIP_TRY(d_ops.alloc((size_t)ops_bytes));
    HIP_TRY(d_fill.alloc(nt * 5)); HIP_TRY(d_back.alloc(nt * 3));
    if (!blocks.empty()) {
        // words: a ticket per launch of row blocks, then the error word; the strips start without this call's epoch
        HIP_TRY(d_blocks.upload(blocks)); HIP_TRY(d_best.alloc(n_blk_slots * 4)); HIP_TRY(d_words.alloc(4));
        HIP_TRY(d_strips.alloc((size_t)strip_granules + 1));
        HIP_TRY(hipMemsetAsync(d_words.p, 0, 4 * sizeof(int32_t), nullptr));
        HIP_TRY(hipMemsetAsync(d_strips.p, 0, ((size_t)strip_granules + 1) * 8, nullptr));
    }
    const NraSeqArgs seq{d_reads.p, d_regs.p, d_pool.p, d_q2.p, d_nm.p, to_params(*sc)};     // this call's own buffers
    int n_block_launches = 0;
    for (const Launch& L : launches) {
        const size_t off = L.off;
        if (L.blocks) {
            LAUNCH_TRY(nra_launch_trace_fill_mt(L.R, ps.has_n ? 1 : 0, L.wide ? 1 : 0, nullptr, L.n_blocks,
                                                d_blocks.p + L.blk_off, d_words.p + n_block_launches, d_tasks.p + off, seq,
                                                d_trace.p, d_best.p, d_strips.p, 1u, d_words.p + 3));
            LAUNCH_TRY(nra_launch_trace_best(nullptr, L.count, d_tasks.p + off, d_reads.p, block_rows, L.wide ? 1 : 0,
                                             d_best.p, seq.sp, d_fill.p + off * 5));
            ++n_block_launches;
        } else {
            LAUNCH_TRY(nra_launch_trace_fill(L.R, ps.has_n ? 1 : 0, nullptr, L.count, d_tasks.p + off, seq, d_trace.p,
                                             d_fill.p + off * 5));
        }
        LAUNCH_TRY(nra_launch_trace_back(nullptr, L.count, d_tasks.p + off, d_reads.p, d_regs.p, d_trace.p,
                                         d_fill.p + off * 5, d_ops.p, d_back.p + off * 3));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (!blocks.empty()) {
        int32_t gave_up = 0;
        HIP_TRY(copy_d2h(&gave_up, d_words.p + 3, 4));
        if (gave_up) return fail(NRA_E_DEVICE, "trace fill: a row block waited too long for the block above it");
    }
    std::vector<int32_t> fill(nt * 5), back(nt * 3);
    std::vector<uint8_t> ops((size_t)ops_bytes);
    if (nt) {
        HIP_TRY(copy_d2h(fill.data(), d_fill.p, nt * 5 * 4));
        HIP_TRY(copy_d2h(back.data(), d_back.p, nt * 3 * 4));
        HIP_TRY(copy_d2h(ops.data(), d_ops.p, (size_t)ops_bytes));
    }
    // per pair: extents + run-length encoded CIGAR
    std::vector<std::string> cg((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) { score[i] = -1; tstart[i] = -1; tend[i] = -1; qstart[i] = -1; qend[i] = -1; }
    for (size_t t = 0; t < nt; ++t) {
        const int64_t i = order[t];
        const int32_t* f = &fill[t * 5];
        if (f[0] < 0) continue;
        score[i] = f[0]; tstart[i] = back[t * 3 + 2]; tend[i] = f[2]; qstart[i] = back[t * 3 + 1]; qend[i] = f[3] + 1;
        const int n = back[t * 3];
        const uint8_t* op = ops.data() + tasks[t].ops_off + tasks[t].ops_cap - n;
        std::string& out = cg[i];
        for (int k = 0; k < n;) {
            int e = k;
            while (e < n && op[e] == op[k]) ++e;
            out += std::to_string(e - k);
            out += (char)op[k];
            k = e;
        }
    }
    int64_t pos = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        cigar_off[i] = pos;
        if (pos + (int64_t)cg[i].size() + 1 > cigar_cap)
            return fail(NRA_E_ARG, "cigar buffer too small");
        memcpy(cigar + pos, cg[i].c_str(), cg[i].size() + 1);
        pos += (int64_t)cg[i].size() + 1;
    }
    cigar_off[n_pairs] = pos;
    return NRA_OK;
}

}  // namespace

int nra_align_pairs_cigar(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, int64_t n_pairs,
                          const int32_t* pair_query, const int32_t* pair_target, const nra_scoring_t* sc,
                          int32_t flags, int32_t* score, int32_t* tstart, int32_t* tend, int32_t* qstart,
                          int32_t* qend, char* cigar, int64_t cigar_cap, int64_t* cigar_off)
{
    (void)flags;
    return align_cigar_pairs(device, n_seqs, seqs, seq_off, n_pairs, pair_query, pair_target, sc, false, 0, false,
                             score, tstart, tend, qstart, qend, cigar, cigar_cap, cigar_off);
}

int nra_align_paths(int device, int32_t n_seqs, const char* seqs, const int64_t* seq_off, int64_t n_pairs,
                    const int32_t* pair_query, const int32_t* pair_target, const nra_scoring_t* sc,
                    int32_t flags, int32_t* score, int32_t* tstart, int32_t* tend, int32_t* qstart,
                    int32_t* qend, char* cigar, int64_t cigar_cap, int64_t* cigar_off)
{
    (void)flags;
    // the limits, before the device is touched
    if (n_seqs < 0 || n_pairs < 0) return fail(NRA_E_ARG, "negative count");
    if (n_seqs > 0 && (!seqs || !seq_off)) return fail(NRA_E_ARG, "NULL sequence array");
    if (n_pairs > 0 && (!pair_query || !pair_target)) return fail(NRA_E_ARG, "NULL pair array");
    uint64_t trace_bytes = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t q = pair_query[i], t = pair_target[i];
        if (q < 0 || q >= n_seqs || t < 0 || t >= n_seqs) return fail(NRA_E_ARG, "pair index out of range");
        const int64_t ql = seq_off[q + 1] - seq_off[q], tl = seq_off[t + 1] - seq_off[t];
        if (ql < 0 || tl < 0) return fail(NRA_E_ARG, "seq_off must be non-decreasing");
        if (ql > NRA_MAX_QLEN) return fail(NRA_E_RANGE, "query longer than " + std::to_string(NRA_MAX_QLEN));
        if (tl > NRA_MAX_TLEN) return fail(NRA_E_RANGE, "target longer than " + std::to_string(NRA_MAX_TLEN));
        trace_bytes += (uint64_t)ql * (uint64_t)tl;
        if (trace_bytes > (8ull << 30)) return fail(NRA_E_RANGE, "trace needs more than 8 GiB: split the call");
    }
    // NRA_TEST_TRACE_BLOCK_ROWS (tests): every pair in row blocks of so many rows, a height the kernel is built for
    int block_r = NRA_TRACE_CHAIN_R;
    bool force_blocks = false;
    if (const char* e = getenv("NRA_TEST_TRACE_BLOCK_ROWS")) {
        const int rows = atoi(e);
        bool built = false;
#define CASE(r) built = built || rows == 64 * (r);
        NRA_TRACE_MT_R_LIST(CASE)
#undef CASE
        if (!built) return fail(NRA_E_ARG, "NRA_TEST_TRACE_BLOCK_ROWS: 64 x one of 1, 2, 3, 4, 6, 8, 12, 16, 24");
        block_r = rows / 64;
        force_blocks = true;
    }
    return align_cigar_pairs(device, n_seqs, seqs, seq_off, n_pairs, pair_query, pair_target, sc, true, block_r,
                             force_blocks, score, tstart, tend, qstart, qend, cigar, cigar_cap, cigar_off);
}

// ---- common -------------------------------------------------------------------------
static int account_run(nra_batch* b);
namespace { int finish_refine(nra_batch* b); }

int nra_batch_run(nra_batch_t* b)
{
    if (!b) return fail(NRA_E_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    // the events are about to be re-recorded: a finished run nobody synchronised on is accounted first
    if (b->ran && !b->accounted) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        int rc0 = account_run(b);
        if (rc0) return rc0;
    }
    if (b->kind == 2 && !b->have_cells) return fail(NRA_E_ARG, "2D batch without a cell list: call nra_batch2d_set_cells");
    int rc = b->kind == 1 ? run_1d(b) : run_2d(b);
    if (!rc) { b->ran = true; b->accounted = false; }
    return rc;
}

// Reads the HIP events of the run that has just completed (the stream is idle) into the batch's
// statistics: the last run's timings and their sums over all runs, so that a caller timing many runs
// gets averages that belong to the same runs as its wall clock.
static int account_run(nra_batch* b)
{
    if (!b->ran || b->accounted) return NRA_OK;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
    b->stats.total_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, b->phase_ev[0], b->phase_ev[1]));
    b->stats.score_phase_ms = ms;
    // event pairs were recorded in launch order: 1D: score..., extents...; 2D: probe..., window...
    double first = 0, second = 0;
    const int n_first = b->kind == 1 ? b->n_score_ev : b->n_ext_ev;
    const int n_second = b->kind == 1 ? b->n_ext_ev : b->n_score_ev;
    int ev = 2;
    for (int i = 0; i < n_first; ++i, ev += 2) { HIP_TRY(hipEventElapsedTime(&ms, b->ev[ev], b->ev[ev + 1])); first += ms; }
    for (int i = 0; i < n_second; ++i, ev += 2) { HIP_TRY(hipEventElapsedTime(&ms, b->ev[ev], b->ev[ev + 1])); second += ms; }
    b->stats.score_kernel_ms = b->kind == 1 ? first : second;
    b->stats.extent_kernel_ms = b->kind == 1 ? second : first;
    b->stats.n_score_launches = b->n_score_ev;
    b->stats.n_runs += 1;
    b->stats.sum_score_kernel_ms += b->stats.score_kernel_ms;
    b->stats.sum_extent_kernel_ms += b->stats.extent_kernel_ms;
    b->stats.sum_total_ms += b->stats.total_ms;
    b->stats.sum_score_phase_ms += b->stats.score_phase_ms;
    b->accounted = true;
    return b->kind == 2 ? finish_refine(b) : NRA_OK;
}

int nra_batch_sync(nra_batch_t* b)
{
    if (!b) return fail(NRA_E_ARG, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const int rc = account_run(b);
    if (rc || b->kind != 1) return rc;
    return one_copy_1d(b) ? stage_results_1d(b) : check_mt(b);
}

int nra_batch1d_resweeps(nra_batch_t* b, int64_t* tasks, int64_t* reads, int64_t* tasks_total, int64_t* reads_total)
{
    if (!b || b->kind != 1) return fail(NRA_E_ARG, "nra_batch1d_resweeps needs a 1D batch");
    int64_t nt = 0, nr = 0, tt = 0, tr = 0;
    if (b->redo.n > 0) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));
        std::vector<int32_t> f(b->redo.n);
        HIP_TRY(hipMemcpy(f.data(), b->redo.p, f.size() * 4, hipMemcpyDeviceToHost));
        for (const Bucket& bk : b->buckets) {
            if (!bk.taint) continue;
            for (int t = 0; t < bk.n_sweep; ++t) {
                const size_t i = bk.sweep_off + (size_t)t;
                tt += 1; tr += b->task_reads[i];
                if (f[i]) { nt += 1; nr += b->task_reads[i]; }
            }
        }
    }
    if (tasks) *tasks = nt;
    if (reads) *reads = nr;
    if (tasks_total) *tasks_total = tt;
    if (reads_total) *reads_total = tr;
    return NRA_OK;
}

int nra_batch1d_saturation(nra_batch_t* b, int64_t* sweeps, int64_t* steps, int64_t* sweeps_total, int64_t* steps_total)
{
    if (!b || b->kind != 1) return fail(NRA_E_ARG, "nra_batch1d_saturation needs a 1D batch");
    int64_t ns = 0, nst = 0, ts = 0, tst = 0;
    bool any = false;
    for (const Bucket& bk : b->buckets) any = any || bk.quanta;
    if (any) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));
        std::vector<int32_t> w(b->sat_count.n);
        HIP_TRY(hipMemcpy(w.data(), b->sat_count.p, w.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < b->buckets.size(); ++i) {
            const Bucket& bk = b->buckets[i];
            if (!bk.quanta) continue;
            ts += bk.n_sweep; tst += bk.q_fwd_steps;
            int64_t steps64;
            memcpy(&steps64, &w[4 * i + 2], 8);
            ns += w[4 * i]; nst += steps64;
        }
    }
    if (sweeps) *sweeps = ns;
    if (steps) *steps = nst;
    if (sweeps_total) *sweeps_total = ts;
    if (steps_total) *steps_total = tst;
    return NRA_OK;
}

int nra_batch1d_clears(nra_batch_t* b, int32_t* scores, int32_t* extents)
{
    if (!b || b->kind != 1) return fail(NRA_E_ARG, "nra_batch1d_clears needs a 1D batch");
    if (scores) *scores = clears_scores_1d(b) ? 1 : 0;
    if (extents) *extents = clears_extents_1d(b) ? 1 : 0;
    return NRA_OK;
}

int nra_batch_stats(nra_batch_t* b, nra_stats_t* st)
{
    if (!b || !st) return fail(NRA_E_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    if (b->ran) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        int rc = account_run(b);
        if (rc) return rc;
        if (b->kind == 1 && !(b->flags & NRA_F_ALL_EXTENTS) && !b->buckets.empty()) {
            std::vector<int32_t> tc(b->buckets.size());
            HIP_TRY(hipMemcpy(tc.data(), b->tie_count.p, tc.size() * 4, hipMemcpyDeviceToHost));
            int64_t n = 0;
            for (int32_t v : tc) n += v;
            b->stats.n_extent_tasks = n;
        }
    }
    *st = b->stats;
    return NRA_OK;
}

void nra_batch_destroy(nra_batch_t* b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    delete b;
}

}  // extern "C"
