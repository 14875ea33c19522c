// nra_methyl_host.cpp -- C ABI of the per-read CpG methylation counts (nra_read_methylation): argument checks, the order
// of the reads (length, descending), the chunks that bound the device and host buffers (bases, lists and results), and
// the launches of k_read_methylation (nra_methyl.hip).  NRA_DEBUG in the environment traces every chunk on stderr.
#include "nra_host_util.h"

#include <algorithm>
#include <cstdio>
#include <limits>
#include <new>
#include <numeric>
#include <string>
#include <vector>

using namespace nra_host;

namespace {

const int64_t kChunkBudget = int64_t(1) << 28;  // bytes per chunk (one read beyond it goes alone)
const int kGroupsPerCU = 8;                     // workgroups of 4 waves resident per CU

struct Call {
    const char* seqs;
    const int64_t* seq_off;
    const int32_t* deltas;
    const uint8_t* probs;
    const int64_t* mod_off;
    const uint8_t* flags;
    const int32_t* tract_lo;
    const int32_t* tract_hi;
    int32_t flank, bin, nb, lo_byte, hi_byte;
    int32_t* counts;
    int32_t* n_c;
    int32_t* status;
    int64_t len(int32_t r) const { return seq_off[r + 1] - seq_off[r]; }
    // the entries of read r's list that go to the device: none of a list longer than the read (BAD_TAG as it stands)
    int64_t mods(int32_t r) const
    {
        const int64_t m = mod_off[r + 1] - mod_off[r];
        return m > len(r) ? 0 : m;
    }
    int64_t cells() const { return (2 * (int64_t)nb + 1) * NRA_METH_COUNTERS; }
    // what a read costs of a chunk's budget: its bases, its deltas and call bytes, its counters (device and host)
    int64_t cost(int32_t r) const
    {
        return len(r) + mods(r) * (int64_t)(sizeof(int32_t) + 1) + cells() * (int64_t)sizeof(int32_t);
    }
};

int run_chunk(const Call& c, size_t first, size_t last, const std::vector<int32_t>& order, int n_cu)
{
    const size_t n = last - first;
    std::vector<NraMethRead> rd(n);
    int64_t seq_bytes = 0, n_mods = 0;
    for (size_t l = 0; l < n; ++l) {
        const int32_t r = order[first + l];
        const bool too_many = c.mod_off[r + 1] - c.mod_off[r] > c.len(r);
        rd[l].seq = (uint64_t)seq_bytes;
        rd[l].mod = (uint64_t)n_mods;
        rd[l].n = (int32_t)c.len(r);
        rd[l].m = (int32_t)c.mods(r);
        rd[l].lo = c.tract_lo[r];
        rd[l].hi = c.tract_hi[r];
        rd[l].flags = (int32_t)c.flags[r] | (too_many ? NRA_METH_F_TOO_MANY : 0);
        rd[l].pad = 0;
        seq_bytes += rd[l].n;
        n_mods += rd[l].m;
    }
    if (getenv("NRA_DEBUG"))
        fprintf(stderr, "nra_read_methylation: chunk of %zu read(s), %lld base(s), %lld listed\n", n,
                (long long)seq_bytes, (long long)n_mods);
    std::vector<uint8_t> seq((size_t)seq_bytes), probs((size_t)n_mods);
    std::vector<int32_t> deltas((size_t)n_mods);
    for (size_t l = 0; l < n; ++l) {
        const int32_t r = order[first + l];
        if (rd[l].n) std::memcpy(seq.data() + rd[l].seq, c.seqs + c.seq_off[r], (size_t)rd[l].n);
        if (rd[l].m) {
            std::memcpy(deltas.data() + rd[l].mod, c.deltas + c.mod_off[r], (size_t)rd[l].m * sizeof(int32_t));
            std::memcpy(probs.data() + rd[l].mod, c.probs + c.mod_off[r], (size_t)rd[l].m);
        }
    }
    const size_t cells = (size_t)c.cells();
    DevBuf<NraMethRead> d_rd;
    DevBuf<uint8_t> d_seq, d_probs;
    DevBuf<int32_t> d_ranks, d_counts, d_nc, d_status;
    NRA_HIP_TRY(d_rd.alloc(n));
    NRA_HIP_TRY(d_seq.alloc(seq.size()));
    NRA_HIP_TRY(d_probs.alloc(probs.size()));
    NRA_HIP_TRY(d_ranks.alloc(deltas.size()));
    NRA_HIP_TRY(d_counts.alloc(n * cells));
    NRA_HIP_TRY(d_nc.alloc(n));
    NRA_HIP_TRY(d_status.alloc(n));
    NRA_HIP_TRY(hipMemcpy(d_rd.p, rd.data(), n * sizeof(NraMethRead), hipMemcpyHostToDevice));
    if (!seq.empty()) NRA_HIP_TRY(hipMemcpy(d_seq.p, seq.data(), seq.size(), hipMemcpyHostToDevice));
    if (!probs.empty()) {
        NRA_HIP_TRY(hipMemcpy(d_probs.p, probs.data(), probs.size(), hipMemcpyHostToDevice));
        NRA_HIP_TRY(hipMemcpy(d_ranks.p, deltas.data(), deltas.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const int grid = (int)std::min<int64_t>((int64_t)n, (int64_t)n_cu * kGroupsPerCU);
    const int e = nra_launch_read_methylation(nullptr, grid, (int)n, d_rd.p, d_seq.p, d_ranks.p, d_probs.p, c.flank,
                                              c.bin, c.nb, c.lo_byte, c.hi_byte, d_counts.p, d_nc.p, d_status.p);
    if (e != 0) return fail(NRA_E_DEVICE, std::string("k_read_methylation: ") + hipGetErrorString((hipError_t)e));
    NRA_HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<int32_t> counts(n * cells), nc(n), st(n);
    NRA_HIP_TRY(hipMemcpy(counts.data(), d_counts.p, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    NRA_HIP_TRY(hipMemcpy(nc.data(), d_nc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    NRA_HIP_TRY(hipMemcpy(st.data(), d_status.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < n; ++l) {
        const int64_t r = order[first + l];
        std::memcpy(c.counts + r * (int64_t)cells, counts.data() + l * cells, cells * sizeof(int32_t));
        c.n_c[r] = nc[l];
        c.status[r] = st[l];
    }
    return NRA_OK;
}

}  // namespace

extern "C" {

int nra_read_methylation(int device, int32_t n_reads, const char* seqs, const int64_t* seq_off, const int32_t* deltas,
                         const uint8_t* probs, const int64_t* mod_off, const uint8_t* flags, const int32_t* tract_lo,
                         const int32_t* tract_hi, int32_t flank, int32_t bin, int32_t lo_byte, int32_t hi_byte,
                         int32_t* counts, int32_t* n_c, int32_t* status)
{
    if (flank < 1) return fail(NRA_E_ARG, "flank must be at least 1");
    if (flank > NRA_METH_MAX_FLANK) return fail(NRA_E_RANGE, "flank is longer than 100000 bases");
    if (bin < 1 || bin > flank) return fail(NRA_E_ARG, "bin must be in 1..flank");
    const int32_t nb = (flank + bin - 1) / bin;
    if (nb > NRA_METH_MAX_BINS) return fail(NRA_E_RANGE, "more than 64 bins per flank");
    if (lo_byte < 0 || hi_byte > 255 || lo_byte >= hi_byte)
        return fail(NRA_E_ARG, "call bytes must satisfy 0 <= lo_byte < hi_byte <= 255");
    if (n_reads < 0) return fail(NRA_E_ARG, "negative read count");
    if (n_reads > 0) {
        if (!seq_off || !mod_off || !flags || !tract_lo || !tract_hi || !counts || !n_c || !status)
            return fail(NRA_E_ARG, "NULL read array");
        if (int rc = check_tract_offsets(n_reads, seq_off, NRA_METH_MAX_N, "read", "read")) return rc;
        if (int rc = check_tract_offsets(n_reads, mod_off, std::numeric_limits<int64_t>::max(), "modification"))
            return rc;
        if (seq_off[n_reads] > seq_off[0] && !seqs) return fail(NRA_E_ARG, "seqs is NULL");
        if (mod_off[n_reads] > mod_off[0] && (!deltas || !probs)) return fail(NRA_E_ARG, "NULL modification array");
        for (int32_t r = 0; r < n_reads; ++r) {
            if (flags[r] & ~(NRA_METH_F_REVERSED | NRA_METH_F_IMPLICIT))
                return fail(NRA_E_ARG, "read " + std::to_string(r) + " has a flag bit other than 0 and 1");
            if (tract_lo[r] < 0 || tract_lo[r] > tract_hi[r] || tract_hi[r] > seq_off[r + 1] - seq_off[r])
                return fail(NRA_E_ARG, "read " + std::to_string(r) + " has a tract outside 0 <= lo <= hi <= n");
        }
        for (int64_t j = mod_off[0]; j < mod_off[n_reads]; ++j)
            if (deltas[j] < 0) return fail(NRA_E_ARG, "negative delta");
    }
    if (int rc = use_device(device, n_reads > 0)) return rc;
    if (n_reads == 0) return NRA_OK;
    try {
        int n_cu = 0;
        NRA_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n_cu, 1);
        const Call c{seqs, seq_off, deltas, probs, mod_off, flags, tract_lo, tract_hi, flank, bin, nb,
                     lo_byte, hi_byte, counts, n_c, status};

        // length descending, then index: the workgroups that start together run about as long
        std::vector<int32_t> order((size_t)n_reads);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return c.len(a) > c.len(b); });
        const int64_t budget = test_bytes("NRA_TEST_METH_BYTES", kChunkBudget);
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            int64_t bytes = 0;
            while (j < order.size()) {
                const int64_t b = c.cost(order[j]);
                if (j > i && bytes + b > budget) break;
                bytes += b;
                ++j;
            }
            const int rc = run_chunk(c, i, j, order, n_cu);
            if (rc != NRA_OK) return rc;
            i = j;
        }
    } catch (const std::bad_alloc&) {
        return fail(NRA_E_NOMEM, "read methylation: host allocation failed");
    }
    return NRA_OK;
}

}  // extern "C"
