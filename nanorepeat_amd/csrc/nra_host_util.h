// nra_host_util.h -- what the one-shot feature hosts (nra_*_host.cpp, not nra_host.cpp) share: the error return and the
// HIP-error macro, the device buffer, the byte-to-code table, the device preamble and the checks of motifs and offsets.
#ifndef NRA_HOST_UTIL_H
#define NRA_HOST_UTIL_H
#include "nanorepeat_amd.h"
#include "nra_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

namespace nra_host {

inline int fail(int code, const std::string& msg) { return nra_set_error(code, msg.c_str()); }

#define NRA_HIP_TRY(expr)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return nra_host::fail(e_ == hipErrorOutOfMemory ? NRA_E_NOMEM : NRA_E_DEVICE,        \
                                  std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// a device buffer of `cap` elements (at least one): alloc() for a buffer of one size, ensure() for one that grows
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(size_t n)
    {
        release();
        n = std::max<size_t>(n, 1);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    hipError_t ensure(size_t n) { return std::max<size_t>(n, 1) <= cap ? hipSuccess : alloc(n); }
};

// the code of a sequence byte: A, C, G, T in either case are 0..3, every other byte is 4
const int kCodeOther = 4;
static_assert(NRA_STRUCT_CODE_OTHER == kCodeOther && NRA_MOTIF_CODE_OTHER == kCodeOther &&
                  NRA_CONS_CODE_OTHER == kCodeOther,
              "the kernels agree on the code of a byte other than ACGT");
struct BaseCodes {
    uint8_t of[256];
    constexpr BaseCodes() : of()
    {
        for (int c = 0; c < 256; ++c) of[c] = (uint8_t)kCodeOther;
        of['A'] = of['a'] = 0;
        of['C'] = of['c'] = 1;
        of['G'] = of['g'] = 2;
        of['T'] = of['t'] = 3;
    }
};
inline constexpr BaseCodes kBase{};

inline void encode(uint8_t* dst, const char* src, int64_t n)
{
    const unsigned char* s = reinterpret_cast<const unsigned char*>(src);
    for (int64_t i = 0; i < n; ++i) dst[i] = kBase.of[s[i]];
}

// The device of a call, after the checks of its arguments.  `work` false: the call has nothing to launch; the device is
// still checked but not made current.
inline int use_device(int device, bool work = true)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NRA_E_DEVICE, "no HIP device: nanorepeat_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(NRA_E_ARG, "device index out of range");
    if (work) NRA_HIP_TRY(hipSetDevice(device));
    return NRA_OK;
}

// a byte budget, or what the environment variable `env_name` (NRA_TEST_*_BYTES: tests force small chunks) gives
inline int64_t test_bytes(const char* env_name, int64_t budget)
{
    if (const char* e = getenv(env_name)) return std::max<int64_t>(1, atoll(e));
    return budget;
}

// motifs [first, last): not empty, at most max_len bases, upper-case ACGT only
inline int check_motifs(int32_t first, int32_t last, const char* motifs, const int64_t* motif_off, int64_t max_len)
{
    for (int32_t m = first; m < last; ++m) {
        const int64_t p = motif_off[m + 1] - motif_off[m];
        if (p < 1) return fail(NRA_E_ARG, "motif " + std::to_string(m) + " is empty");
        if (p > max_len)
            return fail(NRA_E_RANGE, "motif " + std::to_string(m) + " is longer than " + std::to_string(max_len) + " bases");
        for (int64_t i = motif_off[m]; i < motif_off[m + 1]; ++i)
            if (!std::strchr("ACGT", motifs[i]) || motifs[i] == 0)
                return fail(NRA_E_ARG, "motif " + std::to_string(m) + " has a base other than A, C, G, T");
    }
    return NRA_OK;
}

// the n + 1 offsets of n sequences: not negative, not decreasing, no sequence longer than max_len.  `noun` names the
// offsets ("read", "tract"), `item` the sequence that is too long
inline int check_tract_offsets(int32_t n, const int64_t* off, int64_t max_len, const char* noun, const char* item = "tract")
{
    if (off[0] < 0) return fail(NRA_E_ARG, std::string("negative ") + noun + " offset");
    for (int32_t r = 0; r < n; ++r) {
        const int64_t len = off[r + 1] - off[r];
        if (len < 0) return fail(NRA_E_ARG, std::string(noun) + " offsets must not decrease");
        if (len > max_len)
            return fail(NRA_E_RANGE, std::string(item) + " " + std::to_string(r) + " is longer than " +
                                         std::to_string(max_len) + " bases");
    }
    return NRA_OK;
}

}  // namespace nra_host

#endif  // NRA_HOST_UTIL_H
