"""The tandem-period contract in numpy, vectorised over a tract's positions, and as a plain double
loop; and k_tract_periods' word algorithm lane by lane (`words_tract_periods`), which checks the kernel's arithmetic
without a GPU.  The first two are restatements for the tests: the product counts with k_tract_periods
(nra_tract_periods) and calls with nanorepeat_amd.periods.

The tract s (n bases) is upper-cased.  For p in 1..P (P <= 64): valid[p] = the positions i (0 <= i, i + p < n) where
s[i] and s[i + p] are both A, C, G or T, match[p] = those of them with s[i] == s[i + p]; both 0 where n <= p.
"""
import numpy as np

MAX_PERIOD, MAX_TRACT_LEN = 64, 200000
_LUT = np.full(256, 4, np.int8)
for _i, _b in enumerate("ACGT"):
    _LUT[ord(_b)] = _i
    _LUT[ord(_b.lower())] = _i


def _codes(s):
    b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    return _LUT[np.frombuffer(b, np.uint8)] if b else np.zeros(0, np.int8)


def _tract_numpy(s, max_period):
    c = _codes(s)
    n = len(c)
    ok = c < 4
    match, valid = np.zeros(max_period, np.int32), np.zeros(max_period, np.int32)
    for p in range(1, min(max_period, n - 1) + 1):
        both = ok[:n - p] & ok[p:]
        valid[p - 1] = both.sum()
        match[p - 1] = (both & (c[:n - p] == c[p:])).sum()
    return match, valid


def _tract_plain(s, max_period):
    s = s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s
    s = s.upper()
    match, valid = [0] * max_period, [0] * max_period
    for p in range(1, max_period + 1):
        for i in range(0, len(s) - p):
            if s[i] in "ACGT" and s[i + p] in "ACGT":
                valid[p - 1] += 1
                match[p - 1] += s[i] == s[i + p]
    return match, valid


def ref_tract_periods(tracts, max_period=64, device=0, vectorised=True):
    """Same signature and outputs as nanorepeat_amd._capi.tract_periods."""
    if not 1 <= max_period <= MAX_PERIOD:
        raise ValueError("max_period in 1..64")
    if any(len(t) > MAX_TRACT_LEN for t in tracts):
        raise ValueError("tract longer than 200000 bases")
    n = len(tracts)
    out = dict(match=np.zeros((n, max_period), np.int32), valid=np.zeros((n, max_period), np.int32))
    for t, s in enumerate(tracts):
        out["match"][t], out["valid"][t] = (_tract_numpy if vectorised else _tract_plain)(s, max_period)
    return out


_M64 = (1 << 64) - 1


def words_tract_periods(s):
    """k_tract_periods lane by lane in Python integers: words of 32 bases packed to 2-bit codes and a validity mask (bit
    2j: base j is ACGT and inside the tract), 64 words packed at a time of which the wave takes 62, lane l shifting the
    pair (word, next) by l + 1 bases for l < 32 and the pair (next, next2) by l - 31 bases beyond.  -> (match, valid) of
    the 64 lags."""
    c = [int(x) for x in _codes(s)]
    n = len(c)
    n_words = (n + 31) // 32

    def pack(g):
        rem, bits, ok = n - 32 * g, 0, 0
        for j in range(32 if rem > 0 else 0):
            code = c[32 * g + j] if j < rem else 4              # what lies behind the tract does not matter
            bits |= (code & 3) << (2 * j)
            ok |= int(code <= 3 and j < rem) << (2 * j)
        return bits, ok

    match, valid = [0] * 64, [0] * 64
    for w0 in range(0, n_words, 62):
        packed = [pack(w0 + lane) for lane in range(64)]
        for lane in range(64):
            far = lane >= 32
            sh = 2 * (lane - 31 if far else lane + 1)
            for w in range(min(62, n_words - w0)):
                (b0, m0), (b1, m1), (b2, m2) = packed[w], packed[w + 1], packed[w + 2]
                (ba, bb), (ma, mb) = ((b1, b2), (m1, m2)) if far else ((b0, b1), (m0, m1))
                bs = ((ba >> sh) if sh < 64 else 0) | ((bb << (64 - sh)) & _M64)
                ms = ((ma >> sh) if sh < 64 else 0) | ((mb << (64 - sh)) & _M64)
                x, both = b0 ^ bs, m0 & ms
                valid[lane] += bin(both).count("1")
                match[lane] += bin(both & ~(x | (x >> 1)) & _M64).count("1")
    return match, valid
