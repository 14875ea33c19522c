"""The tandem-motif contract in numpy, vectorised over a tract's positions, and in plain Python
by brute force.  Both are restatements for the tests: the product counts with k_tract_motifs (nra_tract_motifs) and
calls and re-sizes with nanorepeat_amd.motifs.

The tract s is upper-cased.  For p in 1..P (P <= 6), position i (i + 2p <= len(s)) is a tandem position when
s[i:i+p] == s[i+p:i+2p], all 2p bases are ACGT (any other byte breaks the window) and w = s[i:i+p] is primitive (not
x^m for a shorter x).  The class of w is its lexicographically smallest rotation (A < C < G < T), its code that
rotation read in base 4, first base most significant; there are 964 classes for p <= 6.  Per tract: n_tandem[p] for
p = 1..P and the top T classes (1 <= T <= 8) as (p, code, count), by count descending, then p, then code ascending;
(0, -1, 0) in unused slots.
"""
import numpy as np

BASES = "ACGT"
_LUT = np.full(256, 4, np.int64)
for _i, _b in enumerate(BASES):
    _LUT[ord(_b)] = _i
    _LUT[ord(_b.lower())] = _i


def _codes(s):
    b = s.encode("latin-1") if isinstance(s, str) else bytes(s)
    return _LUT[np.frombuffer(b, np.uint8)] if b else np.zeros(0, np.int64)


def _tract_numpy(s, max_period):
    """-> (n_tandem [max_period], {(p, code): count}) of one tract."""
    c = _codes(s)
    n = len(c)
    tandem = np.zeros(max_period, np.int64)
    counts = {}
    for p in range(1, max_period + 1):
        m = n - 2 * p + 1                                   # positions i with i + 2p <= n
        if m <= 0:
            continue
        other = (c > 3).astype(np.int64)
        nbad = np.convolve(other, np.ones(2 * p, np.int64), mode="valid")[:m]
        cc = np.where(c > 3, 0, c)
        w1 = np.zeros(m, np.int64)
        w2 = np.zeros(m, np.int64)
        for j in range(p):
            w1 = w1 * 4 + cc[j:j + m]
            w2 = w2 * 4 + cc[p + j:p + j + m]
        mask = (1 << (2 * p)) - 1
        rot_min, prim = w1.copy(), np.ones(m, bool)
        for r in range(1, p):
            x = ((w1 << (2 * r)) | (w1 >> (2 * (p - r)))) & mask
            prim &= x != w1
            rot_min = np.minimum(rot_min, x)
        hit = (w1 == w2) & (nbad == 0) & prim
        tandem[p - 1] = int(hit.sum())
        codes, cnt = np.unique(rot_min[hit], return_counts=True)
        for code, k in zip(codes.tolist(), cnt.tolist()):
            counts[(p, code)] = k
    return tandem, counts


def _tract_plain(s, max_period):
    """The same by brute force over strings."""
    s = s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s
    s = s.upper()
    tandem = [0] * max_period
    counts = {}
    for p in range(1, max_period + 1):
        for i in range(0, len(s) - 2 * p + 1):
            w = s[i:i + p]
            if s[i + p:i + 2 * p] != w or set(s[i:i + 2 * p]) - set(BASES):
                continue
            if any(w == w[:d] * (p // d) for d in range(1, p) if p % d == 0):
                continue
            cls = min(w[r:] + w[:r] for r in range(p))
            code = 0
            for ch in cls:
                code = code * 4 + BASES.index(ch)
            tandem[p - 1] += 1
            counts[(p, code)] = counts.get((p, code), 0) + 1
    return tandem, counts


def ref_tract_motifs(tracts, max_period=6, top_n=4, device=0, vectorised=True):
    """Same signature and outputs as nanorepeat_amd._capi.tract_motifs."""
    if not 1 <= max_period <= 6 or not 1 <= top_n <= 8:
        raise ValueError("max_period in 1..6, top_n in 1..8")
    n = len(tracts)
    out = dict(n_tandem=np.zeros((n, max_period), np.int32), top_p=np.zeros((n, top_n), np.int8),
               top_code=np.full((n, top_n), -1, np.int32), top_count=np.zeros((n, top_n), np.int32))
    for t, s in enumerate(tracts):
        tandem, counts = (_tract_numpy if vectorised else _tract_plain)(s, max_period)
        out["n_tandem"][t] = tandem
        best = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))[:top_n]
        for q, ((p, code), k) in enumerate(best):
            out["top_p"][t, q], out["top_code"][t, q], out["top_count"][t, q] = p, code, k
    return out


def lyndon_classes(max_period=6):
    """Every class of 1..max_period bases as (p, code), in (p, code) order."""
    out = []
    for p in range(1, max_period + 1):
        mask = (1 << (2 * p)) - 1
        for w in range(1 << (2 * p)):
            if all((((w << (2 * r)) | (w >> (2 * (p - r)))) & mask) > w for r in range(1, p)):
                out.append((p, w))
    return out
