"""Plain-Python restatement of nra_read_methylation (include/nanorepeat_amd.h), written from the
contract and not from the kernel: it materialises the sequenced strand O with a real reverse complement, walks its C
with a counter and keeps the listed ranks in a dict.  `ref_read_methylation` has the signature of
_capi.read_methylation and stands in for it as `methylation_engine`; `np_read_methylation` is the numpy form of the
same contract, for timing comparisons on long reads."""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
BAD_TAG = 1


def sequenced_strand(stored, reversed_):
    s = stored.upper()
    return "".join(COMP.get(c, c) for c in reversed(s)) if reversed_ else s


def ref_one_read(stored, deltas, probs, flags, lo, hi, flank, bin_len, lo_byte, hi_byte):
    """-> (counts [2 nb + 1][5] as lists, n_c, status)"""
    n = len(stored)
    nb = (flank + bin_len - 1) // bin_len
    zero = [[0] * 5 for _ in range(2 * nb + 1)]
    rev, implicit = bool(flags & 1), bool(flags & 2)
    o = sequenced_strand(stored, rev)
    rank_at, n_c = {}, 0                       # position in O -> rank among the C of O
    for i, c in enumerate(o):
        if c == "C":
            rank_at[i] = n_c
            n_c += 1
    if len(deltas) > n:
        return zero, n_c, BAD_TAG
    listed, at = {}, -1
    for d, p in zip(deltas, probs):
        at += int(d) + 1                       # Python integers: no wrap
        listed[at] = int(p)
    if len(deltas) and at >= n_c:
        return zero, n_c, BAD_TAG
    counts = zero
    s_up = stored.upper()
    for s in range(n - 1):
        if s_up[s] != "C" or s_up[s + 1] != "G":
            continue
        r = rank_at[n - 2 - s if rev else s]
        if lo <= s and s + 2 <= hi:
            seg = nb
        elif s + 2 <= lo and lo - s - 2 < flank:
            seg = (lo - s - 2) // bin_len
        elif s >= hi and s - hi < flank:
            seg = nb + 1 + (s - hi) // bin_len
        else:
            continue
        call = listed.get(r, 0 if implicit else None)
        c = counts[seg]
        c[0] += 1
        if call is not None:
            c[1] += 1
            c[2] += call >= hi_byte
            c[3] += call <= lo_byte
            c[4] += call
    return counts, n_c, 0


def ref_read_methylation(reads, mods, flags, tract_lo, tract_hi, flank=2000, bin=200, lo_byte=63, hi_byte=192, device=0):
    n = len(reads)
    nb = (flank + bin - 1) // bin
    out = dict(counts=np.zeros((n, 2 * nb + 1, 5), np.int32), n_c=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for i in range(n):
        seq = reads[i] if isinstance(reads[i], str) else bytes(reads[i]).decode("latin-1")
        c, n_c, st = ref_one_read(seq, mods[i][0], mods[i][1], int(flags[i]), int(tract_lo[i]), int(tract_hi[i]),
                                  flank, bin, lo_byte, hi_byte)
        out["counts"][i], out["n_c"][i], out["status"][i] = c, n_c, st
    return out


def np_one_read(stored, deltas, probs, flags, lo, hi, flank, bin_len, lo_byte, hi_byte):
    """The same contract with numpy arrays over the whole read (stored: bytes)."""
    s = np.frombuffer(stored, np.uint8) & 0xDF
    n = len(s)
    nb = (flank + bin_len - 1) // bin_len
    counts = np.zeros((2 * nb + 1, 5), np.int64)
    rev, implicit = bool(flags & 1), bool(flags & 2)
    is_c = (s[::-1] == ord("G")) if rev else (s == ord("C"))          # in the order of O
    rank = np.cumsum(is_c) - is_c                                      # C of O before each position
    n_c = int(is_c.sum())
    m = len(deltas)
    listed = np.cumsum(np.asarray(deltas, np.int64) + 1) - 1
    if m > n or (m and listed[-1] >= n_c):
        return counts.astype(np.int32), n_c, BAD_TAG
    site = np.flatnonzero((s[:-1] == ord("C")) & (s[1:] == ord("G"))) if n > 1 else np.zeros(0, np.int64)
    r = rank[n - 2 - site] if rev else rank[site]
    seg = np.full(len(site), -1, np.int64)
    in_tract = (lo <= site) & (site + 2 <= hi)
    before = (site + 2 <= lo) & (lo - site - 2 < flank)
    after = (site >= hi) & (site - hi < flank) & ~in_tract
    seg[in_tract] = nb
    seg[before] = (lo - site[before] - 2) // bin_len
    seg[after] = nb + 1 + (site[after] - hi) // bin_len
    keep = seg >= 0
    seg, r = seg[keep], r[keep]
    j = np.searchsorted(listed, r)
    hit = (j < m) & (listed[np.minimum(j, max(m - 1, 0))] == r) if m else np.zeros(len(r), bool)
    call = np.where(hit, np.asarray(probs, np.int64)[np.minimum(j, max(m - 1, 0))] if m else 0, 0 if implicit else -1)
    rows = 2 * nb + 1
    has = call >= 0
    counts[:, 0] = np.bincount(seg, minlength=rows)
    counts[:, 1] = np.bincount(seg[has], minlength=rows)
    counts[:, 2] = np.bincount(seg[has & (call >= hi_byte)], minlength=rows)
    counts[:, 3] = np.bincount(seg[has & (call <= lo_byte)], minlength=rows)
    counts[:, 4] = np.bincount(seg[has], weights=call[has], minlength=rows).astype(np.int64)
    return counts.astype(np.int32), n_c, 0


def np_read_methylation(reads, mods, flags, tract_lo, tract_hi, flank=2000, bin=200, lo_byte=63, hi_byte=192, device=0):
    n = len(reads)
    nb = (flank + bin - 1) // bin
    out = dict(counts=np.zeros((n, 2 * nb + 1, 5), np.int32), n_c=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for i in range(n):
        seq = reads[i].encode("latin-1") if isinstance(reads[i], str) else bytes(reads[i])
        out["counts"][i], out["n_c"][i], out["status"][i] = np_one_read(
            seq, mods[i][0], mods[i][1], int(flags[i]), int(tract_lo[i]), int(tract_hi[i]), flank, bin, lo_byte, hi_byte)
    return out
