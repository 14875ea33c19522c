"""The anchored wraparound extension contract (include/nanorepeat_amd.h) in plain Python -- the
closed form, cell by cell -- and in numpy, vectorised across the reads that share a motif length, with the deletions
as two sequential passes and the wrap between them.  Both are restatements for the tests: the product computes it
with k_extend (nra_extend_tracts).

A sequence s (upper-cased; a byte other than ACGT mismatches every motif base) against u repeated without end, anchored
at row 0 (H[0][j] = 0, M[0][j] = 0, any start phase, no zero floor later):
T[j] = max(diag H[i-1][j-1 mod p] + (a if c == u[j-1 mod p] else -b) with count + 1, ins H[i-1][j] - g), a tie taking
the diagonal; H[i][j] = max over d = 0..p-1 of T[j-d mod p] - g d with count + d, the smallest d among equals.
best = the largest H over all rows, the smallest row and then the smallest phase among equals; (0, 0, 0, 0) when
nothing is positive.
"""
import numpy as np


def _upper(s):
    return s.decode("latin-1").upper() if isinstance(s, (bytes, bytearray)) else s.upper()


def plain_extend(s, u, a=2, b=4, g=6):
    """-> (score, end, end_phase, motif_bases) of one sequence: the closed form of the contract."""
    s, p = _upper(s), len(u)
    H, M = [0] * p, [0] * p
    best = (0, 0, 0, 0)
    for i in range(1, len(s) + 1):
        c = s[i - 1]
        T, TM = [0] * p, [0] * p
        for j in range(p):
            k = (j - 1) % p
            diag = H[k] + (a if c == u[k] else -b)
            ins = H[j] - g
            T[j], TM[j] = (diag, M[k] + 1) if diag >= ins else (ins, M[j])
        H, M = [0] * p, [0] * p
        for j in range(p):
            hv, mv = T[j], TM[j]
            for d in range(1, p):
                k = (j - d) % p
                if T[k] - g * d > hv:
                    hv, mv = T[k] - g * d, TM[k] + d
            H[j], M[j] = hv, mv
        for j in range(p):
            if H[j] > best[0]:
                best = (H[j], i, j, M[j])
    return best


def _delete_pass(H, M, g, ramp, idx):
    """One sequential pass H[j] = max(H[j], H[j-1] - g) over j = 1..p-1 (strictly greater replaces, the count follows)
    for all reads at once: H[j] = max over k <= j of H[k] - g (j - k), and among equal sources the largest k."""
    V = H + ramp                                         # H[k] + g k: the source of j maximises it over k <= j
    cm = np.maximum.accumulate(V, axis=1)
    src = np.maximum.accumulate(np.where(V == cm, idx, -1), axis=1)
    return cm - ramp, np.take_along_axis(M, src, axis=1) + (idx - src)


def numpy_extend_same_p(tracts, motifs, a=2, b=4, g=6):
    """The contract for many sequences whose motifs share one length p, as array operations over the reads; the
    deletions in the two-pass form: a sequential pass over j = 1..p-1, the wrap into phase 0, and the pass once more.
    -> (score, end, end_phase, motif_bases) arrays."""
    R = len(tracts)
    if R == 0:
        return tuple(np.zeros(0, np.int32) for _ in range(4))
    p = len(motifs[0])
    assert all(len(u) == p for u in motifs)
    lens = np.array([len(t) for t in tracts], np.int64)
    N = int(lens.max())
    codes = np.full((R, max(N, 1)), 255, np.uint8)
    for r, t in enumerate(tracts):
        if len(t):
            codes[r, :len(t)] = np.frombuffer(_upper(t).encode("latin-1"), np.uint8)
    U = np.array([np.frombuffer(u.encode(), np.uint8) for u in motifs]).reshape(R, p)
    Uprev = np.roll(U, 1, axis=1)                        # Uprev[:, j] = u[(j - 1) mod p]
    idx = np.broadcast_to(np.arange(p, dtype=np.int64), (R, p))
    ramp = g * idx
    rows = np.arange(R)
    H = np.zeros((R, p), np.int64)
    M = np.zeros((R, p), np.int64)
    best = np.zeros((R, 4), np.int64)
    for i in range(N):
        live = lens > i
        c = codes[:, i][:, None]
        diag = np.roll(H, 1, axis=1) + np.where(c == Uprev, a, -b)
        ins = H - g
        take = diag >= ins
        nH = np.where(take, diag, ins)
        nM = np.where(take, np.roll(M, 1, axis=1) + 1, M)
        if p > 1:
            nH, nM = _delete_pass(nH, nM, g, ramp, idx)
            wrap = nH[:, p - 1] - g > nH[:, 0]
            nH[:, 0] = np.where(wrap, nH[:, p - 1] - g, nH[:, 0])
            nM[:, 0] = np.where(wrap, nM[:, p - 1] + 1, nM[:, 0])
            nH, nM = _delete_pass(nH, nM, g, ramp, idx)
        H = np.where(live[:, None], nH, H)
        M = np.where(live[:, None], nM, M)
        j = H.argmax(axis=1)                             # the first phase that holds the row's maximum
        t = live & (H[rows, j] > best[:, 0])
        best[t] = np.stack([H[rows, j], np.full(R, i + 1), j, M[rows, j]], axis=1)[t]
    return tuple(best[:, q].astype(np.int32) for q in range(4))


def ref_extend_tracts(motifs, tracts, read_motif, match=2, mismatch=4, gap=6, device=0, vectorised=True):
    """Stand-in for _capi.extend_tracts (same arguments, same result dict) on the CPU."""
    n = len(tracts)
    rm = np.asarray(read_motif, np.int64)
    if not (1 <= match <= 127 and 0 <= mismatch <= 127 and 1 <= gap <= 127):
        raise ValueError("score out of range")
    for u in motifs:
        if not (1 <= len(u) <= 64) or set(u) - set("ACGT"):
            raise ValueError(f"bad motif {u!r}")
    keys = ("score", "end", "end_phase", "motif_bases")
    out = {k: np.zeros(n, np.int32) for k in keys}
    by_p = {}
    for r in range(n):
        by_p.setdefault(len(motifs[rm[r]]), []).append(r)
    for p, idx in by_p.items():
        if vectorised:
            got = numpy_extend_same_p([tracts[r] for r in idx], [motifs[rm[r]] for r in idx], match, mismatch, gap)
        else:
            rows = [plain_extend(tracts[r], motifs[rm[r]], match, mismatch, gap) for r in idx]
            got = tuple(np.array([row[q] for row in rows], np.int32) for q in range(4))
        for q, k in enumerate(keys):
            out[k][idx] = got[q]
    return out
