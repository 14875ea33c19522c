"""The motif-run contract (include/nanorepeat_amd.h) restated twice for the tests: `plain_segment`
is plain Python over the full matrix with the layers T / A / D spelled out, `numpy_forward` + `_trace` do the forward
pass as array operations over all tracts that share a motif set.  The product computes the same with k_segment
(nra_tract_segments).

A motif set is M <= 8 motifs with S = sum of their lengths <= 32 states, state (m, j) = "in motif m, j motif bases
consumed mod p_m", ordered by (m, j).  Per tract base: T = min(diagonal, insertion), A = T closed under deletions
cyclic inside each motif, D = min(A, best A of another motif + W).  Ties: diagonal, insertion, deletion, switch.
"""
import numpy as np

MATCH, MISMATCH, INSERTION = 0, 1, 2
MAX_MOTIFS, MAX_STATES, MAX_TRACT_LEN, MAX_SWITCH_COST = 8, 32, 200000, 1000
BIG = 1 << 28


def _upper(s):
    return s.decode("latin-1").upper() if isinstance(s, (bytes, bytearray)) else s.upper()


def check_set(motifs, switch_cost):
    """ValueError for what the C ABI answers with NRA_E_ARG or NRA_E_RANGE."""
    if not 1 <= switch_cost <= MAX_SWITCH_COST:
        raise ValueError(f"switch cost {switch_cost}")
    if not 1 <= len(motifs) <= MAX_MOTIFS:
        raise ValueError(f"{len(motifs)} motifs in a set")
    if any(len(u) == 0 or set(u) - set("ACGT") for u in motifs):
        raise ValueError(f"bad motif in {motifs!r}")
    if sum(len(u) for u in motifs) > MAX_STATES:
        raise ValueError(f"more than {MAX_STATES} states in {motifs!r}")


def layout(motifs):
    """-> (prev, base, mot, phase): per state, the state a diagonal or a deletion comes from, the motif base that step
    consumes, the state's motif and its phase."""
    states = [(m, j) for m, u in enumerate(motifs) for j in range(len(u))]
    index = {st: g for g, st in enumerate(states)}
    prev = [index[(m, (j - 1) % len(motifs[m]))] for m, j in states]
    base = [motifs[m][(j - 1) % len(motifs[m])] for m, j in states]
    return prev, base, [m for m, _ in states], [j for _, j in states]


def _trace(s, n, end, rows, prev, base, mot, phase):
    """rows[i - 1] = (ins, dl, sw, s1, s2) of row i -> (start_phase, start_motif, path bytes, motif bytes)."""
    path, which = bytearray(n), bytearray(n)
    g = end
    for i in range(n, 0, -1):
        ins, dl, sw, s1, s2 = rows[i - 1]
        if sw[g]:
            g = s1 if mot[g] != mot[s1] else s2          # continues at the A-layer of the source state
        nd = 0
        while dl[g]:
            g, nd = prev[g], nd + 1
        which[i - 1] = mot[g]
        if ins[g]:
            op = INSERTION
        else:
            op = MATCH if s[i - 1] == base[g] else MISMATCH
            g = prev[g]
        path[i - 1] = op | nd << 2
    return phase[g], mot[g], bytes(path), bytes(which)


def plain_segment(s, motifs, switch_cost):
    """One tract, row by row as the contract states it -> (edits, start_phase, start_motif, path, motif_of)."""
    s, n, W = _upper(s), len(s), switch_cost
    prev, base, mot, phase = layout(motifs)
    S = len(prev)
    D = [0] * S
    rows = []
    for i in range(1, n + 1):
        c = s[i - 1]
        T, ins = [0] * S, [False] * S
        for g in range(S):
            diag = D[prev[g]] + (0 if c == base[g] else 1)
            up = D[g] + 1
            ins[g] = up < diag
            T[g] = min(diag, up)
        A = list(T)
        changed = True
        while changed:
            changed = False
            for g in range(S):
                v = A[prev[g]] + 1
                if v < A[g]:
                    A[g], changed = v, True
        dl = [A[g] < T[g] for g in range(S)]
        b1 = min(A)
        s1 = A.index(b1)
        others = [g for g in range(S) if mot[g] != mot[s1]]
        b2, s2 = None, 0
        if others:
            b2 = min(A[g] for g in others)
            s2 = next(g for g in others if A[g] == b2)
        Dn, sw = list(A), [False] * S
        for g in range(S):
            cand = b1 if mot[g] != mot[s1] else b2
            if cand is not None and cand + W < A[g]:
                Dn[g], sw[g] = cand + W, True
        rows.append((ins, dl, sw, s1, s2))
        D = Dn
    edits = min(D)
    return (edits,) + _trace(s, n, D.index(edits), rows, prev, base, mot, phase)


def numpy_forward(tracts, motifs, switch_cost):
    """The forward pass for many tracts of one motif set as array operations over (tract, state)
    -> (final D [R, S], INS, DEL, SW [N, R, S] bool, S1, S2 [N, R])."""
    R, W = len(tracts), switch_cost
    prev, base, mot, _ = layout(motifs)
    prev, mot = np.array(prev), np.array(mot)
    base = np.frombuffer("".join(base).encode(), np.uint8)
    S = len(prev)
    lens = np.array([len(t) for t in tracts], np.int64)
    N = int(lens.max()) if R else 0
    codes = np.full((R, max(N, 1)), 255, np.uint8)
    for r, t in enumerate(tracts):
        if len(t):
            codes[r, :len(t)] = np.frombuffer(_upper(t).encode("latin-1"), np.uint8)
    D = np.zeros((R, S), np.int64)
    INS, DEL, SW = (np.zeros((N, R, S), bool) for _ in range(3))
    S1, S2 = np.zeros((N, R), np.int64), np.zeros((N, R), np.int64)
    rows = np.arange(R)
    for i in range(N):
        live = (lens > i)[:, None]
        diag = D[:, prev] + (codes[:, i][:, None] != base[None, :])
        up = D + 1
        T = np.minimum(diag, up)
        A = T
        while True:
            A2 = np.minimum(A, A[:, prev] + 1)
            if np.array_equal(A2, A):
                break
            A = A2
        s1 = A.argmin(axis=1)                               # the first state that attains the minimum
        b1 = A[rows, s1]
        same = mot[None, :] == mot[s1][:, None]
        other = np.where(same, BIG, A)
        s2 = other.argmin(axis=1)
        b2 = other[rows, s2]
        cand = np.where(same, b2[:, None], b1[:, None]) + W
        sw = cand < A
        INS[i], DEL[i], SW[i] = (up < diag) & live, (A < T) & live, sw & live
        S1[i], S2[i] = s1, s2
        D = np.where(live, np.where(sw, cand, A), D)
    return D, INS, DEL, SW, S1, S2


def numpy_segment_same_set(tracts, motifs, switch_cost):
    """-> [(edits, start_phase, start_motif, path, motif_of)] per tract."""
    prev, base, mot, phase = layout(motifs)
    D, INS, DEL, SW, S1, S2 = numpy_forward(tracts, motifs, switch_cost)
    out = []
    for r, t in enumerate(tracts):
        n = len(t)
        end = int(D[r].argmin())
        rows = [(INS[i, r], DEL[i, r], SW[i, r], int(S1[i, r]), int(S2[i, r])) for i in range(n)]
        out.append((int(D[r, end]),) + _trace(_upper(t), n, end, rows, prev, base, mot, phase))
    return out


def ref_tract_segments(sets, tracts, tract_set, switch_cost, device=0, vectorised=True):
    """Stand-in for _capi.tract_segments (same arguments, same result dict) on the CPU."""
    sets = [list(x) for x in sets]
    for motifs in sets:
        check_set(motifs, switch_cost)
    n = len(tracts)
    ts = np.asarray(tract_set, np.int64)
    if len(ts) != n or (n and (ts.min() < 0 or ts.max() >= len(sets))):
        raise ValueError("one set index per tract")
    if any(len(t) > MAX_TRACT_LEN for t in tracts):
        raise ValueError("tract beyond 200000 bases")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in tracts])
    out = dict(edits=np.zeros(n, np.int32), start_phase=np.zeros(n, np.int32), start_motif=np.zeros(n, np.int32),
               path=np.zeros(int(off[-1]), np.uint8), motif_of=np.zeros(int(off[-1]), np.uint8), path_off=off)
    by_set = {}
    for r in range(n):
        by_set.setdefault(int(ts[r]), []).append(r)
    for q, idx in by_set.items():
        if vectorised:
            got = numpy_segment_same_set([tracts[r] for r in idx], sets[q], switch_cost)
        else:
            got = [plain_segment(tracts[r], sets[q], switch_cost) for r in idx]
        for r, (e, sp, sm, path, which) in zip(idx, got):
            out["edits"][r], out["start_phase"][r], out["start_motif"][r] = e, sp, sm
            out["path"][off[r]:off[r + 1]] = np.frombuffer(path, np.uint8)
            out["motif_of"][off[r]:off[r + 1]] = np.frombuffer(which, np.uint8)
    return out


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("edits", "start_phase", "start_motif", "path", "motif_of", "path_off"))
