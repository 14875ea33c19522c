"""The repeat-structure contract in plain Python, and a numpy form vectorised across reads that
share a motif length.  Both are restatements for the tests: the product computes the alignment with k_structure
(nra_read_structure) and the units with nanorepeat_amd.structure.

Alignment of a tract s (upper-cased; a byte other than ACGT mismatches every motif base) against u repeated without
end: D[0][j] = 0; T[j] = min(diag D[i-1][j-1 mod p] + (c != u[j-1 mod p]), ins D[i-1][j] + 1), a tie taking the
diagonal; D[i][j] = min(T[j], D[i][j-1 mod p] + 1) cyclically until stable, a tie keeping T.  edits = min_j D[n][j]
at the smallest such j; the traceback from there gives start_phase and one path byte per base (op | deletions << 2).
"""
import numpy as np

MATCH, MISMATCH, INSERTION = 0, 1, 2


def _upper(s):
    return s.decode("latin-1").upper() if isinstance(s, (bytes, bytearray)) else s.upper()


def plain_align(s, u):
    """-> (edits, start_phase, path bytes) of one tract, row by row as the contract states it."""
    s, p, n = _upper(s), len(u), len(s)
    D = [0] * p
    ptr = []
    for i in range(1, n + 1):
        c = s[i - 1]
        T, ins = [0] * p, [False] * p
        for j in range(p):
            jm = (j - 1) % p
            diag = D[jm] + (0 if c == u[jm] else 1)
            up = D[j] + 1
            ins[j] = up < diag
            T[j] = min(diag, up)
        E = list(T)
        changed = True
        while changed:
            changed = False
            for j in range(p):
                v = E[(j - 1) % p] + 1
                if v < E[j]:
                    E[j], changed = v, True
        ptr.append((ins, [E[j] < T[j] for j in range(p)]))
        D = E
    edits = min(D)
    j = D.index(edits)
    path = bytearray(n)
    for i in range(n, 0, -1):
        ins, dl = ptr[i - 1]
        nd = 0
        while dl[j]:
            j, nd = (j - 1) % p, nd + 1
        if ins[j]:
            op = INSERTION
        else:
            jm = (j - 1) % p
            op = MATCH if s[i - 1] == u[jm] else MISMATCH
            j = jm
        path[i - 1] = op | nd << 2
    return edits, (j if n else 0), bytes(path)


def numpy_align_same_p(tracts, motifs):
    """The contract for many tracts whose motifs share one length p, as array operations over the reads.
    -> (edits, start_phase, [path bytes])."""
    R = len(tracts)
    if R == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), []
    p = len(motifs[0])
    assert all(len(u) == p for u in motifs)
    lens = np.array([len(t) for t in tracts], np.int64)
    N = int(lens.max()) if R else 0
    codes = np.full((R, max(N, 1)), 255, np.uint8)
    for r, t in enumerate(tracts):
        if len(t):
            codes[r, :len(t)] = np.frombuffer(_upper(t).encode("latin-1"), np.uint8)
    U = np.array([np.frombuffer(u.encode(), np.uint8) for u in motifs]).reshape(R, p)
    Uprev = np.roll(U, 1, axis=1)                        # Uprev[:, j] = u[(j - 1) mod p]
    D = np.zeros((R, p), np.int64)
    INS = np.zeros((N, R, p), bool)
    DEL = np.zeros((N, R, p), bool)
    for i in range(N):
        live = lens > i
        c = codes[:, i][:, None]
        diag = np.roll(D, 1, axis=1) + (c != Uprev)
        up = D + 1
        ins = up < diag
        T = np.minimum(diag, up)
        E = T.copy()
        for _ in range(p):
            E2 = np.minimum(E, np.roll(E, 1, axis=1) + 1)
            if np.array_equal(E2, E):
                break
            E = E2
        INS[i] = ins & live[:, None]
        DEL[i] = (E < T) & live[:, None]
        D = np.where(live[:, None], E, D)
    edits = D.min(axis=1)
    j = D.argmin(axis=1)
    paths = np.zeros((R, max(N, 1)), np.uint8)
    rows = np.arange(R)
    for t in range(N):
        i = lens - 1 - t                                  # each read's row falls by one per base
        act = i >= 0
        ii = np.where(act, i, 0)
        nd = np.zeros(R, np.int64)
        while True:
            d = act & DEL[ii, rows, j]
            if not d.any():
                break
            j = np.where(d, (j - 1) % p, j)
            nd += d
        ins = INS[ii, rows, j]
        jm = (j - 1) % p
        op = np.where(ins, INSERTION, np.where(codes[rows, ii] == U[rows, jm], MATCH, MISMATCH))
        j = np.where(act & ~ins, jm, j)
        paths[rows[act], ii[act]] = (op | nd << 2)[act]
    start = np.where(lens > 0, j, 0)
    return edits.astype(np.int32), start.astype(np.int32), [bytes(paths[r, :lens[r]]) for r in range(R)]


def ref_read_structure(motifs, tracts, read_motif, device=0, vectorised=True):
    """Stand-in for _capi.read_structure (same arguments, same result dict) on the CPU."""
    n = len(tracts)
    rm = np.asarray(read_motif, np.int64)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in tracts])
    out = dict(edits=np.zeros(n, np.int32), start_phase=np.zeros(n, np.int32), path=np.zeros(int(off[-1]), np.uint8),
               path_off=off)
    for m, u in enumerate(motifs):
        if not (1 <= len(u) <= 64) or set(u) - set("ACGT"):
            raise ValueError(f"bad motif {u!r}")
    by_p = {}
    for r in range(n):
        by_p.setdefault(len(motifs[rm[r]]), []).append(r)
    for p, idx in by_p.items():
        if vectorised:
            e, st, paths = numpy_align_same_p([tracts[r] for r in idx], [motifs[rm[r]] for r in idx])
        else:
            got = [plain_align(tracts[r], motifs[rm[r]]) for r in idx]
            e, st, paths = [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]
        for k, r in enumerate(idx):
            out["edits"][r], out["start_phase"][r] = e[k], st[k]
            out["path"][off[r]:off[r + 1]] = np.frombuffer(paths[k], np.uint8)
    return out


def plain_units(s, u, start_phase, path):
    """The unit derivation restated: -> dict(purity, pure_units, longest_pure_run, interruptions=[(slot, bases)])
    or None for an empty tract."""
    p = len(u)
    if len(path) == 0:
        return None
    slots = {}
    c = start_phase
    cnt = dict(m=0, x=0, i=0, d=0)
    for i, b in enumerate(path):
        op, nd = b & 3, b >> 2
        sl = slots.setdefault(c // p, dict(pos=0, m=0, bases=""))
        sl["bases"] += s[i]
        if op == INSERTION:
            cnt["i"] += 1
        else:
            cnt["m" if op == MATCH else "x"] += 1
            sl["pos"] += 1
            sl["m"] += op == MATCH
            c += 1
        for _ in range(nd):
            slots.setdefault(c // p, dict(pos=0, m=0, bases=""))["pos"] += 1
            cnt["d"] += 1
            c += 1
    order = sorted(slots)
    complete = {k: slots[k]["pos"] == p for k in order}
    pure = {k: complete[k] and slots[k]["m"] == p and len(slots[k]["bases"]) == p for k in order}
    longest, run = 0, 0
    for k in order:
        run = run + 1 if pure[k] else 0
        longest = max(longest, run)
    inter, cur = [], None
    for k in order:
        if complete[k] and not pure[k]:
            if cur is None:
                cur = [k, ""]
            cur[1] += slots[k]["bases"]
        else:
            if cur is not None:
                inter.append((cur[0], cur[1] or "-"))
            cur = None
    if cur is not None:
        inter.append((cur[0], cur[1] or "-"))
    total = sum(cnt.values())
    return dict(purity=cnt["m"] / total, pure_units=sum(pure.values()), longest_pure_run=longest, interruptions=inter)
