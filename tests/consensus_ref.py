"""The allele-consensus contract (include/nanorepeat_amd.h) restated for the tests, twice:
`ref_tract_consensus(..., banded=False)` fills the full (n + 1) x (t + 1) matrix of every alignment, one tract at a
time, exactly as the contract states it; `banded=True` aligns the tracts of a group together inside bands of 64 c
diagonals and widens a band until it proves its result (the rule the device follows).  Both are stand-ins for
_capi.tract_consensus: same arguments, same result (the `stats` apart).

Contract, in short.  Group = the non-empty tracts, upper-cased, ACGT -> 0..3, other -> 4.  Backbone of round 0: the
tracts sorted by (length, position), element (m - 1) // 2, code-4 bases removed.  Alignment: global, unit cost, a code 4
mismatches everything; traceback from (n, t): diagonal if it attains D[i][j], else insertion (i-1, j), else deletion
(i, j-1).  A tract with D[n][t] > max_dist is left out of the round.  Votes: col[j][A C G T deleted] (a code 4 abstains),
ins[j][A C G T] = the first base, in tract order, of the insertion run in slot j (if ACGT).  New backbone: slot j emits
argmax ins[j] (tie: smallest code) when 2 * sum ins[j] > m_v; column j emits its most voted symbol (tie: the backbone's
own base if tied, else the smallest code, deleted last) unless that is "deleted".  Rounds until a backbone comes back
unchanged (converged) or max_rounds; a round nobody votes in ends the group, not converged.  Support of a base = the
votes for it in the round that emitted it.
"""
import numpy as np

MAX_DIST = 1000
CLASSES = (1, 2, 4, 8, 16)
INF = 1 << 28
DELETED = 5            # in a column-symbol array: the tract deleted the column (4 = aligned a non-ACGT base)

_LUT = np.full(256, 4, np.uint8)
for _i, _ch in enumerate("ACGT"):
    _LUT[ord(_ch)] = _i
    _LUT[ord(_ch.lower())] = _i


def encode(s):
    if isinstance(s, str):
        s = s.encode("latin-1")
    return _LUT[np.frombuffer(bytes(s), np.uint8)]


def full_matrix(s, b):
    """D of the contract, (n + 1) x (t + 1)."""
    n, t = len(s), len(b)
    D = np.zeros((n + 1, t + 1), np.int32)
    ar = np.arange(t + 1)
    D[0] = ar
    for i in range(1, n + 1):
        T = np.empty(t + 1, np.int64)
        T[0] = i
        T[1:] = np.minimum(D[i - 1, :-1] + (b != s[i - 1]), D[i - 1, 1:] + 1)
        D[i] = ar + np.minimum.accumulate(T - ar)
    return D


def align_full(s, b):
    """-> (distance, col [t]: the code aligned to column j or DELETED, ins [t + 1]: first inserted code of slot j or -1)."""
    n, t = len(s), len(b)
    D = full_matrix(s, b)
    col = np.full(t, -1, np.int8)
    ins = np.full(t + 1, -1, np.int8)
    i, j = n, t
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (s[i - 1] != b[j - 1]):
            col[j - 1] = s[i - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            ins[j] = s[i - 1]            # the walk goes towards the tract's start: the last one written is the first base
            i -= 1
        else:
            col[j - 1] = DELETED
            j -= 1
    return int(D[n, t]), col, ins


def _aligner_full(codes, b, max_dist, stats):
    out = []
    for s in codes:
        d, col, ins = align_full(s, b)
        out.append((col, ins) if d <= max_dist else None)
    return out


def proven(c, n, t):
    """What a band of 64 c diagonals proves for (n, t): distances up to the value returned; -1 if it holds no band."""
    extra = 64 * c - 1 - abs(t - n)
    return -1 if extra < 0 else abs(t - n) + 2 * (extra // 2)


def _band_batch(S, b, c):
    """Banded alignment of the tracts S (code arrays) to b in class c, together.  -> (dist [R], col [R, t], ins [R, t+1]);
    col / ins are meaningful only for tracts whose distance the band proves."""
    R, B, t = len(S), 64 * c, len(b)
    n = np.array([len(s) for s in S], np.int64)
    nmax = int(n.max())
    delta = t - n
    h = (B - 1 - np.abs(delta)) // 2
    assert (h >= 0).all()
    lo = np.minimum(0, delta) - h
    codes = np.full((R, nmax), 4, np.uint8)
    for r, s in enumerate(S):
        codes[r, :len(s)] = s
    bpad = np.concatenate([b, [5]]).astype(np.uint8)
    k = np.arange(B)[None, :]
    j = lo[:, None] + k
    D = np.where((j >= 0) & (j <= t), j, INF).astype(np.int64)
    PTR = np.zeros((nmax, R, B), np.uint8)
    infcol = np.full((R, 1), INF, np.int64)
    for i in range(1, nmax + 1):
        j = i + lo[:, None] + k
        valid = (j >= 0) & (j <= t)
        bj = bpad[np.where((j >= 1) & (j <= t), j - 1, t)]
        diag = D + (bj != codes[:, i - 1][:, None])
        up = np.concatenate([D[:, 1:], infcol], axis=1) + 1
        T = np.where(valid, np.minimum(diag, up), INF)
        E = np.where(valid, k + np.minimum.accumulate(T - k, axis=1), INF)
        PTR[i - 1] = np.where(diag == E, 0, np.where(up == E, 1, 2))
        live = (n >= i)[:, None]
        D = np.where(live, E, D)
    rows = np.arange(R)
    dist = D[rows, delta - lo]
    col = np.full((R, t), -1, np.int8)
    ins = np.full((R, t + 1), -1, np.int8)
    i, j = n.copy(), np.full(R, t, np.int64)
    ok = dist <= np.abs(delta) + 2 * h
    while True:
        act = ok & ((i > 0) | (j > 0))
        if not act.any():
            break
        ii, jj = np.maximum(i, 1), np.maximum(j, 1)
        kk = np.clip(j - i - lo, 0, B - 1)
        op = PTR[ii - 1, rows, kk]
        op = np.where(i == 0, 2, np.where(j == 0, 1, op))
        base = codes[rows, ii - 1]
        dg, up, dl = act & (op == 0), act & (op == 1), act & (op == 2)
        col[rows[dg], jj[dg] - 1] = base[dg]
        ins[rows[up], j[up]] = base[up]
        col[rows[dl], jj[dl] - 1] = DELETED
        i = i - (dg | up)
        j = j - (dg | dl)
    return dist, col, ins


def start_class(n, t, max_dist):
    want = min(max_dist, abs(t - n) + n // 6 + 8)
    for ci, c in enumerate(CLASSES):
        if proven(c, n, t) >= want:
            return ci
    return len(CLASSES) - 1


def _aligner_banded(codes, b, max_dist, stats, budget=1 << 27):
    """The widening rule: a tract is aligned in class c; a banded distance <= min(proven, max_dist) is exact and votes,
    else proven >= max_dist says left out, else the next class."""
    t = len(b)
    out = [None] * len(codes)
    todo = {}
    for r, s in enumerate(codes):
        if abs(t - len(s)) <= max_dist:          # the distance is at least |t - n|
            todo.setdefault(start_class(len(s), t, max_dist), []).append(r)
    for ci, c in enumerate(CLASSES):
        idx = sorted(todo.pop(ci, []), key=lambda r: -len(codes[r]))
        at = 0
        while at < len(idx):
            nmax = len(codes[idx[at]])
            step = max(1, budget // (nmax * 64 * c))
            part = idx[at:at + step]
            at += step
            dist, col, ins = _band_batch([codes[r] for r in part], b, c)
            for q, r in enumerate(part):
                w = proven(c, len(codes[r]), t)
                stats["aligned_%d" % (64 * c)] = stats.get("aligned_%d" % (64 * c), 0) + 1
                if dist[q] <= min(w, max_dist):
                    out[r] = (col[q], ins[q])
                elif w < max_dist:
                    stats["widened"] = stats.get("widened", 0) + 1
                    todo.setdefault(ci + 1, []).append(r)
    assert not todo
    return out


def build_backbone(b, colv, insv, mv):
    """-> (new backbone, supports) from the votes of m_v tracts."""
    t = len(b)
    new, sup = [], []
    tot = insv.sum(axis=1)
    ic = insv.argmax(axis=1)                     # the first maximum: the smallest code on a tie
    mx = colv.max(axis=1) if t else np.zeros(0, np.int64)
    for j in range(t + 1):
        if 2 * tot[j] > mv:
            new.append(ic[j])
            sup.append(insv[j, ic[j]])
        if j < t:
            if colv[j, b[j]] == mx[j]:
                sym = b[j]
            else:
                sym = int(np.flatnonzero(colv[j] == mx[j])[0])
            if sym != 4:
                new.append(sym)
                sup.append(mx[j])
    return np.array(new, np.uint8), np.array(sup, np.int32)


def consensus_group(tracts, max_dist=MAX_DIST, max_rounds=8, banded=True, stats=None):
    """One group -> dict(consensus, support, n_rounds, converged, voted, left_out)."""
    stats = {} if stats is None else stats
    aligner = _aligner_banded if banded else _aligner_full
    codes = [encode(t) for t in tracts if len(t)]
    m = len(codes)
    if m == 0:
        return dict(consensus="", support=np.zeros(0, np.int32), n_rounds=0, converged=0, voted=0, left_out=0)
    order = sorted(range(m), key=lambda q: (len(codes[q]), q))
    b = codes[order[(m - 1) // 2]]
    b = b[b < 4]
    support = np.zeros(len(b), np.int32)
    n_rounds = converged = voted = left = 0
    for rnd in range(1, max_rounds + 1):
        n_rounds = rnd
        res = [x for x in aligner(codes, b, max_dist, stats) if x is not None]
        mv = len(res)
        if mv == 0:
            converged, voted, left = 0, 0, m
            break
        t = len(b)
        colv = np.zeros((t, 5), np.int64)
        insv = np.zeros((t + 1, 4), np.int64)
        for col, ins in res:
            for c in range(4):
                colv[:, c] += col == c
                insv[:, c] += ins == c
            colv[:, 4] += col == DELETED
        new, support = build_backbone(b, colv, insv, mv)
        same = np.array_equal(new, b)
        b, voted, left = new, mv, m - mv
        if same:
            converged = 1
            break
    return dict(consensus="".join("ACGT"[c] for c in b), support=support, n_rounds=n_rounds, converged=converged,
                voted=voted, left_out=left)


def ref_tract_consensus(groups, max_dist=MAX_DIST, max_rounds=8, device=0, banded=True):
    """Stand-in for _capi.tract_consensus (same arguments, same result dict) on the CPU."""
    if not 0 <= max_dist <= MAX_DIST or not 1 <= max_rounds <= 64:
        raise ValueError("max_dist or max_rounds out of range")
    stats = {}
    got = [consensus_group(list(g), max_dist, max_rounds, banded, stats) for g in groups]
    return dict(consensus=[g["consensus"] for g in got], support=[g["support"] for g in got],
                n_rounds=np.array([g["n_rounds"] for g in got], np.int32),
                converged=np.array([g["converged"] for g in got], np.int32),
                voted=np.array([g["voted"] for g in got], np.int32),
                left_out=np.array([g["left_out"] for g in got], np.int32), stats=stats)


def same_result(a, b):
    """Every field of two results but the stats."""
    return (a["consensus"] == b["consensus"] and len(a["support"]) == len(b["support"])
            and all(np.array_equal(x, y) for x, y in zip(a["support"], b["support"]))
            and all(np.array_equal(a[k], b[k]) for k in ("n_rounds", "converged", "voted", "left_out")))
