"""The flank-haplotype contract (include/nanorepeat_amd.h) restated for the tests, twice:
`ref_flank_phase(..., banded=False)` fills the full (n + 1) x (t + 1) matrix of every alignment; `banded=True` aligns
inside the bands j - i in [-h, h], h = 32 c - 1, with the widening rule of the device.  Both are stand-ins for
_capi.flank_phase: same arguments, same result (the `stats` apart).

Contract, in short.  Per group two backbone sides (A C G T, from the repeat outward) and rows of up to two segments
(coded as consensus tracts, from the repeat outward).  A segment is aligned to its side with the start pinned and the
end free: e = min_j D[n][j], j* the smallest such j, traceback from (n, j*) by diagonal, insertion, deletion; columns
below j* get the aligned code 0..4 or 5 (deleted), columns from j* on 6 (not covered); e > max_dist leaves the side out
(dist -1, end 0), an absent or empty segment has dist -2, end 0.  Per column n[c] over the rows, cov = rows with a code
<= 5; a site iff offset >= skip, n[b] >= min_count, 100 n[b] >= min_share_pct (n[a] + n[b]), 2 (n[a] + n[b]) >= cov;
beyond max_sites the largest n[b] stay.  Haplotypes and verdict: steps 3 and 4 of tests/split_ref.py over the rows with
an aligned side; any other row has label -1.
"""
import numpy as np

import consensus_ref as C
import split_ref as S

MAX_DIST = 500
NOT_COVERED = 6
UNDECIDED = 2
DEFAULTS = dict(max_dist=MAX_DIST, skip=20, min_count=3, min_share_pct=25, min_purity_pct=75, min_sites=2,
                max_sites=256, max_iter=16)
RES_FIELDS = ("phased", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations")
FIELDS = ("label", "dist", "end", "sites", "site_sym")


def align_full(s, b, max_dist):
    """-> (dist, end, col [t]) of one segment (n >= 1 codes) in the full matrix."""
    n, t = len(s), len(b)
    D = C.full_matrix(s, b)
    e = int(D[n].min())
    col = np.full(t, NOT_COVERED, np.uint8)
    if e > max_dist:
        return -1, 0, col
    end = int(np.argmax(D[n] == e))
    i, j = n, end
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (s[i - 1] != b[j - 1]):
            col[j - 1] = s[i - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            i -= 1
        else:
            col[j - 1] = C.DELETED
            j -= 1
    return e, end, col


def start_class(n, max_dist):
    want = min(max_dist, n // 32 + 8)
    for ci, c in enumerate(C.CLASSES):
        if 32 * c - 1 >= want:
            return ci
    return len(C.CLASSES) - 1


def _band_batch(segs, sides, c):
    """Banded alignment in class c of segs[r] to sides[r], together.  -> (e [R], end [R], cols: list of [t_r] arrays);
    end and cols are meaningful only where e <= h."""
    R, h = len(segs), 32 * c - 1
    B = 2 * h + 1
    n = np.array([len(s) for s in segs], np.int64)
    t = np.array([len(b) for b in sides], np.int64)
    nmax, tmax = int(n.max()), int(t.max())
    codes = np.full((R, nmax), 4, np.uint8)
    bpad = np.full((R, tmax + 1), 5, np.uint8)
    for r in range(R):
        codes[r, :n[r]] = segs[r]
        bpad[r, :t[r]] = sides[r]
    rows = np.arange(R)
    k = np.arange(B)[None, :]
    j = k - h
    D = np.where((j >= 0) & (j <= t[:, None]), j, C.INF).astype(np.int64)
    PTR = np.zeros((nmax, R, B), np.uint8)
    infcol = np.full((R, 1), C.INF, np.int64)
    for i in range(1, nmax + 1):
        j = i - h + k
        valid = (j >= 0) & (j <= t[:, None])
        bj = bpad[rows[:, None], np.where((j >= 1) & (j <= t[:, None]), j - 1, tmax)]
        diag = D + ((bj != codes[:, i - 1][:, None]) | (j < 1) | (j > t[:, None]))
        up = np.concatenate([D[:, 1:], infcol], axis=1) + 1
        T = np.where(valid, np.minimum(diag, up), C.INF)
        E = np.where(valid, k + np.minimum.accumulate(T - k, axis=1), C.INF)
        PTR[i - 1] = np.where(diag == E, 0, np.where(up == E, 1, 2))
        D = np.where((n >= i)[:, None], E, D)
    e = D.min(axis=1)
    kend = np.argmax(D == e[:, None], axis=1)
    end = n - h + kend
    cols = [np.full(t[r], NOT_COVERED, np.uint8) for r in range(R)]
    for r in range(R):
        if e[r] > h:
            continue
        i, jj = int(n[r]), int(end[r])
        while jj > 0:
            op = 2 if i == 0 else int(PTR[i - 1, r, jj - i + h])
            if op == 0:
                cols[r][jj - 1] = codes[r, i - 1]
                i, jj = i - 1, jj - 1
            elif op == 1:
                i -= 1
            else:
                cols[r][jj - 1] = C.DELETED
                jj -= 1
    return e, end, cols


def _align_banded(items, max_dist, stats, budget=1 << 26):
    """items = [(segment codes, side codes)] -> [(dist, end, col)] by the widening rule."""
    out = [None] * len(items)
    todo = {}
    for q, (s, b) in enumerate(items):
        todo.setdefault(start_class(len(s), max_dist), []).append(q)
    for ci, c in enumerate(C.CLASSES):
        h = 32 * c - 1
        idx = sorted(todo.pop(ci, []), key=lambda q: -len(items[q][0]))
        at = 0
        while at < len(idx):
            step = max(1, budget // (len(items[idx[at]][0]) * 64 * c))
            part = idx[at:at + step]
            at += step
            e, end, cols = _band_batch([items[q][0] for q in part], [items[q][1] for q in part], c)
            for x, q in enumerate(part):
                stats["aligned_%d" % (64 * c)] = stats.get("aligned_%d" % (64 * c), 0) + 1
                if e[x] <= min(h, max_dist):
                    out[q] = (int(e[x]), int(end[x]), cols[x])
                elif h < max_dist:
                    stats["widened"] = stats.get("widened", 0) + 1
                    todo.setdefault(ci + 1, []).append(q)
                else:
                    out[q] = (-1, 0, np.full(len(items[q][1]), NOT_COVERED, np.uint8))
    assert not todo
    return out


def phase_group(m, t_left, t_right, aligned, skip, min_count, min_share_pct, min_purity_pct, min_sites, max_sites,
                max_iter):
    """One group from its alignments: aligned[(row, side)] = (dist, end, col) for the segments of >= 1 base.
    -> dict(label [m], dist [m, 2], end [m, 2], res (8 ints), sites [S, 12], site_sym [S, m])."""
    t = t_left + t_right
    label = np.full(m, -1, np.int32)
    dist = np.full((m, 2), -2, np.int32)
    end = np.zeros((m, 2), np.int32)
    P = np.full((m, t), NOT_COVERED, np.uint8)
    for (r, side), (d, e, col) in aligned.items():
        dist[r, side], end[r, side] = d, e
        if side == 0:
            P[r, :t_left] = col
        else:
            P[r, t_left:] = col
    have = [r for r in range(m) if (dist[r] >= 0).any()]
    mv = len(have)
    P = P[have].reshape(mv, t)
    sites = []
    if mv:
        n = np.stack([(P == c).sum(axis=0) for c in range(4)], axis=1)          # [t, 4]
        cov = (P <= C.DELETED).sum(axis=0)
        for j in range(t):
            o = j if j < t_left else j - t_left
            a, bb = S._top2(n[j])
            na, nb = int(n[j, a]), int(n[j, bb])
            if (o >= skip and nb >= min_count and 100 * nb >= min_share_pct * (na + nb)
                    and 2 * (na + nb) >= int(cov[j])):
                sites.append((j, nb, a, bb))
        if len(sites) > max_sites:
            sites = sorted(sorted(sites, key=lambda s: (-s[1], s[0]))[:max_sites])
    ns = len(sites)
    cols = np.array([s[0] for s in sites], np.int64)
    ab = np.array([[s[2], s[3]] for s in sites], np.int64).reshape(ns, 2)
    M = P[:, cols].T.copy() if ns else np.zeros((0, mv), np.uint8)            # [site][row]
    lab = np.zeros(mv, np.int64)
    iters = 0
    if ns:
        anchor = min(range(ns), key=lambda q: (-sites[q][1], sites[q][0]))
        lab = np.where(M[anchor] == ab[anchor, 0], 0, np.where(M[anchor] == ab[anchor, 1], 1, UNDECIDED))
        shows = M < 4
        for _ in range(max_iter):
            iters += 1
            _, sym = S._hap_symbols(M, lab, ab)
            m0 = (shows & (M != sym[0][:, None])).sum(axis=0)
            m1 = (shows & (M != sym[1][:, None])).sum(axis=0)
            new = np.where(m0 < m1, 0, np.where(m1 < m0, 1, lab))
            same = np.array_equal(new, lab)
            lab = new
            if same:
                break
    cnt, sym = S._hap_symbols(M, lab, ab)
    n0, n1, und = int((lab == 0).sum()), int((lab == 1).sum()), int((lab == UNDECIDED).sum())
    if n1 > n0:
        lab = np.where(lab == 0, 1, np.where(lab == 1, 0, lab))
        cnt, sym, n0, n1 = cnt[::-1], sym[::-1], n1, n0
    out_sites = np.zeros((ns, 12), np.int32)
    n_sup = 0
    for q in range(ns):
        ok = sym[0, q] != sym[1, q]
        for hp in (0, 1):
            own, tot = int(cnt[hp, q, sym[hp, q]]), int(cnt[hp, q].sum())
            ok = ok and own > 0 and 100 * own >= min_purity_pct * tot
        n_sup += bool(ok)
        out_sites[q] = [cols[q], sym[0, q], sym[1, q], *cnt[0, q], *cnt[1, q], int(ok)]
    phased = int(n0 >= min_count and n1 >= min_count and n_sup >= min_sites)
    label[have] = lab
    site_sym = np.full((ns, m), NOT_COVERED, np.uint8)
    if ns:
        site_sym[:, have] = M
    return dict(label=label, dist=dist, end=end, res=np.array([phased, n0, n1, und, m - mv, ns, n_sup, iters], np.int32),
                sites=out_sites, site_sym=site_sym)


def ref_flank_phase(groups, backbones, device=0, banded=True, **kw):
    """Stand-in for _capi.flank_phase (same arguments, same result dict) on the CPU."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"flank_phase: unknown threshold(s) {sorted(unknown)}")
    p = dict(DEFAULTS, **kw)
    if len(groups) != len(backbones):
        raise ValueError("one pair of backbone sides per group")
    for name, hi in (("min_share_pct", 100), ("min_purity_pct", 100), ("max_sites", S.MAX_SITES_LIMIT), ("max_iter", 64),
                     ("min_count", 1 << 30), ("min_sites", 1 << 30)):
        if not 1 <= p[name] <= hi:
            raise ValueError(name + " out of range")
    if not 0 <= p["max_dist"] <= MAX_DIST or p["skip"] < 0:
        raise ValueError("max_dist or skip out of range")
    max_dist = p.pop("max_dist")
    stats = {}
    sides = [[C.encode(x or "") for x in bb] for bb in backbones]
    if any((b > 3).any() for bb in sides for b in bb):
        raise ValueError("backbone bases must be A, C, G or T")
    items, owner = [], []
    for g, rows in enumerate(groups):
        for r, row in enumerate(rows):
            for side in (0, 1):
                s = C.encode(row[side] or "")
                if len(s):
                    items.append((s, sides[g][side]))
                    owner.append((g, r, side))
    if banded:
        res = _align_banded(items, max_dist, stats) if items else []
    else:
        res = [align_full(s, b, max_dist) for s, b in items]
    per = [dict() for _ in groups]
    for (g, r, side), x in zip(owner, res):
        per[g][(r, side)] = x
    got = [phase_group(len(rows), len(sides[g][0]), len(sides[g][1]), per[g], **p) for g, rows in enumerate(groups)]
    r8 = np.array([x["res"] for x in got], np.int32).reshape(len(got), 8)
    out = {k: [x[k] for x in got] for k in FIELDS}
    out["stats"] = stats
    for q, name in enumerate(RES_FIELDS):
        out[name] = r8[:, q].copy()
    return out


def same_result(a, b):
    """Every field of two results but the stats."""
    return (len(a["label"]) == len(b["label"])
            and all(np.array_equal(a[k], b[k]) for k in RES_FIELDS)
            and all(x.shape == y.shape and np.array_equal(x, y) for k in FIELDS for x, y in zip(a[k], b[k])))
