"""The allele-split contract (include/nanorepeat_amd.h) restated for the tests, twice:
`ref_allele_split(..., banded=False)` aligns every tract in the full matrix; `banded=True` aligns inside bands of 64 c
diagonals with the widening rule of the device (tests/consensus_ref.py has both alignments).  Both are stand-ins for
_capi.allele_split: same arguments, same result (the `stats` apart).

Contract, in short.  Per group: tracts coded as for the consensus (ACGT -> 0..3, other -> 4; empty tracts stay), one
backbone of A C G T.  Step 1: a tract at distance <= max_dist gets a row sym[j] in {0..3 base, 4 abstains, 5 deleted}
over the backbone columns; the others are left out (label -1, distance -1).  Step 2: per column the base counts n[c]
over the m_v rows, a = most voted, b = second (ties: smaller code); a site iff n[b] >= min_count and
100 n[b] >= min_share_pct (n[a] + n[b]) and 2 (n[a] + n[b]) >= m_v; beyond max_sites the largest n[b] stay (ties:
smaller column); sites in column order.  Step 3: anchor = the site of largest n[b] (smaller column); labels 0 / 1 /
undecided (2) from a / b / anything else at the anchor; up to max_iter times: haplotype symbols per site = the most voted
base of its reads (ties: smaller code; nobody shows a base: a for 0, b for 1), every row's mismatches against either
haplotype over the sites where it shows a base, fewer wins, a tie keeps the label; stop when nothing changes.  No site:
every row is label 0.  Step 4: with the symbols and counts of the final labels, a site is supported when the symbols
differ and in each haplotype at least one read shows its symbol and 100 * (reads showing it) >= min_purity_pct * (reads
showing a base); split iff both haplotypes have >= min_count reads and >= min_sites sites are supported; haplotype 0 is
the one with more reads (a tie keeps the start).
"""
import numpy as np

import consensus_ref as C

MAX_SITES_LIMIT = 4096
UNDECIDED, NO_ROW = 2, 6
DEFAULTS = dict(max_dist=C.MAX_DIST, min_count=3, min_share_pct=25, min_purity_pct=75, min_sites=1, max_sites=256,
                max_iter=16)


def _rows_full(codes, b, max_dist, stats):
    out = []
    for s in codes:
        d, col, _ = C.align_full(s, b)
        out.append((d, col.astype(np.uint8)) if d <= max_dist else None)
    return out


def _rows_banded(codes, b, max_dist, stats, budget=1 << 27):
    """consensus_ref's widening rule, keeping the distance (and taking empty tracts)."""
    t = len(b)
    out = [None] * len(codes)
    todo = {}
    for r, s in enumerate(codes):
        if len(s) == 0 and t <= max_dist:        # every column deleted, whatever the band
            out[r] = (t, np.full(t, C.DELETED, np.uint8))
        elif abs(t - len(s)) <= max_dist:
            todo.setdefault(C.start_class(len(s), t, max_dist), []).append(r)
    for ci, c in enumerate(C.CLASSES):
        idx = sorted(todo.pop(ci, []), key=lambda r: -len(codes[r]))
        at = 0
        while at < len(idx):
            step = max(1, budget // (max(1, len(codes[idx[at]])) * 64 * c))
            part = idx[at:at + step]
            at += step
            dist, col, _ = C._band_batch([codes[r] for r in part], b, c)
            for q, r in enumerate(part):
                w = C.proven(c, len(codes[r]), t)
                stats["aligned_%d" % (64 * c)] = stats.get("aligned_%d" % (64 * c), 0) + 1
                if dist[q] <= min(w, max_dist):
                    out[r] = (int(dist[q]), col[q].astype(np.uint8))
                elif w < max_dist:
                    stats["widened"] = stats.get("widened", 0) + 1
                    todo.setdefault(ci + 1, []).append(r)
    assert not todo
    return out


def _top2(n):
    """(a, b) of four counts: the most voted and the second, ties to the smaller code."""
    a = int(np.argmax(n))
    rest = [(-int(n[c]), c) for c in range(4) if c != a]
    return a, min(rest)[1]


def _hap_symbols(M, labels, ab):
    """counts [2, S, 4] over the rows labelled 0 / 1, symbols [2, S]."""
    S = M.shape[0]
    cnt = np.zeros((2, S, 4), np.int64)
    for h in (0, 1):
        sel = M[:, labels == h]
        for c in range(4):
            cnt[h, :, c] = (sel == c).sum(axis=1)
    sym = cnt.argmax(axis=2)
    for h in (0, 1):
        none = cnt[h].sum(axis=1) == 0
        sym[h, none] = ab[none, h]
    return cnt, sym


def split_group(tracts, backbone, max_dist, min_count, min_share_pct, min_purity_pct, min_sites, max_sites, max_iter,
                banded=True, stats=None):
    """One group -> dict(label [m], dist [m], res (8 ints), sites [S, 12], site_sym [S, m])."""
    stats = {} if stats is None else stats
    b = C.encode(backbone)
    if (b > 3).any():
        raise ValueError("backbone bases must be A, C, G or T")
    codes = [C.encode(t) for t in tracts]
    m, t = len(codes), len(b)
    rows = (_rows_banded if banded else _rows_full)(codes, b, max_dist, stats) if m else []
    label = np.full(m, -1, np.int32)
    dist = np.full(m, -1, np.int32)
    have = [r for r in range(m) if rows[r] is not None]
    for r in have:
        dist[r] = rows[r][0]
    mv = len(have)
    P = np.array([rows[r][1] for r in have], np.uint8).reshape(mv, t)
    # step 2
    sites = []
    if mv:
        n = np.stack([(P == c).sum(axis=0) for c in range(4)], axis=1)          # [t, 4]
        for j in range(t):
            a, bb = _top2(n[j])
            na, nb = int(n[j, a]), int(n[j, bb])
            if nb >= min_count and 100 * nb >= min_share_pct * (na + nb) and 2 * (na + nb) >= mv:
                sites.append((j, nb, a, bb))
        if len(sites) > max_sites:
            keep = sorted(sites, key=lambda s: (-s[1], s[0]))[:max_sites]
            sites = sorted(keep)
    S = len(sites)
    cols = np.array([s[0] for s in sites], np.int64)
    ab = np.array([[s[2], s[3]] for s in sites], np.int64).reshape(S, 2)
    M = P[:, cols].T.copy() if S else np.zeros((0, mv), np.uint8)            # [site][row]
    lab = np.zeros(mv, np.int64)
    iters = 0
    if S:
        anchor = min(range(S), key=lambda q: (-sites[q][1], sites[q][0]))
        lab = np.where(M[anchor] == ab[anchor, 0], 0, np.where(M[anchor] == ab[anchor, 1], 1, UNDECIDED))
        shows = M < 4
        for _ in range(max_iter):
            iters += 1
            _, sym = _hap_symbols(M, lab, ab)
            m0 = (shows & (M != sym[0][:, None])).sum(axis=0)
            m1 = (shows & (M != sym[1][:, None])).sum(axis=0)
            new = np.where(m0 < m1, 0, np.where(m1 < m0, 1, lab))
            same = np.array_equal(new, lab)
            lab = new
            if same:
                break
    # step 4
    cnt, sym = _hap_symbols(M, lab, ab)
    n0, n1, und = int((lab == 0).sum()), int((lab == 1).sum()), int((lab == UNDECIDED).sum())
    if n1 > n0:
        lab = np.where(lab == 0, 1, np.where(lab == 1, 0, lab))
        cnt, sym, n0, n1 = cnt[::-1], sym[::-1], n1, n0
    out_sites = np.zeros((S, 12), np.int32)
    n_sup = 0
    for q in range(S):
        ok = sym[0, q] != sym[1, q]
        for h in (0, 1):
            own, tot = int(cnt[h, q, sym[h, q]]), int(cnt[h, q].sum())
            ok = ok and own > 0 and 100 * own >= min_purity_pct * tot
        n_sup += bool(ok)
        out_sites[q] = [cols[q], sym[0, q], sym[1, q], *cnt[0, q], *cnt[1, q], int(ok)]
    split = int(n0 >= min_count and n1 >= min_count and n_sup >= min_sites)
    label[have] = lab
    site_sym = np.full((S, m), NO_ROW, np.uint8)
    if S:
        site_sym[:, have] = M
    return dict(label=label, dist=dist, res=np.array([split, n0, n1, und, m - mv, S, n_sup, iters], np.int32),
                sites=out_sites, site_sym=site_sym)


RES_FIELDS = ("split", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations")


def ref_allele_split(groups, backbones, device=0, banded=True, **kw):
    """Stand-in for _capi.allele_split (same arguments, same result dict) on the CPU."""
    p = dict(DEFAULTS, **kw)
    if len(groups) != len(backbones):
        raise ValueError("one backbone per group")
    for name, hi in (("min_share_pct", 100), ("min_purity_pct", 100), ("max_sites", MAX_SITES_LIMIT), ("max_iter", 64),
                     ("min_count", 1 << 30), ("min_sites", 1 << 30)):
        if not 1 <= p[name] <= hi:
            raise ValueError(name + " out of range")
    if not 0 <= p["max_dist"] <= C.MAX_DIST:
        raise ValueError("max_dist out of range")
    stats = {}
    got = [split_group(list(g), bb, banded=banded, stats=stats, **p) for g, bb in zip(groups, backbones)]
    res = np.array([g["res"] for g in got], np.int32).reshape(len(got), 8)
    out = dict(label=[g["label"] for g in got], dist=[g["dist"] for g in got], sites=[g["sites"] for g in got],
               site_sym=[g["site_sym"] for g in got], stats=stats)
    for q, name in enumerate(RES_FIELDS):
        out[name] = res[:, q].copy()
    return out


def same_result(a, b):
    """Every field of two results but the stats."""
    return (len(a["label"]) == len(b["label"])
            and all(np.array_equal(a[k], b[k]) for k in RES_FIELDS)
            and all(np.array_equal(x, y) for k in ("label", "dist", "sites", "site_sym") for x, y in zip(a[k], b[k])))
