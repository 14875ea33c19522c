"""Inputs that put every band class of the banded tract alignment (cons_band_align<C, FREE_END>, C = 1, 2, 4, 8, 16:
bands of 64 C diagonals) at its borders, for nra_allele_split, nra_tract_consensus and nra_flank_phase (the CPU and the
GPU test share them; DESIGN.md section 18.5 has the table).

A tract is a dict(seq, cls, dist): `cls` is the class (C) the case means it to be decided in (None: not claimed, e.g.
a tract ruled out by its length alone) and `dist` its true distance (None: not claimed, -1: left out).  A flank row is
the same with `side` (0 left, 1 right) and `end`.  Every claim is checked against the full matrix by
tests/test_band_borders_cpu.py, so a wrong label is an error of the case and fails there.

How one alignment is observed.  Exact edit counts: a base replaced by N (code 4 mismatches everything) costs exactly one
edit, d appended N make delta = t - n = -d, d bases cut from the end make delta = +d; the distance is the number of N
plus d.  The whole walked path: every group carries eight marker tracts, the backbone with every 8th column substituted
(one marker per residue), and is called with LOOSE thresholds, so that every backbone column is a variant site and
site_sym is the complete pileup row of every tract.
"""
import contextlib
import functools

import numpy as np

import consensus_ref as CR
import flank_ref as FR
import split_ref as SR
from consensus_cases import _rand, _mutate

CLASSES = (1, 2, 4, 8, 16)
# n = t that starts a tract in class C at the default max_dist (want = n / 6 + 8 against what the class below proves)
START_LEN = {1: 200, 2: 348, 4: 732, 8: 1500, 16: 3036}
LOOSE = dict(min_count=1, min_share_pct=1, min_sites=1, max_sites=4096)
MAX_PROBES = 8                   # per group (and flank side): with eight markers every column still passes 2 (na + nb) >= m_v
PTR_BYTES = "65536"              # NRA_TEST_CONS_PTR_BYTES of the routing test


def tract(seq, cls=None, dist=None):
    return dict(seq=seq, cls=cls, dist=dist)


def with_n(s, k, lo=0, hi=None):
    """s with k of the bases in [lo, hi) replaced by N, evenly spread: each costs exactly one edit."""
    hi = len(s) if hi is None else hi
    assert 0 <= k <= hi - lo
    out = list(s)
    for q in range(k):
        out[lo + q * (hi - lo) // k] = "N"
    return "".join(out)


def edits(b, k, delta):
    """b with k bases replaced by N and delta = t - n: -d appends d N, +d cuts d bases from the end.  Distance k + |delta|."""
    keep = len(b) - max(delta, 0)
    return with_n(b[:keep], k) + "N" * max(-delta, 0)


def markers(b):
    """Eight tracts: b with the columns of one residue mod 8 substituted.  Each is at distance about len(b) / 8."""
    out = []
    for r in range(8):
        s = list(b)
        for j in range(r, len(b), 8):
            s[j] = "ACGT"[("ACGT".index(s[j]) + 1 + j // 8 % 3) % 4]
        out.append("".join(s))
    return out


def _rng(C, salt):
    return np.random.default_rng(1000 * salt + C)


def _group(b, probes):
    assert len(probes) <= MAX_PROBES, len(probes)
    return dict(backbone=b, tracts=probes + [tract(m) for m in markers(b)], n_probes=len(probes))


def _fit(rng, s, n):
    """s cut or padded to n bases at random places."""
    s = list(s)
    while len(s) > n:
        del s[int(rng.integers(0, len(s)))]
    while len(s) < n:
        s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[int(rng.integers(0, 4))])
    return "".join(s)


# ---- family 1: the proven width.  n = t proves w = 64 C - 2; |delta| = 1 proves 64 C - 1 (extra even), |delta| = 2
# proves 64 C - 2 again (extra odd, h one less).

def proven_width(C, max_dist=CR.MAX_DIST):
    """One group on a backbone of START_LEN[C]: distances at w and around it for the given max_dist (the default, or
    w - 1, w, w + 1 of class C).  Class 16 proves 1022 > NRA_CONS_MAX_DIST: its border is max_dist itself."""
    b = _rand(_rng(C, 1), START_LEN[C])
    w, nxt = 64 * C - 2, 2 * C
    if C == 16:
        assert max_dist == CR.MAX_DIST
        return _group(b, [tract(edits(b, 1000, 0), 16, 1000), tract(edits(b, 1001, 0), 16, -1),
                          tract(edits(b, 999, -1), 16, 1000), tract(edits(b, 1000, -1), 16, -1),
                          tract(edits(b, 999, 1), 16, 1000), tract(edits(b, 1000, 1), 16, -1)])
    if max_dist == CR.MAX_DIST:
        p = [tract(edits(b, w, 0), C, w), tract(edits(b, w + 1, 0), nxt, w + 1)]
        for sign in (-1, 1):
            p += [tract(edits(b, w, sign), C, w + 1), tract(edits(b, w + 1, sign), nxt, w + 2),        # proves w + 1
                  tract(edits(b, w - 2, 2 * sign), C, w)]                                                # proves w
        return _group(b, p)
    if max_dist == w - 1:
        return _group(b, [tract(edits(b, w - 1, 0), C, w - 1), tract(edits(b, w, 0), C, -1),
                          tract(edits(b, w - 2, 1), C, w - 1), tract(edits(b, w - 1, -1), C, -1)])
    if max_dist == w:
        return _group(b, [tract(edits(b, w, 0), C, w), tract(edits(b, w + 1, 0), C, -1),
                          tract(edits(b, w - 1, -1), C, w), tract(edits(b, w, -1), C, -1),
                          tract(edits(b, w - 2, 2), C, w), tract(edits(b, w - 1, 2), C, -1)])
    assert max_dist == w + 1
    return _group(b, [tract(edits(b, w, 0), C, w), tract(edits(b, w + 1, 0), nxt, w + 1), tract(edits(b, w + 2, 0), nxt, -1),
                      tract(edits(b, w, -1), C, w + 1), tract(edits(b, w + 1, -1), C, -1),
                      tract(edits(b, w, 1), C, w + 1), tract(edits(b, w + 1, 1), C, -1)])


# ---- family 2: a band that barely holds both corners.  |delta| = 64 C - 1: h = 0, a band of pure indels, kend = 0
# (delta < 0) or 64 C - 1 (delta > 0: lane 63, cell C - 1).

def barely_holds(C, max_dist=CR.MAX_DIST):
    """Two groups (delta < 0, delta > 0) on a backbone of 64 C + 100.  max_dist = 64 C - 1: |delta| = 64 C - 1 is tried
    and decided in class C, 64 C - 3 with one, two, three more edits, 64 C - 2 starts in the next class (class C proves
    only 64 C - 2).  max_dist = 64 C - 2: |delta| = 64 C - 2 with h = 0, |delta| = 64 C - 1 is ruled out by length.
    Default: |delta| = 64 C goes to the next class.  Class 16 holds |delta| <= 1000 with h >= 11: 1000 and 999."""
    b = _rand(_rng(C, 2), 64 * C + 100)
    B, nxt = 64 * C, 2 * C
    groups = []
    for sign in (-1, 1):
        if C == 16:
            assert max_dist == CR.MAX_DIST
            p = [tract(edits(b, 0, sign * 1000), 16, 1000), tract(edits(b, 1, sign * 1000), 16, -1),
                 tract(edits(b, 1, sign * 999), 16, 1000), tract(edits(b, 2, sign * 999), 16, -1)]
        elif max_dist == B - 1:
            p = [tract(edits(b, 0, sign * (B - 1)), C, B - 1), tract(edits(b, 1, sign * (B - 1)), C, -1),
                 tract(edits(b, 1, sign * (B - 3)), C, B - 2), tract(edits(b, 2, sign * (B - 3)), C, B - 1),
                 tract(edits(b, 3, sign * (B - 3)), C, -1),
                 tract(edits(b, 0, sign * (B - 2)), nxt, B - 2), tract(edits(b, 1, sign * (B - 2)), nxt, B - 1)]
        elif max_dist == B - 2:
            p = [tract(edits(b, 0, sign * (B - 2)), C, B - 2), tract(edits(b, 1, sign * (B - 2)), C, -1),
                 tract(edits(b, 0, sign * (B - 1)), None, -1)]
        else:
            assert max_dist == CR.MAX_DIST
            p = [tract(edits(b, 0, sign * B), nxt, B), tract(edits(b, 3, sign * B), nxt, B + 3)]
        groups.append(_group(b, p))
    return groups


# ---- family 3: a path that touches the outermost diagonal of the band and comes back

def excursions(C):
    """n = t (band columns 0 .. 64 C - 1 are the diagonals -(32 C - 1) .. 32 C): h N inserted near the start and h
    backbone bases dropped near the end (down to diagonal -h), and the mirror image (up to +h), h = 32 C - 1 (column 0 /
    the proven width exactly) and 32 C (must widen).  |delta| = 1 reaches the other edge: delta = +1 up to diagonal
    32 C = column 64 C - 1, delta = -1 down to -32 C = column 0, both at distance 64 C - 1, what the band proves.  Class
    16: 400 and 500 (within max_dist), on a backbone long enough that the excursion is the cheapest path.  The distances
    are claimed from the construction and checked on the full matrix."""
    t = START_LEN[C]
    b = _rand(_rng(C, 1 if C == 16 else 3), t)    # class 16: the backbone of proven_width, whose markers are aligned already
    h = 32 * C - 1

    def down(x, y):                               # x N inserted after column 20, y bases dropped before the last 20
        return b[:20] + "N" * x + b[20:t - 20 - y] + b[t - 20:]

    def up(x, y):                                 # y bases dropped after column 20, x N inserted before the last 20
        return b[:20] + b[20 + y:t - 20] + "N" * x + b[t - 20:]

    if C == 16:
        p = [tract(f(x, x), 16, 2 * x) for x in (400, 500) for f in (down, up)]
        return _group(b, p)
    nxt = 2 * C
    return _group(b, [tract(down(h, h), C, 2 * h), tract(up(h, h), C, 2 * h),
                      tract(down(h + 1, h + 1), nxt, 2 * h + 2), tract(up(h + 1, h + 1), nxt, 2 * h + 2),
                      tract(up(h, h + 1), C, 2 * h + 1), tract(down(h + 1, h), C, 2 * h + 1)])


# ---- family 4: rows per 16-byte pointer piece (R = 64 / C), per staged tile (64), columns per 16-byte row piece (16)

ROW_SHAPES = {1: ((191, 192, 193), (191, 192, 193)),                       # C: (n values, t values)
              2: ((351, 352, 353, 383, 384, 385), (367, 368, 369)),
              4: ((735, 736, 737, 767, 768, 769), (751, 752, 753)),
              8: ((1519, 1520, 1521, 1535, 1536, 1537), (1535, 1536, 1537)),
              16: ((1023, 1024, 1025, 1026), (1023, 1024, 1025))}


def piece_and_tile_rows(C):
    """Three groups (t = 16 m - 1, 16 m, 16 m + 1), each with a tract of every n in {R m - 1, R m, R m + 1} and
    {64 m - 1, 64 m, 64 m + 1}; every tract carries a few real indels, so the walk changes lanes and pieces.  Class 16
    (R = 4: all four residues) is reached by widening: its tracts carry 520 N as well, beyond what class 8 proves."""
    rng = _rng(C, 4)
    ns, ts = ROW_SHAPES[C]
    groups = []
    for t in ts:
        b = _rand(rng, t)
        p = []
        for n in ns:
            s = _fit(rng, _mutate(rng, b, 5), n)
            p.append(tract(with_n(s, 520) if C == 16 else s, C))
        groups.append(_group(b, p))
    return groups


# ---- the calls of one class for allele_split and tract_consensus

def split_max_dists(C):
    return (CR.MAX_DIST,) if C == 16 else (CR.MAX_DIST, 64 * C - 3, 64 * C - 2, 64 * C - 1)


def split_groups(C, max_dist):
    """The groups of class C that are called with this max_dist (split_max_dists(C) lists the values)."""
    g = [proven_width(C, max_dist)]
    if max_dist == CR.MAX_DIST:
        g += barely_holds(C) + [excursions(C)] + piece_and_tile_rows(C)
    elif C < 16 and max_dist >= 64 * C - 2:
        g += barely_holds(C, max_dist)
    return g


def split_call(groups, max_dist):
    """-> (groups, backbones, thresholds) of _capi.allele_split."""
    return [[x["seq"] for x in g["tracts"]] for g in groups], [g["backbone"] for g in groups], dict(LOOSE, max_dist=max_dist)


def consensus_groups(groups):
    """[b, b, b, b, s, s', b] for the probes of every group, two at a time (the median tract by (length, position), the
    round-0 backbone, is then a copy of b whatever the lengths of s and s').  -> (groups of strings, labelled tracts)."""
    out, labelled = [], []
    for g in groups:
        b, p = g["backbone"], g["tracts"][:g["n_probes"]]
        for q in range(0, len(p), 2):
            pair = p[q:q + 2]
            mine = [tract(b, None, 0)] * 4 + pair + [tract(b, None, 0)] * (7 - 4 - len(pair))
            out.append([x["seq"] for x in mine])
            labelled.append(dict(backbone=b, tracts=mine))
    return out, labelled


# ---- family 5: the flanks (FREE_END): band j - i in [-h, h + 1], h = 32 C - 1, proves e <= h

def _row(seq, side, cls=None, dist=None, end=None):
    return dict(seq=seq, side=side, cls=cls, dist=dist, end=end)


def _side(rng, t):
    """A side whose last five bases differ from their neighbours: a marker substituted next to the free end then cannot
    end one column early at the same cost (the smaller column would win and take the last columns out of the sites)."""
    s = _rand(rng, t - 4)
    at = "ACGT".index(s[-1]) + 1
    return s + ("ACGT" * 2)[at:at + 4]


def flank_max_dists(C):
    return (FR.MAX_DIST,) if C == 16 else (FR.MAX_DIST, 32 * C - 1)


def flank_groups(C, max_dist=FR.MAX_DIST):
    """Two groups.  On sides of up to 600 columns: e = h and h + 1 (class 16: 500 and 501 at max_dist 500); a free end
    whose minimum ties between two columns (a trailing N: inserted after column n - 1 or aligned to column n; the smaller
    wins) at e = 24 C; j* = 16 m - 1, 16 m, 16 m + 1 at e = 20 C; rows with real indels.  On sides of 100 columns:
    segments longer than their side by h and by h + 1 (row n below the band).  With max_dist = h the h + 1 cases are
    left out in class C instead of widened.  Segments start in class 1 or 2 and reach class C by widening."""
    rng = _rng(C, 5)
    h = 32 * C - 1
    nxt = 2 * C
    top = C == 16 or max_dist == h                       # nothing beyond class C: e > min(h, max_dist) is left out
    lim = min(h, max_dist)                               # class 16: 500
    tl = min(600, 8 * max_dist)                          # a marker's distance is t / 8
    sides = (_side(rng, tl), _side(rng, tl))
    n0 = min(tl - 40, 560)
    rows = []
    for side in (0, 1):
        s = sides[side]
        rows += [_row(with_n(s[:n0], lim, hi=n0 - 40), side, C, lim, n0),
                 _row(with_n(s[:n0], lim + 1, hi=n0 - 40), side, C if top else nxt, -1 if top else lim + 1, 0 if top else n0)]
    if max_dist == FR.MAX_DIST:
        n1 = min(tl - 40, 480)
        rows += [_row(with_n(sides[0][:n1], 24 * C - 1, hi=n1 - 40) + "N", 0, C, 24 * C, n1),
                 _row(with_n(sides[1][:n1 + 7], 24 * C - 1, hi=n1 - 40) + "N", 1, C, 24 * C, n1 + 7)]
        for q, n in enumerate((415, 416, 417)):
            rows.append(_row(with_n(sides[q % 2][:n], 20 * C, hi=n - 40), q % 2, C, 20 * C, n))
        for side in (0, 1):
            rows.append(_row(_mutate(rng, with_n(sides[side][:500], 20 * C), 6), side, C))
    per_side = [sum(1 for r in rows if r["side"] == side) for side in (0, 1)]
    assert max(per_side) <= MAX_PROBES
    g1 = dict(sides=sides, rows=rows + [_row(m, side) for side in (0, 1) for m in markers(sides[side])])
    short = (_side(rng, 100), _side(rng, 100))
    rows = []
    for side in (0, 1):
        s = short[side]
        rows += [_row(s + "N" * lim, side, C, lim, 100),
                 _row(s + "N" * (lim + 1), side, C if top else nxt, -1 if top else lim + 1, 0 if top else 100),
                 _row(with_n(s, 3) + "N" * (lim - 3), side, C, lim, 100)]
    if C == 16:                                          # row n below even the widest band: h = 511 >= max_dist
        rows.append(_row(short[0] + "N" * 512, 0, 16, -1, 0))
    g2 = dict(sides=short, rows=rows + [_row(m, side) for side in (0, 1) for m in markers(short[side])])
    return [g1, g2]


def flank_call(groups, max_dist):
    """-> (groups, backbones, thresholds) of _capi.flank_phase: one segment per row, the other side absent."""
    return ([[(r["seq"], "") if r["side"] == 0 else ("", r["seq"]) for r in g["rows"]] for g in groups],
            [g["sides"] for g in groups], dict(LOOSE, skip=0, max_dist=max_dist))


# ---- family 6: host routing.  The default-max_dist groups of every class in one call, the tracts of a group shuffled.

def shuffled(groups, key, seed=6):
    """-> (the groups with their `key` lists permuted, the permutations)."""
    rng = np.random.default_rng(seed)
    out, perms = [], []
    for g in groups:
        p = rng.permutation(len(g[key]))
        out.append(dict(g, **{key: [g[key][i] for i in p]}))
        perms.append(p)
    return out, perms


# ---- the routes the widening rule takes, from the true distances (the CPU test holds the labels against them)

def split_route(n, t, dist, max_dist):
    """The classes (C values) the rule of nra_cons_host.h / cons_band_align runs a tract of true distance `dist` in.
    -> (classes, accepted); no class when |t - n| alone rules the tract out."""
    if abs(t - n) > max_dist:
        return [], False
    ci = CR.start_class(n, t, max_dist)
    run = []
    while True:
        c = CLASSES[ci]
        run.append(c)
        w = CR.proven(c, n, t)
        if dist <= min(w, max_dist):
            return run, True
        if w >= max_dist:
            return run, False
        ci += 1


def flank_route(n, e, max_dist):
    """As split_route for a flank segment of n bases whose free-end distance is e."""
    ci = FR.start_class(n, max_dist)
    run = []
    while True:
        c = CLASSES[ci]
        run.append(c)
        h = 32 * c - 1
        if e <= min(h, max_dist):
            return run, True
        if h >= max_dist:
            return run, False
        ci += 1


def route_stats(routes):
    """aligned_<64 C> and widened of a list of routes (tuples that end in classes, accepted), as the stats of the
    restatements and of the device count them."""
    st = {}
    for run in (r[-2] for r in routes):
        for c in run:
            st["aligned_%d" % (64 * c)] = st.get("aligned_%d" % (64 * c), 0) + 1
        if len(run) > 1:
            st["widened"] = st.get("widened", 0) + len(run) - 1
    return st


CLASS_STATS = ("aligned_64", "aligned_128", "aligned_256", "aligned_512", "aligned_1024", "widened")


def class_stats(st):
    return {k: st.get(k, 0) for k in CLASS_STATS}


def true_dist(s, b):
    """D[n][t] of the full matrix (remembered)."""
    with shared_full_matrix():
        return CR.align_full(CR.encode(s), CR.encode(b))[0]


def split_routes(groups, max_dist):
    """[(tract, true distance, classes, accepted)] of every tract of the groups (dicts with backbone and tracts), in order."""
    out = []
    for g in groups:
        b = g["backbone"]
        for x in g["tracts"]:
            d = true_dist(x["seq"], b)
            out.append((x, d) + split_route(len(x["seq"]), len(b), d, max_dist))
    return out


def flank_routes(groups, full, max_dist):
    """[(row, dist, end, classes, accepted)] of every row of the flank groups, from the full-matrix result of their call."""
    out = []
    for g, grp in enumerate(groups):
        for r, x in enumerate(grp["rows"]):
            d, e = int(full["dist"][g][r, x["side"]]), int(full["end"][g][r, x["side"]])
            out.append((x, d, e) + flank_route(len(x["seq"]), d if d >= 0 else max_dist + 1, max_dist))
    return out


@contextlib.contextmanager
def shared_full_matrix():
    """While open, the full-matrix alignments of consensus_ref and flank_ref remember their results by (tract, backbone):
    the markers and the copies of the backbone recur in every call of a class, and each is filled once."""
    cons, flank = CR.align_full, FR.align_full
    mc, mf = _MEMO.setdefault("cons", {}), _MEMO.setdefault("flank", {})

    def cons_cached(s, b):
        k = (s.tobytes(), b.tobytes())
        if k not in mc:
            mc[k] = cons(s, b)
        d, col, ins = mc[k]
        return d, col.copy(), ins.copy()

    def flank_cached(s, b, max_dist):
        k = (s.tobytes(), b.tobytes(), max_dist)
        if k not in mf:
            mf[k] = flank(s, b, max_dist)
        d, e, col = mf[k]
        return d, e, col.copy()

    CR.align_full, FR.align_full = cons_cached, flank_cached
    try:
        yield
    finally:
        CR.align_full, FR.align_full = cons, flank


_MEMO = {}


# ---- the calls with their full-matrix references, computed once per process and shared by the tests of a module

@functools.lru_cache(maxsize=None)
def split_case(C, max_dist):
    """-> (labelled groups, (groups, backbones, thresholds), ref_allele_split(banded=False))"""
    groups = split_groups(C, max_dist)
    call = split_call(groups, max_dist)
    with shared_full_matrix():
        full = SR.ref_allele_split(call[0], call[1], banded=False, **call[2])
    return groups, call, full


@functools.lru_cache(maxsize=None)
def consensus_case(C, max_dist, max_rounds):
    """-> (labelled groups, groups of strings, ref_tract_consensus(banded=False))"""
    groups, labelled = consensus_groups(split_groups(C, max_dist))
    with shared_full_matrix():
        full = CR.ref_tract_consensus(groups, max_dist=max_dist, max_rounds=max_rounds, banded=False)
    return labelled, groups, full


@functools.lru_cache(maxsize=None)
def flank_case(C, max_dist):
    """-> (labelled groups, (groups, backbones, thresholds), ref_flank_phase(banded=False))"""
    groups = flank_groups(C, max_dist)
    call = flank_call(groups, max_dist)
    with shared_full_matrix():
        full = FR.ref_flank_phase(call[0], call[1], banded=False, **call[2])
    return groups, call, full


def by_length(groups, max_dist):
    """The tracts |t - n| > max_dist rules out before any alignment: the device's left_out_by_length."""
    return sum(1 for g in groups for x in g["tracts"] if abs(len(g["backbone"]) - len(x["seq"])) > max_dist)


def concat(outs, res_fields, list_fields):
    """The results of several calls as the result of one call over all their groups."""
    out = {k: [x for o in outs for x in o[k]] for k in list_fields}
    out.update({k: np.concatenate([o[k] for o in outs]) for k in res_fields})
    return out


def permuted(out, perms, row_fields, list_fields, res_fields):
    """A split or flank result as it reads when the rows of group g are given in the order perms[g]: the rule counts
    rows and breaks ties by code and column, never by row order."""
    got = {k: out[k] for k in res_fields}
    for k in list_fields:
        got[k] = [x[p] if k in row_fields else x[:, p] if k == "site_sym" else x for x, p in zip(out[k], perms)]
    return got


SPLIT_FIELDS = ("label", "dist", "sites", "site_sym")


def routing_split():
    """-> (groups, perms, full-matrix result): the default-max_dist groups of every class, the tracts of each shuffled."""
    cases = [split_case(C, CR.MAX_DIST) for C in CLASSES]
    mixed, perms = shuffled([g for c in cases for g in c[0]], "tracts")
    want = concat([c[2] for c in cases], SR.RES_FIELDS, SPLIT_FIELDS)
    return mixed, perms, permuted(want, perms, ("label", "dist"), SPLIT_FIELDS, SR.RES_FIELDS)


def routing_flank():
    """As routing_split for the flank groups at the default max_dist, the rows of each shuffled."""
    cases = [flank_case(C, FR.MAX_DIST) for C in CLASSES]
    mixed, perms = shuffled([g for c in cases for g in c[0]], "rows")
    want = concat([c[2] for c in cases], FR.RES_FIELDS, FR.FIELDS)
    return mixed, perms, permuted(want, perms, ("label", "dist", "end"), FR.FIELDS, FR.RES_FIELDS)


def routing_consensus(max_rounds=2, seed=6):
    """-> (groups of strings, full-matrix result): the default-max_dist consensus groups of every class in a shuffled
    order (a group's own order decides its round-0 backbone and stays)."""
    cases = [consensus_case(C, CR.MAX_DIST, max_rounds) for C in CLASSES]
    groups = [g for c in cases for g in c[1]]
    order = np.random.default_rng(seed).permutation(len(groups))
    want = {k: [x for c in cases for x in c[2][k]] for k in ("consensus", "support")}
    want.update({k: np.concatenate([c[2][k] for c in cases]) for k in ("n_rounds", "converged", "voted", "left_out")})
    got = {k: [want[k][i] for i in order] for k in ("consensus", "support")}
    got.update({k: want[k][order] for k in ("n_rounds", "converged", "voted", "left_out")})
    return [groups[i] for i in order], got
