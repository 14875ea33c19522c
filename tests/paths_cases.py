"""Cases shared by test_paths_cpu.py and test_paths_gpu.py: a small panel for the round-3 alignment file and the
checks of a PAF row against its CIGAR."""
import os
import re

import numpy as np

from nanorepeat_amd import paf as P, synth


def paths_panel(long_units=0, reads_per_allele=3, anchor_len=500, seed=17):
    """Three regions on one chromosome, two alleles each, `reads_per_allele` hifi reads an allele, half of them
    reverse-complemented: GAA (20 units, and `long_units` when given, else 45), CAG (17 / 36), TATTG (12 / 30)."""
    rng = np.random.default_rng(seed)
    loci = [("GAA", (20, long_units or 45), 20), ("CAG", (17, 36), 20), ("TATTG", (12, 30), 16)]
    gap, extra = 3000, 600
    parts, regions, at = [], [], 0
    for unit, _, ref_k in loci:
        left, right = synth.rand_seq(rng, anchor_len + extra), synth.rand_seq(rng, anchor_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(unit) * ref_k, unit))
        parts += [synth.rand_seq(rng, gap), left, unit * ref_k, right]
        at += gap + len(left) + len(unit) * ref_k + len(right)
    parts.append(synth.rand_seq(rng, gap))
    chrom = "".join(parts)
    reads = []
    for g, ((unit, alleles, _), (_, st, en, _)) in enumerate(zip(loci, regions)):
        for a, k in enumerate(alleles):
            for i in range(reads_per_allele):
                lo, ro = anchor_len + int(rng.integers(0, 200)), anchor_len + int(rng.integers(0, 200))
                s = synth.apply_errors(rng, chrom[st - lo:st] + unit * k + chrom[en:en + ro], "hifi")
                reads.append((f"p{g}_{a}_{i}", synth.revcomp(s) if (i + a) % 2 else s))
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads)


def paf_rows(path):
    """[(PAF, rs tag value)] of an alignment file."""
    rows = []
    for line in open(path):
        cols = line.rstrip("\n").split("\t")
        rs = [c for c in cols if c.startswith("rs:f:")]
        assert len(rs) == 1, line
        rows.append((P.PAF(cols), rs[0][5:]))
    return rows


def spans_fit_cigar(p):
    """The query and target spans of a row are what its CIGAR consumes."""
    q = t = 0
    for op, n in P.cigar_ops(p.cigar):
        if op in "=X":
            q += n; t += n
        elif op == "I":
            q += n
        elif op == "D":
            t += n
    return q == p.qend - p.qstart and t == p.tend - p.tstart and 0 <= p.qstart and p.qend <= p.qlen and \
        0 <= p.tstart and p.tend <= p.tlen


# ---- cases for the alignment paths: test_path_check_cpu.py (oracle) and test_path_forms_gpu.py (device) ------------------
#
# A pair is a dict(name, q, t) with, where a builder plants something, what it planted (`planted`, `tstart`, `tend`,
# ...).  Every builder is seeded and asserts under the oracle's score that the pairs meant to give a record do.

DEFAULT_SCHEME = dict(match=2, mismatch=4, gap_open1=4, gap_ext1=2, gap_open2=24, gap_ext2=1, sc_ambi=1, min_dp_score=0)

# (name, overrides of the default scheme); every entry with min_dp_score = 0
SCHEMES = (
    ("default", {}),
    ("all_ties", dict(match=1, mismatch=1, gap_open1=0, gap_ext1=1, gap_open2=0, gap_ext2=1)),
    ("equal_pieces", dict(gap_open2=4, gap_ext2=2)),                 # E ties E2 (and F ties F2) in every cell
    ("mismatch0", dict(mismatch=0)),
    ("ambi0", dict(sc_ambi=0)),
    ("ambi64", dict(sc_ambi=64)),
    ("pieces_swapped", dict(gap_open1=30, gap_ext1=1, gap_open2=4, gap_ext2=2)),
    ("knee16", dict(match=3, mismatch=8, gap_open1=7, gap_ext1=3, gap_open2=39, gap_ext2=1)),
    ("match64", dict(match=64)),
)


def scheme_values(over):
    """The eight values of a scheme given as overrides of the default one (min_dp_score 0)."""
    assert set(over) <= set(DEFAULT_SCHEME), over
    return dict(DEFAULT_SCHEME, **over)


def scheme_in_range(v):
    """What the library accepts as scoring (scoring_ok in nra_host.cpp), restated."""
    return 0 < v["match"] <= 64 and 0 <= v["mismatch"] <= 64 and v["gap_ext1"] > 0 and v["gap_ext2"] > 0 and \
        v["gap_open1"] >= 0 and v["gap_open2"] >= 0 and v["gap_open1"] + v["gap_ext1"] <= 1024 and \
        v["gap_open2"] + v["gap_ext2"] <= 1024 and 0 <= v["sc_ambi"] <= 64


def gap_cost(l, v):
    return min(v["gap_open1"] + l * v["gap_ext1"], v["gap_open2"] + l * v["gap_ext2"])


def knee_of(v):
    """The gap length at which the two pieces cost the same; 20 (the default scheme's) where they never cross."""
    if v["gap_ext1"] == v["gap_ext2"]:
        return 20
    return abs(v["gap_open2"] - v["gap_open1"]) // abs(v["gap_ext1"] - v["gap_ext2"])


def has_n(pair):
    return bool(re.search("[^ACGTacgt]", pair["q"] + pair["t"]))


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def _records(pairs, over):
    """Asserts that every pair gives a record under the scheme (score >= max(1, min_dp_score) = 1)."""
    O = _oracle()
    sc = O.default_scoring(**scheme_values(over))
    for p in pairs:
        assert p["q"] and p["t"] and O.align(p["q"], p["t"], sc)[0] >= 1, p["name"]
    return pairs


def _with_n(s, at, n=1):
    return s[:at] + "N" * n + s[at + n:]


REPEAT_UNITS = ("A", "AT", "CAG", "CCTG", "TATTG", "GGCCCC")
REPEAT_DELTAS = (-21, -20, -19, -7, -1, 0, 1, 7, 19, 20, 21)        # bases


def repeat_panel(over):
    """L + unit^k + R against the last 40 bases of L + unit^(k + d) + the first 40 of R, unit lengths 1 .. 6: the d
    (in bases, rounded to whole units, the unit count floored at 0) sit on both sides of the l = 20 knee, each query once
    exact and once with ont errors; N in the query, in the target or in both on half of the pairs; one query in lower
    case.  Where the surplus or missing units go inside the repeat is tie-breaking alone."""
    rng = np.random.default_rng(20260501)
    pairs = []
    for unit in REPEAT_UNITS:
        m = len(unit)
        L, R = synth.rand_seq(rng, 60), synth.rand_seq(rng, 60)
        k = -(-24 // m) + 1
        t = L + unit * k + R
        for du in sorted({int(np.sign(d)) * max(1, int(abs(d) / m + 0.5)) for d in REPEAT_DELTAS}):
            exact = L[-40:] + unit * max(0, k + du) + R[:40]
            for model in (None, "ont"):
                q, tt = (synth.apply_errors(rng, exact, model) if model else exact), t
                i = len(pairs)
                if i % 6 in (1, 5):
                    q = _with_n(q, int(rng.integers(0, len(q) - 3)), 1 + i % 3)
                if i % 6 in (3, 5):
                    tt = _with_n(tt, int(rng.integers(0, len(tt) - 2)), 1 + i % 2)
                if i == 4:
                    q = q.lower()
                pairs.append(dict(name=f"repeat:{unit}:k={k}:d={du}:{model or 'exact'}", q=q, t=tt))
    assert sum(p["q"].islower() for p in pairs) == 1
    kinds = {(bool(re.search("[^ACGTacgt]", p["q"])), bool(re.search("[^ACGTacgt]", p["t"]))) for p in pairs}
    assert len(kinds) == 4, kinds
    return _records(pairs, over)


def knee_pairs(over):
    """An insertion and a deletion of knee - 1 .. knee + 2 bases between random flanks long enough that bridging the gap
    beats keeping one flank alone (match * |flank| > g(l), the rule of test_oracle_independent._cases)."""
    v = scheme_values(over)
    rng = np.random.default_rng(20260502)
    knee = knee_of(v)
    pairs = []
    for l in (knee - 1, knee, knee + 1, knee + 2):
        flank = max(20, gap_cost(l, v) // v["match"] + 12)
        a, b = synth.rand_seq(rng, flank + int(rng.integers(0, 6))), synth.rand_seq(rng, flank + int(rng.integers(0, 6)))
        gap = synth.rand_seq(rng, l)
        assert v["match"] * min(len(a), len(b)) > gap_cost(l, v)
        pairs.append(dict(name=f"knee:{l}I", q=a + gap + b, t=a + b, planted=f"{l}I"))
        pairs.append(dict(name=f"knee:{l}D", q=a + b, t=a + gap + b, planted=f"{l}D"))
    return _records(pairs, over)


def r_list():
    """The rows-per-lane classes k_trace_fill is built for: NRA_R_LIST of nra_internal.h."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nanorepeat_amd", "csrc", "nra_internal.h")
    text = open(path).read().replace("\\\n", " ")
    m = re.search(r"#define\s+NRA_R_LIST\(X\)((?:\s*X\(\d+\))+)", text)
    assert m, "NRA_R_LIST not found"
    rs = [int(x) for x in re.findall(r"X\((\d+)\)", m.group(1))]
    assert len(rs) == 24 and rs == sorted(set(rs)) and rs[-1] == 48, rs
    return rs


def _planted_target(rng, piece, k, keep_head):
    """`piece` with hifi errors (12 bases at its head or at its tail exact) and one 25-base gap: 25 bases cut out (25I
    in the path) for even k, 25 random bases put in (25D) for odd k.  Pieces under 90 bases stay as they are."""
    if len(piece) < 90:
        return piece
    body = synth.apply_errors(rng, piece[12:] if keep_head else piece[:-12], "hifi")
    mid = len(body) // 2
    body = body[:mid] + body[mid + 25:] if k % 2 == 0 else body[:mid] + synth.rand_seq(rng, 25) + body[mid:]
    return piece[:12] + body if keep_head else body + piece[-12:]


def class_border_pairs():
    """(pairs, the same with one N in every query).  Two queries for every class R of NRA_R_LIST: 64 R bases (every lane
    full) against about 150 - 170 bases cut from the query's end, so that the best cell sits in the last occupied lane,
    and 64 R_prev + 1 bases (the first length of the class: one row in its last occupied lane) against a cut from the
    query's start.  `R` is kept in each pair."""
    rng = np.random.default_rng(20260503)
    plain, prev = [], 0
    for k, R in enumerate(r_list()):
        q = synth.rand_seq(rng, 64 * R)
        cut = min(len(q), int(rng.integers(150, 171)))
        plain.append(dict(name=f"class:R={R}:full", q=q, t=_planted_target(rng, q[-cut:], k, False), R=R, last_lane=True))
        q = synth.rand_seq(rng, 64 * prev + 1)
        cut = min(len(q), int(rng.integers(150, 171)))
        plain.append(dict(name=f"class:R={R}:first", q=q, t=_planted_target(rng, q[:cut], k + 1, True), R=R, last_lane=False))
        prev = R
    with_n = []
    for p in plain:
        # (inside the part of the query that the target was cut from, clear of its exact end)
        lo, hi = (len(p["q"]) - 100, len(p["q"]) - 20) if p["last_lane"] else (20, 100)
        at = int(rng.integers(lo, hi)) if len(p["q"]) > 120 else len(p["q"]) // 2
        with_n.append(dict(p, name=p["name"] + ":N", q=_with_n(p["q"], at)))
    O = _oracle()
    for p in plain + with_n:
        R, n = p["R"], len(p["q"])
        assert min(r for r in r_list() if 64 * r >= n) == R, p["name"]
        if p["last_lane"] and "N" not in p["q"]:
            r = O.align_cigar(p["q"], p["t"], O.default_scoring(min_dp_score=0))
            assert (r["qend"] - 1) // R == 63, (p["name"], r["qend"])
    return _records(plain, {}), _records([p for p in with_n if len(p["q"]) > 1], {})


def target_edge_pairs():
    """A 100-base query against targets of 1 .. 193 columns, where the number of 64-column chunks of the fill,
    (ncols + 126) >> 6, turns over: once with the match ending in the target's last column (`edge` = "end"), once with
    the match beginning in its first (`edge` = "start")."""
    rng = np.random.default_rng(20260504)
    q = synth.rand_seq(rng, 100)
    pairs = []
    for tl in (1, 63, 64, 65, 127, 128, 129, 191, 192, 193):
        n = min(tl, 70)
        piece = q[15:15 + n]
        if n > 30:
            piece = piece[:8] + synth.apply_errors(rng, piece[8:-8], "ont") + piece[-8:]
        pad = max(0, tl - len(piece))
        for edge, t in (("end", synth.rand_seq(rng, pad) + piece), ("start", piece + synth.rand_seq(rng, pad))):
            t = t[-tl:] if edge == "end" else t[:tl]
            assert len(t) == tl
            pairs.append(dict(name=f"edge:{tl}:{edge}", q=q, t=t, edge=edge))
    O = _oracle()
    for p in pairs:
        r = O.align_cigar(p["q"], p["t"], O.default_scoring(min_dp_score=0))
        assert (r["tend"] == len(p["t"])) if p["edge"] == "end" else (r["tstart"] == 0), (p["name"], r)
    return _records(pairs, {})


def long_target_pairs():
    """Origin columns beyond 15 bits in the int32 cell (its low 16 bits, part of every max): a 65 000-column target (the
    longest there is, its last pipeline chunk partial) with a 150-base query at columns 64 840 .. 64 990 and one at
    column 0, and a 40 000-column target with a query at column 33 000.  25.5 M cells in all."""
    rng = np.random.default_rng(20260505)
    t65, t40 = synth.rand_seq(rng, 65000), synth.rand_seq(rng, 40000)

    def image(t, a):
        s = t[a:a + 150]
        return s[:10] + synth.apply_errors(rng, s[10:-10], "hifi") + s[-10:]

    pairs = [dict(name="long:65000:end", q=image(t65, 64840), t=t65, tstart=64840, tend=64990),
             dict(name="long:65000:start", q=image(t65, 0), t=t65, tstart=0, tend=150),
             dict(name="long:40000:33000", q=image(t40, 33000), t=t40, tstart=33000, tend=33150)]
    assert sum(len(p["q"]) * len(p["t"]) for p in pairs) < 30e6
    return _records(pairs, {})


def best_cell_tie_pairs(block_rows):
    """Equal maxima for the best-cell rule (the maximum packed value, then the smallest column, then the smallest row),
    S a 40-base segment: X + S + Y + S + Z against S (two maxima in one column, their rows in different row blocks of
    `block_rows` rows and in different lanes: |X + S| < block_rows <= |X + S + Y|), S against S + W + S (two columns; the
    origin column is part of the value), and both at once."""
    assert block_rows >= 64
    rng = np.random.default_rng([20260506, block_rows])
    S = synth.rand_seq(rng, 40)
    # (X, Y and Z without A and W all A: no base around a copy of S in the query equals one around a copy in the target, so
    # no maximum grows past its copy, and joining two copies through Y and W loses: every maximum is one exact copy, 80)
    X, Y, Z = ("".join(rng.choice(list("CGT"), n)) for n in (block_rows - 48, 48, 7))
    W = "A" * 55
    assert len(X + S) < block_rows <= len(X + S + Y)
    two_rows = X + S + Y + S + Z
    pairs = [dict(name=f"tie:{block_rows}:rows", q=two_rows, t=S, score=80),
             dict(name=f"tie:{block_rows}:columns", q=S, t=S + W + S, score=80),
             dict(name=f"tie:{block_rows}:both", q=two_rows, t=S + W + S, score=80)]
    O = _oracle()
    for p in pairs:
        assert O.align(p["q"], p["t"], O.default_scoring(min_dp_score=0))[0] == 80, p["name"]
    return pairs


def score_border_pairs():
    """match = 64: identical pairs of 500 bases (score 32 000, the last an int32 cell takes in either entry point) and of
    501 (32 064: 64-bit cells in nra_align_paths, NRA_E_RANGE in nra_align_pairs_cigar), and the 501-base query with one N
    (31 999 under sc_ambi = 1: through the N costs 1, either side alone at most 250 x 64)."""
    rng = np.random.default_rng(20260507)
    s500, s501 = synth.rand_seq(rng, 500), synth.rand_seq(rng, 501)
    pairs = [dict(name="border:500", q=s500, t=s500, score=32000), dict(name="border:501", q=s501, t=s501, score=32064),
             dict(name="border:501:N", q=_with_n(s501, 250), t=s501, score=31999)]
    return _records(pairs, dict(match=64))


TRACE_BLOCK_ROWS = (64, 128, 192, 256, 384, 512, 768, 1024, 1536)   # 64 x NRA_TRACE_MT_R_LIST


def is_wide(pair, match):
    """Whether nra_align_paths gives the pair 64-bit cells: match * min(qlen, tlen) beyond 32 000."""
    return match * min(len(pair["q"]), len(pair["t"])) > 32000


def row_block_pairs(rows, wide, nb=2):
    """Pairs for row blocks of `rows` rows (NRA_TEST_TRACE_BLOCK_ROWS): a query of nb * rows + 5 bases -- nb full blocks
    and a last one of 5 rows -- against two targets of 220 columns (`wide`: 520, for match = 64), and a copy of the query
    with N runs across the first and the last seam.  Target A's image in the query carries a 30-base insertion across the
    first seam (rows rows - 15 .. rows + 14).  Target B's image ends with the query, so its path crosses the last seam into
    the 5-row block: on the diagonal for the 220-column targets (5 rows beneath that seam, at 2 per match, cannot pay for
    a 30-base insertion), and for `wide` with a 30-base insertion over rows last seam - 27 .. + 2, which the two
    64-point matches beneath it pay for.  (Under match = 64 and mismatch = 4 random bases align at a profit, so those
    paths run nearly the length of the query, ties and all, whatever is planted; that they cross the first seam is what
    is asserted of them.)  nb = 2 are the queries of 2 * rows + 5 bases;
    64-bit cells are chosen by match * min(qlen, tlen) > 32 000, which 2 * rows + 5 <= 389 bases do not reach, so the
    caller asks for the nb that makes the query exceed 500 bases as well."""
    rng = np.random.default_rng([20260508, rows, int(wide), nb])
    tl = 520 if wide else 220
    ql, last = nb * rows + 5, nb * rows
    ta, tb = synth.rand_seq(rng, tl), synth.rand_seq(rng, tl)
    q = list(synth.rand_seq(rng, ql))
    h = min(rows - 15, 100)                                            # A: h bases, 30 inserted across the seam, h2 bases
    h2 = min(rows - 10, 100) if nb > 2 or rows >= 256 else 39
    q[rows - 15 - h:rows - 15] = ta[60:60 + h]
    q[rows + 15:rows + 15 + h2] = ta[60 + h:60 + h + h2]
    room = ql - (rows + 15 + h2)                                       # rows left under A's image
    if wide:                                                           # B: hb bases, 30 inserted across the last seam, 2 bases
        hb = max(8, min(room - 35, 100))                               # (over A's image where the query has no room)
        q[last - 27 - hb:last - 27] = tb[40:40 + hb]
        q[last + 3:last + 5] = tb[40 + hb:40 + hb + 2]
    else:                                                              # B: the last hb rows, with ont errors but for the ends
        hb = min(room, 100)
        img = tb[40:40 + hb]
        if hb > 40:
            img = (img[:8] + synth.apply_errors(rng, img[8:-8], "ont") + img[-8:])[-hb:]
        q[ql - len(img):] = img
    q = "".join(q)
    assert len(q) == ql and 2 * h > 54 and 2 * h2 > 54 and hb >= 8, (rows, wide, h, h2, hb)
    qn = _with_n(_with_n(_with_n(q, rows - 3, 6), last - 2, 3), rows - 20, 2)
    pairs = []
    kind = f"rows={rows}:nb={nb}:{'match64' if wide else 'default'}"
    for tag, query in (("", q), (":N", qn)):
        pairs.append(dict(name=f"{kind}:A{tag}", q=query, t=ta, seam=rows, planted=None if wide else "30I"))
        # (`seam`: one the path is known to cross.  Under match = 64 it may end a few rows above the last one.)
        pairs.append(dict(name=f"{kind}:B{tag}", q=query, t=tb, seam=rows if wide else last, planted=None))
    return _records(pairs, dict(match=64) if wide else {})
