"""Groups of flank rows with their backbone sides for the flank-haplotype tests (CPU and GPU share them).  A group is a
list of rows (left segment, right segment), a backbone a pair (left side, right side); everything from the repeat
outward."""
import numpy as np

from nanorepeat_amd import synth
from consensus_cases import _rand
from split_cases import _sub


def _with_n(s, k, step=4, first=2):
    """s with k of its bases replaced by N, `step` apart: every N costs exactly one edit against any backbone."""
    out = list(s)
    for q in range(k):
        out[first + q * step] = "N"
    return "".join(out)


def matrix_group(rng, t_left=30, t_right=26, n_sites=3, rows=9, noise=0.15):
    """Rows without indels over two short sides, ragged: at n_sites columns a base drawn per row from two or three
    candidates, an N or nothing changed; every row covers a random prefix of either side or lacks it."""
    b = (_rand(rng, t_left), _rand(rng, t_right))
    cols = [sorted(rng.choice(np.arange(1, t - 1), min(n_sites, t - 2), replace=False).tolist()) for t in (t_left, t_right)]
    hap = rng.integers(0, 2, rows)
    out = []
    for r in range(rows):
        row = []
        for side in (0, 1):
            s = b[side]
            for q, c in enumerate(cols[side]):
                u = rng.random()
                if u < noise:
                    s = s[:c] + "N" + s[c + 1:]
                elif u < 2 * noise:
                    s = _sub(s, c, int(rng.integers(1, 4)))
                elif hap[r] and (q == 0 or rng.random() < 0.7):
                    s = _sub(s, c, 1)
            u = rng.random()
            row.append("" if u < 0.2 else s if u < 0.6 else s[:int(rng.integers(1, len(s) + 1))])
        out.append(tuple(row))
    return out, b


def corner_cases(seed=51):
    """[(groups, backbones, thresholds)]: the corners of the contract.  Small enough for the full matrix."""
    rng = np.random.default_rng(seed)
    calls = []
    loose = dict(skip=0, min_count=1, min_sites=1)
    core, other = _rand(rng, 120), _rand(rng, 90)
    # n = 1; t = 0 on one side or on both; no rows; absent sides; a None segment
    calls.append(([[("A", ""), ("C", "G"), ("", "T"), ("", "")], [("A", "C"), ("", "G")], [("T", "")], [],
                   [(None, core[:1]), (core[:1], None)], [("", ""), (None, None)]],
                  [("", "ACGT"), ("", ""), ("A", ""), (core, other), (core, core), (core, other)], loose))
    # a row whose only side is left out (label -1), one with one side left out and the other aligned
    far = "".join("ACGT"[("ACGT".index(c) + 2) % 4] for c in core)
    calls.append(([[(core, other)] * 3 + [(far[:40], "")] + [(far[:40], other)] + [(_sub(core, 30), _sub(other, 40))] * 3],
                  [(core, other)], dict(loose, max_dist=5)))
    # a segment shorter than its side with j* = 15, 16, 17, 31, 32, 33 (mod 16: 15, 0, 1), and sides of 15, 16, 17 columns
    ends = [(core[:n], other[:n]) for n in (15, 16, 17, 31, 32, 33, 47, 48, 49)]
    calls.append(([ends + [(_sub(core[:n], 7), _sub(other[:n], 9)) for n in (15, 16, 17, 31, 32, 33)]], [(core[:50], other[:50])],
                  loose))
    for t in (15, 16, 17):
        calls.append(([[(core[:t], other[:t])] * 3 + [(_sub(core[:t], 5), _sub(other[:t], 6))] * 2 + [(core[:t - 3], other[:9])]],
                      [(core[:t], other[:t])], loose))
    # a tie for j*: the last base is an N, inserted after column 10 or aligned to column 11
    calls.append(([[(core[:10] + "N", other[:20] + "N")] * 2 + [(core[:30], other[:30])] * 2], [(core[:40], other[:40])], loose))
    # n = t with net deletions, the path ends at column t; n > t
    gone = core[:5] + core[6:9] + core[10:40] + "GG"
    calls.append(([[(gone, other[:40])] * 2 + [(core[:40] + "ACGTA", other[:40] + "T")] + [(core[:40], other[:40])] * 3],
                  [(core[:40], other[:40])], loose))
    # e exactly h and h + 1 in class 1 (h = 31), and at the 63 / 64 border; e exactly max_dist and max_dist + 1
    long_b = _rand(rng, 400)
    for kw in (dict(loose), dict(loose, max_dist=63), dict(loose, max_dist=10), dict(loose, max_dist=0)):
        ks = (31, 32, 63, 64, 10, 11, 0, 1)
        calls.append(([[(_with_n(long_b[:300], k), _with_n(long_b[:290], k, first=1)) for k in ks]], [(long_b, long_b)], kw))
    # a site at offset skip - 1 and one at skip, on either side
    reads = [(core[:60], other[:60])] * 4 + [(_sub(_sub(core[:60], 6), 7), _sub(_sub(other[:60], 6), 7))] * 3
    for skip in (7, 8, 6):
        calls.append(([reads, reads[::-1]], [(core[:60], other[:60])] * 2, dict(skip=skip, min_count=2, min_sites=1)))
    # 2 (n[a] + n[b]) equal to cov and to cov - 1: two rows show a, one b, three or four an N or a deletion
    base = core[:40]
    rows = [(base, "")] * 2 + [(_sub(base, 20), "")] + [(base[:20] + "N" + base[21:], "")] * 2 + [(base[:20] + base[21:], "")]
    calls.append(([rows, rows + [(base[:20] + "N" + base[21:], "")], rows + [(base[:15], "")]], [(base, other[:10])] * 3, loose))
    # a haplotype made only of left-anchored and right-anchored rows that share no column: linked through the b default
    alt_l, alt_r = _sub(_sub(core[:80], 25), 50), _sub(_sub(other[:80], 30), 60)
    lone = [(core[:80], other[:80])] * 6 + [(alt_l, "")] * 4 + [("", alt_r)] * 4
    calls.append(([lone, lone[::-1], lone[6:] + lone[:6]], [(core[:80], other[:80])] * 3, dict(skip=5, min_count=3, min_sites=2)))
    # a group with no site; more sites than max_sites
    many = core[:100]
    for q in range(9):
        many = _sub(many, 8 + 10 * q)
    part = many[:50] + core[50:100]
    g = [(core[:100], other)] * 7 + [(many, other)] * 5 + [(part, other)] * 2
    calls.append(([[(core, other)] * 5, g], [(core, other), (core[:100], other)], loose))
    for k in (4, 1, 9):
        calls.append(([g, g[::-1]], [(core[:100], other)] * 2, dict(skip=0, min_count=2, min_sites=1, max_sites=k)))
    # lower case, code-4 bases
    calls.append(([[(x.lower(), y) for x, y in lone] + [("n" * 12, "N" * 7)]], [(core[:80].lower(), other[:80])], dict(skip=5)))
    # small ragged matrices: ties, undecided rows, haplotypes silent at a site
    groups, bbs = [], []
    for _ in range(60):
        g, bb = matrix_group(rng, n_sites=int(rng.integers(1, 5)), rows=int(rng.integers(4, 14)))
        groups.append(g)
        bbs.append(bb)
    calls.append((groups, bbs, dict(skip=0, min_count=1, min_sites=1)))
    calls.append((groups, bbs, dict(skip=3, min_count=2, min_sites=1, min_share_pct=10, max_iter=2)))
    # noisy rows with a second haplotype and indels, through the real alignment
    groups, bbs = [], []
    for model, m in (("ont", 7), ("hifi", 6), ("ont", 5)):
        bl, br = _rand(rng, 220), _rand(rng, 180)
        al, ar = _sub(_sub(bl, 60), 140), _sub(_sub(br, 45), 120)
        g = []
        for q in range(2 * m):
            sl, sr = (al, ar) if q % 2 else (bl, br)
            g.append((synth.apply_errors(rng, sl[:int(rng.integers(80, 206))], model),
                      synth.apply_errors(rng, sr[:int(rng.integers(60, 170))], model) if q % 5 else ""))
        groups.append(g)
        bbs.append((bl, br))
    calls.append((groups, bbs, dict(skip=10, min_sites=1)))
    calls.append((groups, bbs, dict(skip=10, max_dist=12)))
    return calls


def seeded_groups(count=150, seed=52, max_len=1500):
    """`count` groups with ragged coverage: two sides of 60 to max_len bases, 3 to 12 rows (8 to 16 with a second haplotype) whose segments cover a random
    part of their side (some rows lack a side), ont or hifi errors; every third group holds a second haplotype (1 to 4
    substitutions per side in about half of its rows); now and then a segment with many more errors (the wide band
    classes), a segment of something else (left out) or a side beyond its segment's reach.  -> (groups, backbones)."""
    rng = np.random.default_rng(seed)
    groups, bbs = [], []
    for q in range(count):
        t = [int(60 * (max_len / 60) ** rng.random()) for _ in (0, 1)]
        if q % 10 == 0:
            t[0] = int(rng.integers(max_len * 2 // 3, max_len + 1))
        if q % 14 == 3:
            t[1] = 0
        b = [_rand(rng, x) for x in t]
        alt = list(b)
        if q % 3 == 0:                                                     # most of them in the near half, beyond skip
            for side in (0, 1):
                for at in rng.integers(0, max(1, t[side]), int(rng.integers(1, 5)) if t[side] else 0):
                    at = int(at) if rng.random() < 0.3 else 20 + int(at) // 2 if 20 + int(at) // 2 < t[side] else int(at)
                    alt[side] = _sub(alt[side], at, int(rng.integers(1, 4)))
        model = "ont" if q % 2 == 0 else "hifi"
        rows = []
        for r in range(int(rng.integers(8, 17)) if q % 3 == 0 else int(rng.integers(3, 13))):
            src = alt if rng.random() < 0.5 else b
            row = []
            for side in (0, 1):
                u = rng.random()
                if u < 0.15 or t[side] == 0:
                    row.append("")
                    continue
                reach = t[side] if u < 0.5 else int(rng.integers(1, t[side] + 1))
                row.append(synth.apply_errors(rng, src[side][:reach], model))
            rows.append(tuple(row))
        if q % 7 == 2 and t[0] >= 400:                                     # noisy segments: the classes 256 to 1024
            for passes in (2, 3, 5):
                s = b[0]
                for _ in range(passes):
                    s = synth.apply_errors(rng, s, "ont")
                rows.append((s, ""))
        if q % 11 == 6:                                                    # a segment of something else: left out
            rows.append((_rand(rng, int(rng.integers(30, 900))), ""))
        if q % 13 == 5 and rows:
            s = rows[0][0]
            rows[0] = (s[:len(s) // 2] + "N" + s[len(s) // 2:], rows[0][1])
        if q % 17 == 7:
            rows.append(("", ""))
        groups.append(rows)
        bbs.append(tuple(b))
    return groups, bbs


def long_group(seed=53, length=20000, reach=18750, rows=6):
    """One side of `length` columns with segments of `reach` bases, three planted substitutions in every other row."""
    rng = np.random.default_rng(seed)
    truth = _rand(rng, length)
    other = truth
    for at in (3000, 11111, 17002):
        other = _sub(other, at)
    return [(synth.apply_errors(rng, (other if q % 2 else truth)[:reach], "hifi"), "") for q in range(rows)], (truth, "")
