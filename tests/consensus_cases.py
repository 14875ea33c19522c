"""Seeded groups of tracts for the consensus tests (CPU and GPU share them)."""
import numpy as np

from nanorepeat_amd import synth


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _mutate(rng, s, n_edits):
    """n_edits substitutions, insertions and deletions at random places."""
    s = list(s)
    for _ in range(n_edits):
        kind = int(rng.integers(0, 3))
        at = int(rng.integers(0, max(1, len(s))))
        if kind == 0 and s:
            s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4] if s[at] in "ACGT" else "A"
        elif kind == 1:
            s.insert(at, "ACGT"[int(rng.integers(0, 4))])
        elif s:
            del s[at]
    return "".join(s)


def edge_groups(seed=11):
    """[(groups, max_dist)]: the corners of the contract.  Small enough for the full matrix."""
    rng = np.random.default_rng(seed)
    calls = []
    # delta = t - n from -40 to +40: a backbone-length tract (the median) and tracts shorter / longer by up to 40
    base = "CAG" * 30
    g = [base] * 3
    for d in (-40, -23, -7, -1, 1, 9, 25, 40):
        g.append(base[:len(base) + d] if d < 0 else base + _rand(rng, d))
        g.append(base)                           # keeps the median at the base length
    calls.append(([g], 1000))
    # distances just below, at and just above max_dist: substitutions only, spread out (distance = their number)
    core = _rand(rng, 400)

    def subs(k):
        s = list(core)
        for q in range(k):
            at = 7 + q * 9
            s[at] = "ACGT"[("ACGT".index(s[at]) + 1) % 4]
        return "".join(s)
    # (the tract in the middle of the group is the round-0 backbone: all have one length)
    calls.append(([[subs(11), subs(12), subs(13), core, core, core, subs(30)]], 12))
    calls.append(([[core, subs(1), subs(2)]], 0))
    # code-4 bases in tracts and in the round-0 backbone (the median tract carries N and lower case)
    u = "TATTG" * 12
    calls.append(([[u[:20] + "N" + u[20:], u[:31] + "NN" + u[33:], u.lower(), u[:9] + "n" + u[10:], "N" * 5 + u,
                    u[:40] + "R" + u[40:]],
                   [u[:30] + "N" + u[30:]],                         # one read: its ACGT bases after one round
                   ["NNNN"],                                      # a backbone of no bases
                   ["ACGT" * 5 + "N", "acgtn" * 4]], 1000))
    # one read, two reads (every vote ties), all reads left out, empty groups, empty tracts
    a, b = _rand(rng, 90), _rand(rng, 95)
    calls.append(([[a], [a, b], [a, _mutate(rng, a, 6)], [], ["", ""], ["", a, ""]], 1000))
    calls.append(([[_rand(rng, 60), _rand(rng, 60), _rand(rng, 60)], [_rand(rng, 50), _rand(rng, 120)]], 5))
    # every read left out: with max_dist 0 a tract that carries an N is at distance >= 1 of a backbone without it
    calls.append(([["AAAAAAAAN", "CCCCCCCCN", "GGGGGGGGN"], [core[:50] + "N", core[:50] + "N"], [a, a, b]], 0))
    # noisy alleles of a few shapes
    g = []
    for unit, k, m, model in (("CAG", 25, 7, "ont"), ("A", 30, 9, "ont"), ("TATTG", 20, 2, "ont"), ("GAA", 60, 5, "hifi"),
                              ("AAGGG", 30, 4, "ont")):
        g.append([synth.apply_errors(rng, unit * k, model) for _ in range(m)])
    calls.append((g, 1000))
    calls.append((g, 20))
    return calls


def seeded_alleles(count=200, seed=12, min_len=20, max_len=3000):
    """`count` groups: ONT and HiFi, motif lengths 1-6, 2-60 reads, tracts of min_len..max_len bases."""
    rng = np.random.default_rng(seed)
    groups = []
    for q in range(count):
        p = int(rng.integers(1, 7))
        unit = _rand(rng, p)
        length = int(min_len * (max_len / min_len) ** rng.random())          # log-uniform
        if q % 10 == 0:
            length = int(rng.integers(max_len * 2 // 3, max_len + 1))
        m = int(rng.integers(2, 61)) if length < 1000 else int(rng.integers(2, 13))
        model = "ont" if q % 2 == 0 else "hifi"
        truth = (unit * (length // p + 1))[:length]
        if q % 7 == 3:                                                     # an interruption
            at = len(truth) // 2
            truth = truth[:at] + _rand(rng, 3) + truth[at:]
        reads = [synth.apply_errors(rng, truth, model) for _ in range(m)]
        if q % 9 == 4:                                                     # one read of another size
            reads.append(synth.apply_errors(rng, truth[:len(truth) * 3 // 5], model))
        if q % 13 == 5:
            reads[0] = reads[0][:len(reads[0]) // 2] + "N" + reads[0][len(reads[0]) // 2:]
        if q % 11 == 6:                                                    # a read of something else, as long as the rest:
            reads.append(_rand(rng, len(reads[0])))                          # far beyond the first band tried for it
        groups.append(reads)
    return groups


def long_allele(seed=13, length=20000, reads=4):
    rng = np.random.default_rng(seed)
    truth = ("GGCCTG" * (length // 6 + 1))[:length]
    return [synth.apply_errors(rng, truth, "hifi") for _ in range(reads)]
