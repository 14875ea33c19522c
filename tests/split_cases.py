"""Groups of tracts with their backbones for the allele-split tests (CPU and GPU share them)."""
import numpy as np

from nanorepeat_amd import synth
from consensus_cases import _rand


def _sub(s, at, shift=1):
    return s[:at] + "ACGT"[("ACGT".index(s[at]) + shift) % 4] + s[at + 1:]


def matrix_group(rng, t=40, n_sites=3, reads=9, noise=0.15):
    """Reads without indels: the backbone with, at n_sites fixed columns, a base drawn per read from two or three
    candidates, an N or nothing changed; small enough that odd things happen (ties, undecided reads, a haplotype silent
    at a site)."""
    b = _rand(rng, t)
    cols = sorted(rng.choice(np.arange(2, t - 2), n_sites, replace=False).tolist())
    hap = rng.integers(0, 2, reads)
    out = []
    for r in range(reads):
        s = b
        for q, c in enumerate(cols):
            u = rng.random()
            if u < noise:
                s = s[:c] + "N" + s[c + 1:]
            elif u < 2 * noise:
                s = _sub(s, c, int(rng.integers(1, 4)))
            elif hap[r] and (q == 0 or rng.random() < 0.7):
                s = _sub(s, c, 1)
        out.append(s)
    return out, b


def corner_cases(seed=41):
    """[(groups, backbones, thresholds)]: the corners of the contract.  Small enough for the full matrix."""
    rng = np.random.default_rng(seed)
    calls = []
    b = "CAG" * 20 + "CAA" + "CAG"
    alt = "CAG" * 22
    core = _rand(rng, 120)
    two = [core] * 5 + [_sub(_sub(core, 30), 77)] * 4
    # no tracts; an empty backbone; empty tracts; all left out; no site; one site; a lone read
    calls.append(([[], [b, alt], ["", ""], ["", b, ""], [core, _sub(core, 5), _sub(core, 9)], [b] * 6, [b] * 5 + [alt] * 4,
                   [b]],
                  [b, "", b[:7], b, _rand(rng, 120), b, b, b], dict(min_sites=1)))
    calls.append(([[core, _sub(core, 5), _sub(core, 9)], two, two, [_sub(core, 5), _sub(core, 9)]], [core] * 4,
                  dict(max_dist=0, min_sites=1)))
    # a haplotype none of whose reads shows a base at a site: it takes the site's b there
    silent = [core] * 4 + [_sub(core, 77)] * 3 + [_sub(core, 30)[:77] + "N" + core[78:]] * 4
    calls.append(([silent, silent[::-1]], [core, core], dict(min_sites=1)))
    # thresholds around a two-site pair: min_sites 1, 2 and 3, purity, share, count
    for kw in (dict(min_sites=1), dict(min_sites=2), dict(min_sites=3), dict(min_count=5), dict(min_count=4),
               dict(min_share_pct=45), dict(min_share_pct=44), dict(min_purity_pct=100), dict(max_iter=1)):
        calls.append(([two, two[::-1], two + [_sub(core, 30)] * 2 + [core[:30] + "N" + core[31:76] + core[78:]]],
                      [core] * 3, kw))
    # more sites than max_sites: 12 columns differ, 5 / 1 stay; the uneven counts decide which
    many = core
    for q in range(12):
        many = _sub(many, 8 + 9 * q)
    part = many[:60] + core[60:]
    g = [core] * 7 + [many] * 5 + [part] * 2
    for k in (5, 1, 12, 11):
        calls.append(([g, g[::-1]], [core, many], dict(max_sites=k)))
    # a tie that stays undecided: reads that show no base at any site, or one site each way
    n_at = core[:30] + "N" + core[31:77] + "N" + core[78:]
    each = _sub(core, 30)
    calls.append(([two + [n_at, each, core[:30] + core[31:77] + core[78:]]], [core], dict(min_sites=1)))
    # code-4 bases, lower case, a backbone in lower case
    calls.append(([[x.lower() for x in two] + [n_at]], [core.lower()], dict(min_sites=1, min_count=2)))
    # small matrices: ties, undecided reads, haplotypes silent at a site
    groups, bbs = [], []
    for _ in range(60):
        g, bb = matrix_group(rng, n_sites=int(rng.integers(1, 6)), reads=int(rng.integers(4, 14)))
        groups.append(g)
        bbs.append(bb)
    calls.append((groups, bbs, dict(min_count=1, min_sites=1)))
    calls.append((groups, bbs, dict(min_count=2, min_sites=1, min_share_pct=10, max_iter=2)))
    # noisy alleles with a second haplotype and indels, through the real alignment
    g, bbs = [], []
    for unit, k, m, model in (("CAG", 25, 7, "ont"), ("TATTG", 20, 6, "ont"), ("GAA", 60, 5, "hifi"), ("AAGGG", 30, 8, "ont")):
        truth = unit * k
        other = _sub(_sub(truth, len(truth) // 3), 2 * len(truth) // 3)
        g.append([synth.apply_errors(rng, truth if q % 2 else other, model) for q in range(2 * m)])
        bbs.append(truth)
    calls.append((g, bbs, dict(min_sites=1)))
    calls.append((g, bbs, dict(max_dist=12)))
    return calls


def seeded_groups(count=200, seed=42, min_len=20, max_len=3000):
    """`count` groups like consensus_cases.seeded_alleles, with the true tract as backbone; every third group holds a
    second haplotype: 1 to 4 substituted bases in about half of its reads.  -> (groups, backbones)."""
    rng = np.random.default_rng(seed)
    groups, bbs = [], []
    for q in range(count):
        p = int(rng.integers(1, 7))
        unit = _rand(rng, p)
        length = int(min_len * (max_len / min_len) ** rng.random())          # log-uniform
        if q % 10 == 0:
            length = int(rng.integers(max_len * 2 // 3, max_len + 1))
        m = int(rng.integers(2, 61)) if length < 1000 else int(rng.integers(2, 13))
        model = "ont" if q % 2 == 0 else "hifi"
        truth = (unit * (length // p + 1))[:length]
        other = truth
        if q % 3 == 0:
            for at in rng.integers(0, length, int(rng.integers(1, 5))):
                other = _sub(other, int(at), int(rng.integers(1, 4)))
        reads = [synth.apply_errors(rng, other if rng.random() < 0.5 else truth, model) for _ in range(m)]
        if q % 9 == 4:                                                     # one read of another size
            reads.append(synth.apply_errors(rng, truth[:len(truth) * 3 // 5], model))
        if q % 13 == 5:
            reads[0] = reads[0][:len(reads[0]) // 2] + "N" + reads[0][len(reads[0]) // 2:]
        if q % 11 == 6:                                                    # a read of something else, as long as the rest
            reads.append(_rand(rng, len(reads[0])))
        if q % 17 == 7:
            reads.append("")
        groups.append(reads)
        bbs.append(truth)
    return groups, bbs


def long_group(seed=43, length=20000, reads=6):
    rng = np.random.default_rng(seed)
    truth = ("GGCCTG" * (length // 6 + 1))[:length]
    other = truth
    for at in (3000, 11111, 17002):
        other = _sub(other, at)
    return [synth.apply_errors(rng, other if q % 2 else truth, "hifi") for q in range(reads)], truth
