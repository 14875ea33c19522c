"""Inputs of the motif screen's tests (tests/test_screen_partial_cpu.py, tests/test_screen_partial_gpu.py): each case
is dict(anchors, motifs, reads, k, max_occ, min_hits, pct).  Small enough for the plain-Python restatement."""
import itertools

import numpy as np

from nanorepeat_amd import synth
from screen_partial_ref import motif_root, class_members

TILE = 4096          # NRA_SCREEN_TILE
LDS_MAP = 128        # NRA_SCREEN_MAP


def _rand_anchors(rng, n, length=120):
    return [(synth.rand_seq(rng, length), synth.rand_seq(rng, length)) for _ in range(n)]


def edge_case(k):
    """Hand-built reads: every period 1..6 on both strands and in lower case, an N inside a run, reads shorter than k
    and of exactly k, two classes in one read, p = 6 at k = 11 (k < 2p), and a period-2 stretch inside a p = 4 motif's
    neighbourhood (ACACACAT: ACAC... windows have smallest period 2)."""
    rng = np.random.default_rng(100 + k)
    motifs = ["A", "AC", "CAG", "AAAG", "AATGG", "AACCCT", "CAGCAG", "CTG", "ACACACAT", "ACAT", "AAAAAAC", "GGCCTCA" * 2]
    anchors = _rand_anchors(rng, len(motifs))
    reads = []
    for m in motifs[:6]:
        run = m * (60 // len(m))
        reads += [run, synth.revcomp(run), run.lower(), synth.rand_seq(rng, 37) + run + synth.rand_seq(rng, 23)]
    cag = "CAG" * 20
    reads += [cag[:30] + "N" + cag[:30],            # an N inside a run
              cag[:k - 1], cag[:k], cag[:k + 1], "", "N" * 40,
              "CAG" * 15 + synth.rand_seq(rng, 9) + "AAAG" * 12,      # two classes in one read
              "AACCCT" * 2, ("AACCCT" * 3)[:k + 5],                   # p = 6: k - p bases have to agree
              "ACACACAT" * 6, "ACAT" * 4 + "ACACACACACACACACACAC" + "ACAT" * 5,
              "AC" * 10 + "ACAT" * 8, "GGCCTCA" * 8, "AAAAAAC" * 8,
              synth.rand_seq(rng, 300),
              anchors[2][0] + "CAG" * 30, "CTG" * 30 + synth.revcomp(anchors[2][0]),   # one anchor plus the repeat
              anchors[3][0] + "AAAG" * 5 + anchors[3][1]]
    return dict(anchors=anchors, motifs=motifs, reads=reads, k=k, max_occ=16, min_hits=2, pct=5)


def tile_case():
    """Reads of 4096 and of 4097 windows with a repeat run straddling window position 4096, and one read of about
    20 000 bases over five tiles."""
    rng = np.random.default_rng(7)
    k = 15
    motifs = ["CAG", "AAAG", "TTAGGG"]
    anchors = _rand_anchors(rng, 3)
    reads = []
    for n_win in (TILE, TILE + 1):                 # the run's windows are 4050..4095, then 4050..4096
        n = n_win + k - 1
        reads.append(synth.rand_seq(rng, 4050) + ("CAG" * 30)[:n - 4050])
    body = list(synth.rand_seq(rng, 20000))
    for at, run in ((4000, "AAAG" * 80), (8150, "TTAGGG" * 40), (12250, "CAG" * 40), (16350, "CTG" * 50)):
        body[at:at + len(run)] = run
    reads.append("".join(body))
    reads.append("AAAG" * 2500)
    return dict(anchors=anchors, motifs=motifs, reads=reads, k=k, max_occ=16, min_hits=4, pct=1)


def distinct_roots(n, p=6):
    """n primitive p-base words of n different classes, in lexicographic order."""
    out, seen = [], set()
    for t in itertools.product("ACGT", repeat=p):
        w = "".join(t)
        if len(motif_root(w)) == p and w not in seen:
            seen |= class_members(w)
            out.append(w)
            if len(out) == n:
                return out
    raise ValueError("not that many classes")


FULL_MAP_PERMUTATION = (5, 2, 6, 0, 4, 1, 3)


def full_map_case(permute=False):
    """One tile that meets more than 128 classes: a read of 150 distinct 6-base roots, each three times, with 150
    regions carrying them; around it reads of a few of the roots.  The regions have no anchors, so every (read, region)
    is a pair of kind 0 and carries m(r, class of the region)."""
    rng = np.random.default_rng(12)
    roots = distinct_roots(150)
    anchors = [("", "")] * 150
    big = "".join(r * 3 for r in roots)
    assert len(big) - 15 + 1 <= TILE
    reads = [roots[3] * 10, big, synth.rand_seq(rng, 500), "".join(r * 4 for r in roots[100:140]), roots[149] * 6,
             big[::-1], synth.revcomp(big)]
    if permute:
        reads = [reads[i] for i in FULL_MAP_PERMUTATION]
    return dict(anchors=anchors, motifs=roots, reads=reads, k=15, max_occ=16, min_hits=1, pct=1)


def kinds_case(seed=5):
    """A 12-region synth.panel plus planted reads: one-anchor reads on each side, wholly in-repeat reads, decoys, a
    region with one empty anchor set and one with two."""
    p = synth.panel(12, anchor_len=400, reads_per_region=2, edge_overlaps=(150,), n_decoys=12, shared=0, seed=seed)
    rng = np.random.default_rng(seed)
    anchors = [[p["ref"][c][st - 400:st], p["ref"][c][en:en + 400]] for c, st, en, _ in p["regions"]]
    anchors[10][0] = "AC" * 30                     # every k-mer periodic: an empty left set
    anchors[11] = ["", "ACGTACG"]                  # two empty sets
    motifs = [u for _, _, _, u in p["regions"]]
    reads = [s for _, s in p["reads"]]
    for g in (0, 3, 5, 10):
        left, right = anchors[g]
        u = motifs[g]
        reads += [synth.apply_errors(rng, left[-300:] + u * 150, "ont"),                    # left only
                  synth.revcomp(synth.apply_errors(rng, u * 150 + right[:300], "ont")),      # right only
                  synth.apply_errors(rng, u * 200, "ont"),                                   # in repeat
                  synth.revcomp(synth.apply_errors(rng, (u * 200)[1:], "hifi")).lower()]
    reads += [synth.rand_seq(rng, 5000)[:2500] + "CAG" * 20 + synth.rand_seq(rng, 2500),      # a decoy with a short run
              right[:200] + synth.rand_seq(rng, 300)]
    order = rng.permutation(len(reads))
    return dict(anchors=[tuple(a) for a in anchors], motifs=motifs, reads=[reads[i] for i in order], k=15, max_occ=16,
                min_hits=4, pct=5)
