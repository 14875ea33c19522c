"""Inputs of the repeat scan's tests (CPU and GPU): each case is dict(reads, k, max_gap, min_span).  Seeded; the CPU
tests hold the two restatements equal on every case and check that a case holds what it is for."""
import numpy as np

from nanorepeat_amd import synth

TILE = 4096


def revcomp(s):
    return synth.revcomp(s)


def pure(motif, n, phase=0):
    """n bases of the motif's pure repeat, starting at base `phase` of the motif."""
    return (motif * (n // len(motif) + 2))[phase % len(motif):][:n]


def case(reads, k, max_gap=100, min_span=None):
    return dict(reads=list(reads), k=k, max_gap=max_gap, min_span=k if min_span is None else min_span)


def edge_case(k):
    """Reads around k bases, bytes other than ACGT, case, the smallest period, strands and the self-complementary
    classes."""
    rng = np.random.default_rng(100 + k)
    flank = lambda n: synth.rand_seq(rng, n)
    planted = flank(150) + pure("AAGGG", 300) + flank(170)
    at, acgt = flank(90) + pure("AT", 120) + flank(60), flank(70) + pure("ACGT", 160, 1) + flank(95)
    reads = ["A" * (k - 1), "A" * k, "A" * (k + 1), "CAG" * 3 + "C" * (k - 9), "", "N" * 300,
             pure("cag", 200), pure("CAG", 100) + pure("cag", 77, 1),
             pure("AAAG", 150) + "N" + pure("AAAG", 150, 2), pure("AAAG", 40) + "n" + pure("AAAG", 40, 1),
             "A" * 100, pure("AC", 100), pure("ACG", 100), pure("AACAAC", 60), pure("ACACAT", 90), pure("AAAAAC", 90),
             planted, revcomp(planted), at, revcomp(at), acgt, revcomp(acgt),
             pure("GGCCCC", 200) + flank(30) + pure("CCCCGG", 200), flank(400)]
    return case(reads, k, max_gap=5)


def boundary_case(k=11):
    """Pure runs whose first and whose last window sit at b - 1, b, b + 1 for b in {16, 1024, 4096, 8192}: the edges of
    a lane's 16 positions, of a wave and of a tile.  Then a pure 10 000-base read (three tiles), 16 reads packed back to
    back so that every base offset mod 16 occurs, and a read that ends in the class its successor starts in."""
    rng = np.random.default_rng(7)
    reads = []
    for b in (16, 1024, 4096, 8192):
        for d in (-1, 0, 1):
            reads.append(synth.rand_seq(rng, b + d - 1) + "C" + pure("AAG", 300))       # first window at b + d
            reads.append(pure("AAG", b + d + k) + "C" + synth.rand_seq(rng, 40))         # last window at b + d
    reads.append(pure("AG", 10000))
    for i in range(16):
        n = 16 * (3 + i) + 1                                                           # offsets 0, 1, ..., 15 mod 16
        reads.append(synth.rand_seq(rng, n - 40 - i) + pure("ACCT", 40 + i, i))
    reads.append(synth.rand_seq(rng, 60) + pure("AAAT", 80))
    reads.append(pure("AAAT", 80, 80) + synth.rand_seq(rng, 33))                        # the last read ends the buffer
    return case(reads, k, max_gap=3)


def gap_read(k=11):
    """Two pure runs of one class with a spacer of another class between them; the spacer is a short island of its own."""
    return pure("AC", 120) + pure("AAG", 60) + pure("AC", 120)


def fuzz_case(n_reads=300, seed=11, k=11):
    """Random reads of 20..3000 bases with planted runs of random primitive motifs of 1..6 bases, through `ont` and
    `hifi` errors, both strands, and one read of 70 000 bases."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads + 1):
        n = 70000 if i == n_reads else int(rng.integers(20, 3001))
        parts, size = [], 0
        while size < n:
            if rng.random() < 0.5:
                part = synth.rand_seq(rng, int(rng.integers(1, 400)))
            else:
                motif = synth.primitive_unit(rng, int(rng.integers(1, 7)))
                part = pure(motif, int(rng.integers(8, 700)), int(rng.integers(0, 6)))
            parts.append(part)
            size += len(part)
        s = synth.apply_errors(rng, "".join(parts)[:n], ("ont", "hifi")[i % 2])
        if i % 3 == 0:
            s = revcomp(s)
        if i % 11 == 0:
            s = s.lower()
        if i % 13 == 0 and len(s) > 50:
            s = s[:40] + "N" + s[41:]
        reads.append(s)
    return case(reads, k, max_gap=100, min_span=50)


# ----------------------------------------------------------------------------------- the defaults
TABLE_MOTIFS = ("A", "AC", "GAA", "CAG", "AAAG", "AAGGG", "GGCCCC")     # section 23.4's: every period 1..6


def planted_reads(rng, motif, model, n_reads):
    """Wholly in-repeat reads of 300..3000 bases, every second one reverse-complemented."""
    out = []
    for i in range(n_reads):
        n = int(rng.integers(300, 3001))
        s = synth.apply_errors(rng, pure(motif, n, i), model)
        out.append(revcomp(s) if i % 2 else s)
    return out


def decoy_reads(rng, motif, n_reads, model="ont"):
    """5 kb random reads holding (motif)x20 through the error channel; motif None: random reads."""
    out = []
    for i in range(n_reads):
        if motif is None:
            out.append(synth.rand_seq(rng, 5000))
            continue
        run = motif * 20
        at = int(rng.integers(0, 5000 - len(run)))
        s = synth.apply_errors(rng, synth.rand_seq(rng, at) + run + synth.rand_seq(rng, 5000 - len(run) - at), model)
        out.append(revcomp(s) if i % 2 else s)
    return out
