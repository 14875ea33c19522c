"""Cases of the sketch-pair contract, shared by the CPU tests (the two restatements against each other) and the GPU tests
(nra_sketch_pairs against the restatement).  A case is a dict(seqs, groups, k, min_shared)."""
import numpy as np

from nanorepeat_amd import synth

MAX_LEN = 2048


def case(seqs, groups, k=13, min_shared=1):
    return dict(seqs=list(seqs), groups=list(groups), k=k, min_shared=min_shared)


def twice(rng, n_kmers, k):
    """A sequence in which every k-mer occurs twice: a random piece of n_kmers windows, an N, the same piece."""
    piece = synth.rand_seq(rng, n_kmers + k - 1)
    return piece + "N" + piece


def edge_case(k):
    """One group.  The indices the GPU test names: 0 empty, 1 k - 1 bases, 2 k bases, 3 k + 1 bases, 4 and 5 two random
    2048-base sequences, 6 all N, 7 = 4 in lower case, 8 = 4 in mixed case, 9 = 4 with an N every k bases (no valid
    window), 10 purely periodic (period 5), 11 the reverse complement of 4, 12 every k-mer twice, 13 = 12's piece once,
    14 = 3 again (a pair of two short sequences)."""
    rng = np.random.default_rng(100 + k)
    a, b = synth.rand_seq(rng, MAX_LEN), synth.rand_seq(rng, MAX_LEN)
    short = synth.rand_seq(rng, k + 1)
    mixed = "".join(c.lower() if i % 3 else c for i, c in enumerate(a))
    with_n = "".join("N" if i % k == k - 1 else c for i, c in enumerate(a))
    two = twice(rng, 300, k)
    seqs = ["", short[:k - 1], short[:k], short, a, b, "N" * 500, a.lower(), mixed, with_n, "ACGTT" * 200,
            synth.revcomp(a), two, two[:300 + k - 1], short]
    return case(seqs, [0] * len(seqs), k)


def offset_case(k=13):
    """16 sequences of 97 = 6 * 16 + 1 bases in one group: packed one after the other, sequence i starts at byte offset
    i mod 16.  Each is a copy of one flank through hifi errors, filled or cut to 97 bases."""
    rng = np.random.default_rng(7)
    flank = synth.rand_seq(rng, 97)
    seqs = [(synth.apply_errors(rng, flank, "hifi") + synth.rand_seq(rng, 8))[:97] for _ in range(16)]
    return case(seqs, [0] * 16, k)


def group_size_case(k=13):
    """Groups of 1, 2, 64, 65 and 257 copies of one flank each (a different flank per group): the pair-free group, the
    block edge of the tile list and several tiles per sequence.  Every second copy goes through hifi errors."""
    rng = np.random.default_rng(11)
    seqs, groups = [], []
    for g, n in enumerate((1, 2, 64, 65, 257)):
        flank = synth.rand_seq(rng, 200)
        for i in range(n):
            seqs.append(synth.apply_errors(rng, flank, "hifi") if i % 2 else flank)
            groups.append(g)
    return case(seqs, groups, k, 20)


def boundary_case(k=13):
    """Two adjacent groups holding the same five sequences, and the same five again with a negative group id."""
    rng = np.random.default_rng(13)
    five = [synth.rand_seq(rng, 300)] * 3 + [synth.rand_seq(rng, 300)] * 2
    return case(five * 3, [4] * 5 + [5] * 5 + [-1, -2, -1, -7, -1], k)


def noisy_case(model, k=13, min_shared=8):
    """300 seeded 500-base flanks in 30 groups of 10: per group three loci of 4, 3 and 3 noisy copies."""
    rng = np.random.default_rng(17 if model == "ont" else 19)
    seqs, groups = [], []
    for g in range(30):
        for n in (4, 3, 3):
            flank = synth.rand_seq(rng, 500)
            for _ in range(n):
                x = synth.apply_errors(rng, flank, model)[:MAX_LEN]
                seqs.append(synth.revcomp(x) if rng.random() < 0.5 else x)
                groups.append(g)
    return case(seqs, groups, k, min_shared)


def full_case(k=13):
    """20 full 2048-base sequences in one group (the LDS set at its fullest): ten random ones, each with a noisy copy cut
    to 2048 bases."""
    rng = np.random.default_rng(23)
    seqs = []
    for _ in range(10):
        x = synth.rand_seq(rng, MAX_LEN)
        seqs += [x, (synth.apply_errors(rng, x, "hifi") + synth.rand_seq(rng, 100))[:MAX_LEN]]
    return case(seqs, [3] * len(seqs), k, 4)


def small_cases():
    """Small versions of every case for the CPU comparison of the two restatements."""
    rng = np.random.default_rng(29)
    out = []
    for k in (11, 13, 15):
        c = edge_case(k)
        c["seqs"] = [s[:400] for s in c["seqs"]]
        out.append(c)
    out.append(offset_case())
    c = boundary_case()
    out.append(c)
    c = noisy_case("ont")
    out.append(case(c["seqs"][:40], c["groups"][:40], 13, 8))
    perm = rng.permutation(40)
    out.append(case([c["seqs"][i] for i in perm], [c["groups"][i] * 7 + 3 for i in perm], 13, 8))
    return out


def loci_panel(model, seed=41):
    """Reads for the locus commands: two AAGGG loci with different flanks -- A with two size alleles (8 reads of 60 and 8
    of 100 copies), B with 6 spanning reads of 120 copies and 4 reads that start inside the run (left-open as written)
    -- an AAAAG locus C (5 reads of 70 copies) and 10 decoys holding (motif)x20.  Every read goes through the `model`
    error channel and every second one is reverse-complemented; the file order is shuffled.  Returns dict(reads=[(name,
    seq)], locus={name: "A" | "B" | "C"} of the spanning reads, open=the names of B's open reads, alleles=(60, 100))."""
    import scan_cases
    rng = np.random.default_rng(seed)
    flanks = {x: (synth.rand_seq(rng, 1500), synth.rand_seq(rng, 1500)) for x in "ABC"}
    plan = [("A", "AAGGG", 60, 8, False), ("A", "AAGGG", 100, 8, False), ("B", "AAGGG", 120, 6, False),
            ("B", "AAGGG", 90, 4, True), ("C", "AAAAG", 70, 5, False)]
    reads, locus, opened = [], {}, set()
    for x, unit, copies, n, is_open in plan:
        left, right = flanks[x]
        for i in range(n):
            lo = int(rng.integers(0, 300))
            seq = (unit * copies if is_open else left[lo:] + unit * copies) + right[:1500 - int(rng.integers(0, 300))]
            seq = synth.apply_errors(rng, seq, model)
            name = f"{x}{'open' if is_open else copies}_{i}"
            reads.append((name, synth.revcomp(seq) if len(reads) % 2 else seq))
            if is_open:
                opened.add(name)
            else:
                locus[name] = x
    for i, motif in enumerate((scan_cases.TABLE_MOTIFS * 2)[:10]):
        reads.append((f"decoy{i:02d}", scan_cases.decoy_reads(rng, motif, 1)[0]))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    return dict(reads=reads, locus=locus, open=opened, alleles=(60, 100))
