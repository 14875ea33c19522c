"""Cases shared by test_paths_cpu.py and test_paths_gpu.py: a small panel for the round-3 alignment file and the
checks of a PAF row against its CIGAR."""
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
