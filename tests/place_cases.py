"""Cases of the placement contract, shared by the CPU tests (the two restatements against each
other) and the GPU tests (nra_place_* against the restatement), and the planted references of place.py's tests.  A case
is a dict(queries, chunks, k, max_occ, bin, max_target_occ, min_votes) with chunks = [(contig, pos0, bases)] in the order
they are scanned."""
import numpy as np

from nanorepeat_amd import synth

MAX_LEN = 2048
CEILING = 1024      # NRA_PLACE_OCC_CEILING
TILE = 4096         # the tile of k_place_hits; the GPU tests check it against the handle's tile_windows


def case(queries, chunks, k=13, max_occ=16, bin=64, max_target_occ=64, min_votes=2):
    return dict(queries=list(queries), chunks=list(chunks), k=k, max_occ=max_occ, bin=bin, max_target_occ=max_target_occ,
                min_votes=min_votes)


def cut_at(contig, seq, k, cuts, pos0=0):
    """The chunks of one contig cut at the positions `cuts` (ascending, inside the contig), overlapping by k - 1 bases:
    every window of the contig lies wholly inside exactly one of them."""
    edges = [0] + list(cuts) + [len(seq)]
    return [(contig, pos0 + a, seq[a:min(len(seq), b + k - 1)]) for a, b in zip(edges[:-1], edges[1:])]


def cut(contig, seq, k, size, pos0=0):
    """... in chunks of `size` bases (the last one shorter)."""
    return cut_at(contig, seq, k, list(range(size - (k - 1), len(seq) - (k - 1), size - (k - 1))), pos0)


def edge_case(k):
    """The queries the GPU test names: 0 empty, 1 k - 1 bases, 2 k bases, 3 k + 1 bases, 4 a random 2048-base sequence,
    5 all N, 6 = 4 in lower case, 7 = 4 in mixed case, 8 = 4 with an N every k bases (no valid window), 9 purely periodic
    (period 5), 10 another random 2048-base sequence.  Contig 0 holds query 3 at 300 and query 4 at 300 + k + 1 + 100;
    contig 1 holds the reverse complement of query 4 at 150 and query 10, in lower case, at 150 + 2048 + 50; contig 2
    is contig 1's chunk again under another label and at positions that end at 2^30."""
    rng = np.random.default_rng(200 + k)
    a, b = synth.rand_seq(rng, MAX_LEN), synth.rand_seq(rng, MAX_LEN)
    short = synth.rand_seq(rng, k + 1)
    mixed = "".join(c.lower() if i % 3 else c for i, c in enumerate(a))
    with_n = "".join("N" if i % k == k - 1 else c for i, c in enumerate(a))
    queries = ["", short[:k - 1], short[:k], short, a, "N" * 500, a.lower(), mixed, with_n, "ACGTT" * 200, b]
    c0 = synth.rand_seq(rng, 300) + short + synth.rand_seq(rng, 100) + a + synth.rand_seq(rng, 200)
    c1 = synth.rand_seq(rng, 150) + synth.revcomp(a) + synth.rand_seq(rng, 50) + b.lower() + "NNN" + synth.rand_seq(rng, 40)
    return case(queries, [(0, 0, c0), (1, 0, c1), (2, (1 << 30) - len(c1), c1)], k)


def offset_case(k=13):
    """16 queries of 97 = 6 * 16 + 1 bases, packed one after the other: query i starts at byte offset i mod 16.  Each is
    a copy of one flank through hifi errors, filled or cut to 97 bases; the contig holds the flank and its reverse
    complement."""
    rng = np.random.default_rng(7)
    flank = synth.rand_seq(rng, 97)
    queries = [(synth.apply_errors(rng, flank, "hifi") + synth.rand_seq(rng, 8))[:97] for _ in range(16)]
    contig = synth.rand_seq(rng, 333) + flank + synth.rand_seq(rng, 211) + synth.revcomp(flank) + synth.rand_seq(rng, 77)
    return case(queries, [(0, 0, contig)], k, max_occ=32)


def count_case(n, k=13):
    """n queries of 40 bases; the contig holds up to five of them (the first, the last and three between), every second
    one reverse-complemented."""
    rng = np.random.default_rng(300 + n)
    queries = [synth.rand_seq(rng, 40) for _ in range(n)]
    contig = synth.rand_seq(rng, 100)
    for x, q in enumerate(sorted({0, n // 3, n // 2, (2 * n) // 3, n - 1})):
        contig += (synth.revcomp(queries[q]) if x % 2 else queries[q]) + synth.rand_seq(rng, 60)
    return case(queries, [(5, 1000, contig)], k)


def tile_case(n_win, k=13):
    """One chunk of n_win windows whose first windows are query 0's and whose last windows are query 1's (reverse
    complemented): hits in the first and in the last window of the chunk."""
    rng = np.random.default_rng(400 + n_win % 1000)
    queries = [synth.rand_seq(rng, 30), synth.rand_seq(rng, 30)]
    n = n_win + k - 1
    return case(queries, [(0, 77, queries[0] + synth.rand_seq(rng, n - 60) + synth.revcomp(queries[1]))], k)


def cut_case(k=13, cuts=None):
    """One contig of 3000 bases with four queries planted (one over a cut), cut at 16 places of every residue mod 16, or
    uncut (cuts=())."""
    rng = np.random.default_rng(500)
    queries = [synth.rand_seq(rng, 120) for _ in range(4)]
    contig = synth.rand_seq(rng, 470) + queries[0] + synth.rand_seq(rng, 300) + synth.revcomp(queries[1]) + \
        synth.rand_seq(rng, 500) + queries[2] + synth.rand_seq(rng, 700) + queries[3]
    contig += synth.rand_seq(rng, 3000 - len(contig))
    if cuts is None:
        cuts = [500 + 97 * i for i in range(16)]            # 97 = 1 mod 16
    return case(queries, cut_at(3, contig, k, cuts, 160), k)


def two_contig_case(k=13):
    """Two contigs in chunks of 700 bases: as they come, reversed, and interleaved."""
    rng = np.random.default_rng(600)
    queries = [synth.rand_seq(rng, 200) for _ in range(3)]
    c0 = synth.rand_seq(rng, 900) + queries[0] + synth.rand_seq(rng, 800) + synth.revcomp(queries[1]) + synth.rand_seq(rng, 400)
    c1 = synth.rand_seq(rng, 300) + queries[2] + synth.rand_seq(rng, 1500) + queries[0] + synth.rand_seq(rng, 100)
    a, b = cut(0, c0, k, 700), cut(1, c1, k, 700)
    mixed = [x for pair in zip(a, b) for x in pair] + a[len(b):] + b[len(a):]
    return [case(queries, a + b, k), case(queries, (a + b)[::-1], k), case(queries, mixed, k)]


def bin_edge_case(bin, k=13):
    """One query of 300 bases on one contig per start diagonal d: d at 2 bin - 1, 2 bin, 2 bin + 1, at -1, 0, 1 and, where
    the query is long enough to overhang the contig's start that far, at -bin - 1, -bin, -bin + 1.  Returns (case, the
    diagonals): contig t holds diagonal ds[t]."""
    rng = np.random.default_rng(700 + bin)
    query = synth.rand_seq(rng, 300)
    ds = [2 * bin - 1, 2 * bin, 2 * bin + 1, -1, 0, 1] + ([-bin - 1, -bin, -bin + 1] if bin <= 64 else [])
    ds = sorted(set(ds))
    chunks = [(t, 0, (synth.rand_seq(rng, d) + query if d >= 0 else query[-d:]) + synth.rand_seq(rng, 50))
              for t, d in enumerate(ds)]
    return case([query], chunks, k, bin=bin), ds


def reverse_edge_case(bin=64, k=13):
    """The reverse complement of one 300-base query at contig positions bin - 1, bin and bin + 1, and overhanging the
    contig's start by 1 and by bin + 1: the diagonals of strand 1."""
    rng = np.random.default_rng(800)
    query = synth.rand_seq(rng, 300)
    rc = synth.revcomp(query)
    ds = [-bin - 1, -1, bin - 1, bin, bin + 1]
    chunks = [(t, 0, (synth.rand_seq(rng, d) + rc if d >= 0 else rc[-d:]) + synth.rand_seq(rng, 50))
              for t, d in enumerate(ds)]
    return case([query], chunks, k, bin=bin), ds


def occ_case(k=13):
    """max_occ = 3: X is three queries (kept), Y four (masked).  The contig holds X five times and Y once, N between:
    every key has occ = 5."""
    rng = np.random.default_rng(900)
    x, y = synth.rand_seq(rng, 150), synth.rand_seq(rng, 150)
    contig = "N".join([synth.rand_seq(rng, 90)] + [x] * 5 + [y, synth.rand_seq(rng, 90)])
    return case([x] * 3 + [y] * 4, [(0, 0, contig)], k, max_occ=3, max_target_occ=5)


def hot_case(k=13):
    """One 2 kb query; the target is the query CEILING + 1 times over, in chunks of 2^19 bases: every key is over the
    ceiling."""
    rng = np.random.default_rng(1000)
    query = synth.rand_seq(rng, 2000)
    return case([query], cut(0, query * (CEILING + 1), k, 1 << 19), k, max_target_occ=CEILING, min_votes=1)


def dense_case(k=13):
    """One 2 kb query eight times over in one chunk: all but a few of its 16 000 windows are hits, four tiles full of
    records."""
    rng = np.random.default_rng(1100)
    query = synth.rand_seq(rng, 2000)
    return case([query], [(0, 0, query * 8)], k, max_target_occ=8, min_votes=100)


def noisy_case(model, k=13, n_sides=200, contig_len=500_000, n_contigs=4):
    """n_sides 1 kb sides cut from a random reference of n_contigs contigs, each through the `model` error channel and
    every second one reverse-complemented.  Returns (case, truth): truth[q] = (contig, strand, start)."""
    rng = np.random.default_rng(1200 if model == "ont" else 1300)
    contigs = [synth.rand_seq(rng, contig_len) for _ in range(n_contigs)]
    queries, truth = [], []
    for q in range(n_sides):
        t, at = int(rng.integers(n_contigs)), int(rng.integers(0, contig_len - 1000))
        side = synth.apply_errors(rng, contigs[t][at:at + 1000], model)[:MAX_LEN]
        queries.append(synth.revcomp(side) if q % 2 else side)
        truth.append((t, q % 2, at))
    chunks = [c for t, seq in enumerate(contigs) for c in cut(t, seq, k, 1 << 18)]
    return case(queries, chunks, k, bin=64, min_votes=8), truth


def small_cases():
    """Small versions of every case for the CPU comparison of the two restatements."""
    out = []
    for k in (11, 13, 15):
        c = edge_case(k)
        c["queries"] = [s[:300] for s in c["queries"]]
        c["chunks"] = [(t, pos0 + 250, bases[250:1100]) for t, pos0, bases in c["chunks"]]
        out.append(c)
    out.append(offset_case())
    out.append(count_case(65))
    out.append(tile_case(500))
    out += [cut_case(), cut_case(cuts=())] + two_contig_case()
    out += [bin_edge_case(bin)[0] for bin in (1, 64, 4096)] + [reverse_edge_case()[0]]
    c = occ_case()
    out += [c, dict(c, max_target_occ=4), dict(c, max_occ=2), dict(c, max_occ=4, min_votes=137)]
    c, _ = noisy_case("ont", n_sides=6, contig_len=3000, n_contigs=2)
    out += [c, dict(c, bin=16, min_votes=3)]
    return out


# ------------------------------------------------------------------ planted references for place.py (section 31.3)
UNIT = "AAGGG"


def _flanks(rng, left_len=1200, right_len=1200):
    """A left flank that ends in C and a right flank that starts with T: neither continues an AAGGG tract."""
    return synth.rand_seq(rng, left_len - 1) + "C", "T" + synth.rand_seq(rng, right_len - 1)


def planted_panel(model=None, seed=51):
    """Three contigs of about 50 kb and reads that carry expanded AAGGG tracts at loci planted in them.  The loci, by the
    name their reads start with: p3 (chrA, + strand, 3 copies in the reference), p11 (chrB, reads reverse-complemented,
    11 copies), p0 (chrC, no copy: the flanks touch), amb (the whole locus on chrA and on chrC), disc (left flank on
    chrA, right flank on chrB), openr (a read that starts inside the tract: its right flank on chrB), openl (a read that
    ends inside it: its left flank on chrC), unp (flanks that are nowhere), overs (on chrC, 400 bases behind the
    contig's start: the read's left side overhangs the start by 600) and overe (on chrA, 300 bases before the contig's
    end).  model: None for error-free reads, else every read goes through that error channel.  Returns dict(ref={name:
    sequence}, reads=[(name, sequence)], truth={locus: (chrom, strand, tract start, tract end) or None})."""
    rng = np.random.default_rng(seed)
    fl = {x: _flanks(rng) for x in ("p3", "p11", "p0", "amb", "openr", "openl")}
    fl["overs"] = _flanks(rng, 400, 1200)
    fl["overe"] = _flanks(rng, 1200, 300)
    disc_left, disc_right = _flanks(rng)
    copies = dict(p3=3, p11=11, p0=0, amb=3, openr=5, openl=4, overs=3, overe=3)
    seg = {x: fl[x][0] + UNIT * copies[x] + fl[x][1] for x in fl}
    layout = dict(
        chrA=[5000, "p3", 4000, "amb", 3000, disc_left, 6000, None, 21000, "overe"],
        chrB=[7000, "p11", 5000, disc_right, 5000, "openr", 26000],
        chrC=["overs", 6000, "p0", 4000, "amb", 3000, "openl", 26000])
    ref, truth = {}, {x: None for x in ("amb", "disc", "unp")}
    for name, parts in layout.items():
        contig = ""
        for part in parts:
            if isinstance(part, int):
                contig += synth.rand_seq(rng, part)
            elif part in seg:
                if part != "amb":
                    at = len(contig) + len(fl[part][0])
                    truth[part] = (name, "-" if part == "p11" else "+", at, at + len(UNIT) * copies[part])
                contig += seg[part]
            elif part is not None:
                contig += part
        ref[name] = contig
    foreign = lambda n: synth.rand_seq(rng, n)
    reads = []
    for x, n_copies in (("p3", 60), ("p11", 70), ("p0", 50), ("amb", 60), ("overs", 60), ("overe", 60)):
        left, right = fl[x]
        left = foreign(700) + left if x == "overs" else left[-1100:]
        right = right + foreign(800) if x == "overe" else right[:1100]
        for i in (1, 2):
            seq = left + UNIT * n_copies + right
            reads.append((f"{x}_{i}", synth.revcomp(seq) if x == "p11" else seq))
    reads.append(("disc_1", disc_left[-1100:] + UNIT * 60 + disc_right[:1100]))
    reads.append(("unp_1", _flanks(rng)[0] + UNIT * 60 + _flanks(rng)[1]))
    reads.append(("openr_1", UNIT * 80 + fl["openr"][1][:1100]))
    reads.append(("openl_1", fl["openl"][0][-1100:] + UNIT * 80))
    if model is not None:
        reads = [(n, synth.apply_errors(rng, s, model)) for n, s in reads]
    return dict(ref=ref, reads=reads, truth=truth)


def write_panel(p, directory, wrap=70):
    """The panel's reads as reads.fastq and its reference as ref.fa (lines of `wrap` bases) in `directory`; returns the
    two paths."""
    import os
    fq, fa = os.path.join(str(directory), "reads.fastq"), os.path.join(str(directory), "ref.fa")
    with open(fq, "w") as f:
        f.write("".join(f"@{n}\n{s}\n+\n{'5' * len(s)}\n" for n, s in p["reads"]))
    with open(fa, "w") as f:
        for name, seq in p["ref"].items():
            f.write(f">{name} planted\n" + "".join(seq[i:i + wrap] + "\n" for i in range(0, len(seq), wrap)))
    return fq, fa


def loci_panel(model, seed=61):
    """sketch_cases.loci_panel with a reference: three contigs of 30 kb, each with one locus at 12 000 whose reference
    tract is short -- A on chrA ((AAGGG)10; 8 reads of 60 and 8 of 100 copies, all as the reference reads), B on chrB
    ((AAGGG)12; 6 spanning reads of 120 copies and 4 that start inside the run, every second read reverse-complemented)
    and C on chrC ((AAAAG)8; 5 reads of 70 copies, all reverse-complemented) -- and 10 decoys holding (motif)x20.  Every
    read goes through the `model` error channel; the file order is shuffled.  Returns dict(ref, reads, locus={name: "A"
    | "B" | "C"} of the spanning reads, strand={name: "+" | "-"}, truth={locus: (chrom, tract start, tract end)},
    alleles=(60, 100))."""
    import scan_cases
    rng = np.random.default_rng(seed)
    units = dict(A=("AAGGG", 10), B=("AAGGG", 12), C=("AAAAG", 8))
    ref, truth, flanks = {}, {}, {}
    for x, (unit, copies) in units.items():
        left, right = synth.rand_seq(rng, 11999) + "C", "T" + synth.rand_seq(rng, 17999)
        ref[f"chr{x}"] = left + unit * copies + right
        truth[x] = (f"chr{x}", 12000, 12000 + len(unit) * copies)
        flanks[x] = (left[-1500:], right[:1500])
    plan = [("A", 60, 8, False), ("A", 100, 8, False), ("B", 120, 6, False), ("B", 90, 4, True), ("C", 70, 5, False)]
    reads, locus, strand = [], {}, {}
    for x, copies, n, is_open in plan:
        left, right = flanks[x]
        unit = units[x][0]
        for i in range(n):
            lo = int(rng.integers(0, 300))
            seq = (unit * copies if is_open else left[lo:] + unit * copies) + right[:1500 - int(rng.integers(0, 300))]
            seq = synth.apply_errors(rng, seq, model)
            name = f"{x}{'open' if is_open else copies}_{i}"
            reverse = x == "C" or (x == "B" and i % 2 == 1)
            reads.append((name, synth.revcomp(seq) if reverse else seq))
            strand[name] = "-" if reverse else "+"
            if not is_open:
                locus[name] = x
    for i, motif in enumerate((scan_cases.TABLE_MOTIFS * 2)[:10]):
        reads.append((f"decoy{i:02d}", scan_cases.decoy_reads(rng, motif, 1)[0]))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    return dict(ref=ref, reads=reads, locus=locus, strand=strand, truth=truth, alleles=(60, 100))
