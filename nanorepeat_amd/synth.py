"""Seeded synthetic workloads for the repeat-size scoring path.

All generators are deterministic in `seed`.  Reads are the already-trimmed *core*
sequences the 1D path receives (last `flank` bp of the left flank + unit * k_true +
first `flank` bp of the right flank, through a per-base error channel), or full amplicon
reads for the joint path.
"""
import numpy as np

SEED = 20260116
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

# substitution / insertion / deletion rates (cf. nanoRepeat_bam.py:694-701 totals)
ERROR_MODELS = {
    "ont": (0.025, 0.015, 0.03),
    "ont_q20": (0.010, 0.007, 0.013),
    "hifi": (0.003, 0.007, 0.010),
    "none": (0.0, 0.0, 0.0),
}


def rand_seq(rng, n):
    return _BASES[rng.integers(0, 4, size=n)].tobytes().decode()


def rand_unit(rng, m):
    """Random motif of length m that is not a homopolymer."""
    while True:
        u = rand_seq(rng, m)
        if len(set(u)) > 1 or m == 1:
            return u


def apply_errors(rng, seq, model):
    """Per-base channel: delete, else maybe substitute; then maybe insert a uniform base."""
    sub, ins, dele = ERROR_MODELS[model] if isinstance(model, str) else model
    a = np.frombuffer(seq.encode(), dtype=np.uint8)
    n = len(a)
    if n == 0 or (sub == 0 and ins == 0 and dele == 0):
        return seq
    u = rng.random(n)
    keep = u >= dele
    do_sub = keep & (u < dele + sub)
    b = a.copy()
    if do_sub.any():
        # substitute with one of the three other bases
        idx = np.searchsorted(_BASES, b[do_sub])
        b[do_sub] = _BASES[(idx + rng.integers(1, 4, size=int(do_sub.sum()))) % 4]
    do_ins = rng.random(n) < ins
    out = np.empty(2 * n, dtype=np.uint8)
    mask = np.zeros(2 * n, dtype=bool)
    out[0::2] = b
    mask[0::2] = keep
    out[1::2] = _BASES[rng.integers(0, 4, size=n)]
    mask[1::2] = do_ins
    return out[mask].tobytes().decode()


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTNacgtn", "TGCANtgcan"))


def reference_window(r2, fast_mode=False):
    """k window of round3_align (nanoRepeat_bam.py:463-472), pinned by tests/golden."""
    buffer = max(15, int(r2 * 0.05))
    if buffer > 150:
        buffer = 150
    if fast_mode:
        buffer = 15
    kmax = int(r2 + buffer)
    kmin = int(r2 - buffer)
    if kmin < 0:
        kmin = 0
    return kmin, kmax


def make_1d(n_reads, unit, alleles, model="ont", kwin=None, flank=100, anchor=1000, seed=SEED,
            fast_mode=False, rng=None):
    """One region, diploid (or any list of) alleles.  kwin=(kmin,kmax) fixes every read's
    window; otherwise the reference window rule is applied to r2 = k_true + N(0,1)."""
    rng = rng or np.random.default_rng(seed)
    left, right = rand_seq(rng, anchor), rand_seq(rng, anchor)
    reads, kt = [], []
    kmin = np.zeros(n_reads, np.int32)
    kmax = np.zeros(n_reads, np.int32)
    for i in range(n_reads):
        k = int(alleles[int(rng.integers(0, len(alleles)))])
        core = left[len(left) - flank:] + unit * k + right[:flank]
        reads.append(apply_errors(rng, core, model))
        kt.append(k)
        if kwin is not None:
            kmin[i], kmax[i] = kwin
        else:
            r2 = max(0.0, k + float(rng.normal(0.0, 1.0)))
            kmin[i], kmax[i] = reference_window(r2, fast_mode)
    return dict(regions=[(left, unit, right)], reads=reads, kmin=kmin, kmax=kmax,
                read_region=None, k_true=np.array(kt, np.int32))


def apply_errors_batch(rng, seqs, model):
    """apply_errors over many sequences in one vectorised pass (same channel, its own draw order)."""
    sub, ins, dele = ERROR_MODELS[model] if isinstance(model, str) else model
    lens = np.fromiter((len(x) for x in seqs), np.int64, len(seqs))
    a = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    n = len(a)
    owner = np.repeat(np.arange(len(seqs)), lens)
    u = rng.random(n)
    keep = u >= dele
    do_sub = keep & (u < dele + sub)
    b = a.copy()
    if do_sub.any():
        idx = np.searchsorted(_BASES, b[do_sub])
        b[do_sub] = _BASES[(idx + rng.integers(1, 4, size=int(do_sub.sum()))) % 4]
    do_ins = rng.random(n) < ins
    out = np.empty(2 * n, dtype=np.uint8)
    mask = np.zeros(2 * n, dtype=bool)
    out[0::2] = b
    mask[0::2] = keep
    out[1::2] = _BASES[rng.integers(0, 4, size=n)]
    mask[1::2] = do_ins
    new_len = np.bincount(np.repeat(owner, 2)[mask], minlength=len(seqs))
    text = out[mask].tobytes().decode()
    off = np.r_[0, np.cumsum(new_len)]
    return [text[off[i]:off[i + 1]] for i in range(len(seqs))]


def make_1d_batch(n_reads, unit, alleles, model, rng, flank=100, anchor=1000, fast_mode=False):
    """make_1d with the reference window rule, generated in one vectorised pass (config 4 needs a
    million reads)."""
    left, right = rand_seq(rng, anchor), rand_seq(rng, anchor)
    kt = np.asarray(alleles, np.int32)[rng.integers(0, len(alleles), size=n_reads)]
    cores = {int(k): left[len(left) - flank:] + unit * int(k) + right[:flank] for k in set(kt.tolist())}
    reads = apply_errors_batch(rng, [cores[int(k)] for k in kt], model)
    r2 = np.maximum(0.0, kt + rng.normal(0.0, 1.0, size=n_reads))
    buf = np.full(n_reads, 15.0) if fast_mode else np.clip(np.floor(r2 * 0.05), 15, 150)    # reference_window, vectorised
    kmin = np.maximum(np.trunc(r2 - buf), 0).astype(np.int32)
    kmax = np.trunc(r2 + buf).astype(np.int32)
    return dict(regions=[(left, unit, right)], reads=reads, kmin=kmin, kmax=kmax, read_region=None, k_true=kt)


def config2(n_reads=10000, seed=SEED):
    """BASELINE config 2: 10k ONT-error reads, motif TATTG, k in [5,200], alleles 40/150."""
    return make_1d(n_reads, "TATTG", (40, 150), "ont", kwin=(5, 200), seed=seed)


def config5(n_reads=1000, seed=SEED):
    """BASELINE config 5: HiFi model, 5 bp motif, k in [5,500] wide sweep, alleles 60/420."""
    return make_1d(n_reads, "TATTG", (60, 420), "hifi", kwin=(5, 500), seed=seed)


def config4_region(g, seed=SEED):
    """Descriptor of region g of config 4 (no reads): motif, the two alleles and the generator that
    continues into the flanks and reads, so that any rank can materialise any subset of regions."""
    rng = np.random.default_rng([seed, g])
    m = int(rng.integers(3, 7))
    unit = rand_unit(rng, m)
    alleles = (int(rng.integers(10, 121)), int(rng.integers(10, 121)))
    return dict(m=m, unit=unit, alleles=alleles, rng=rng)


def config4_region_cost(desc, reads_per_region, flank=100, anchor=1000):
    """Expected executed cells of a region (what a shard costs; see dist.executed_cells), from its
    descriptor alone: error-free core length and the reference window around each allele."""
    from .dist import padded_rows
    cost = 0
    for a in desc["alleles"]:
        q = 2 * flank + desc["m"] * a
        cost += int(padded_rows(q, desc["m"])) * (2 * anchor + desc["m"] * reference_window(float(a))[1] + 31 * (desc["m"] + 1))
    return cost * reads_per_region // len(desc["alleles"])


def config4(n_regions=1000, reads_per_region=1000, seed=SEED, only=None):
    """BASELINE config 4: many regions, mixed 3-6 bp motifs, reference window rule.  `only`: the
    region numbers to materialise (a rank's shard); read_region then indexes the returned list and
    `region_id` / `read_id` give the global numbering (read_id = region * reads_per_region + i)."""
    ids = range(n_regions) if only is None else sorted(int(g) for g in only)
    regions, reads, rr, kt, gid, rid = [], [], [], [], [], []
    kmins, kmaxs = [], []
    for j, g in enumerate(ids):
        desc = config4_region(g, seed)
        d = make_1d_batch(reads_per_region, desc["unit"], desc["alleles"], "ont_q20", desc["rng"])
        regions.append(d["regions"][0])
        reads += d["reads"]
        rr.append(np.full(reads_per_region, j, np.int32))
        gid.append(g)
        rid.append(g * reads_per_region + np.arange(reads_per_region, dtype=np.int64))
        kmins.append(d["kmin"]); kmaxs.append(d["kmax"]); kt.append(d["k_true"])
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return dict(regions=regions, reads=reads, kmin=cat(kmins, np.int32), kmax=cat(kmaxs, np.int32),
                read_region=cat(rr, np.int32), k_true=cat(kt, np.int32),
                region_id=np.array(gid, np.int64), read_id=cat(rid, np.int64))


def make_joint(n_reads, unit1="CAG", unit2="CCG", mid="CAACAGCCGCCAC",
               alleles=((17, 10), (55, 7)), weights=(0.46, 0.54), model="ont", read_len=1200,
               read_sd=100, anchor=1000, seed=SEED, minus_frac=0.5):
    """BASELINE config 3 shape: HTT-like joint region, full amplicon reads of either strand,
    per-read round-1 ranges [max(0,k-20), k+5) on both axes (nanoRepeat_joint.py:620-637)."""
    rng = np.random.default_rng(seed)
    left, right = rand_seq(rng, anchor), rand_seq(rng, anchor)
    reads, strands, truth, r1, r2 = [], [], [], [], []
    w = np.asarray(weights, float) / np.sum(weights)
    for _ in range(n_reads):
        a = int(rng.choice(len(alleles), p=w))
        k1, k2 = alleles[a]
        core_len = len(unit1) * k1 + len(mid) + len(unit2) * k2
        total = max(core_len + 200, int(rng.normal(read_len, read_sd)))
        fl = (total - core_len) // 2
        fl = min(fl, anchor)
        s = left[len(left) - fl:] + unit1 * k1 + mid + unit2 * k2 + right[:fl]
        s = apply_errors(rng, s, model)
        st = 1
        if rng.random() < minus_frac:
            s = revcomp(s); st = -1
        reads.append(s); strands.append(st); truth.append((k1, k2))
        r1.append((max(0, k1 - 20), k1 + 5))
        r2.append((max(0, k2 - 20), k2 + 5))
    return dict(region=(left, unit1, mid, unit2, right), reads=reads,
                strand=np.array(strands, np.int8), truth=np.array(truth, np.int32),
                range1=np.array(r1, np.int32), range2=np.array(r2, np.int32))


def config3(n_reads=5000, seed=SEED):
    """BASELINE config 3: HTT amplicon joint CAG+CCG quantification, 5k reads."""
    return make_joint(n_reads, seed=seed)


DECOY_KINDS = ("slice", "random", "single", "nrun", "lower", "short")


def panel(n_regions=12, n_chroms=3, anchor_len=1000, reads_per_region=10, model="ont", edge_overlaps=(), n_decoys=0,
          shared=0, shared_len=300, lower_every=7, seed=SEED, units=None):
    """A seeded multi-region panel for the FASTQ / FASTA command (screen + anchors + rounds).

    Regions sit on `n_chroms` chromosomes with at least 4 kb between the windows region +- anchor_len.  Per region:
    `reads_per_region` spanning reads (both anchors, 0-500 bases beyond each), half of them reverse-complemented,
    and, for every overlap o in `edge_overlaps`, two reads that start or end inside an anchor with o bases of it
    (the other side spans); every read goes through the `model` error channel and every `lower_every`-th one is
    lowercase.  `n_decoys` decoys cycle through DECOY_KINDS: a genome slice outside every window, random sequence,
    one anchor only, random sequence with N runs, a lowercase genome slice, a read shorter than 11 bases.
    `shared` > 0: the same `shared_len`-base element replaces the middle of the left anchor of that many regions
    (k-mers shared by more anchors than max_occ are masked by the screen).  `units`: region g's motif is
    units[g % len(units)] instead of a random one of 3..6 bases.

    Returns dict(ref={chrom: seq}, bed=[line], regions=[(chrom, start, end, unit)], reads=[(name, seq)] in a
    shuffled file order, truth={name: (region, k)}, overlap={name: (left bases, right bases) of the anchors}).
    """
    rng = np.random.default_rng(seed)
    element = rand_seq(rng, shared_len)
    gap, extra = 3000, 800
    chroms = {f"chr{c + 1}": [] for c in range(n_chroms)}
    lengths = {name: 0 for name in chroms}
    regions, deserts = [], []              # deserts: (chrom, start, end) outside every window
    for g in range(n_regions):
        chrom = f"chr{g % n_chroms + 1}"
        unit = units[g % len(units)] if units else rand_unit(rng, int(rng.integers(3, 7)))
        kref = int(rng.integers(8, 21))
        left = rand_seq(rng, anchor_len + extra)
        if g < shared:
            mid = len(left) - anchor_len // 2 - shared_len // 2
            left = left[:mid] + element + left[mid + shared_len:]
        parts = [rand_seq(rng, gap), left, unit * kref, rand_seq(rng, anchor_len + extra)]
        at = lengths[chrom]
        deserts.append((chrom, at, at + gap))
        start = at + gap + len(left)
        regions.append((chrom, start, start + len(unit) * kref, unit))
        chroms[chrom] += parts
        lengths[chrom] += sum(len(p) for p in parts)
    for chrom in chroms:                   # a tail gap after the last window
        deserts.append((chrom, lengths[chrom], lengths[chrom] + gap))
        chroms[chrom].append(rand_seq(rng, gap))
    ref = {name: "".join(p) for name, p in chroms.items()}

    raw, truth, overlap = [], {}, {}
    for g, (chrom, st, en, unit) in enumerate(regions):
        kref = (en - st) // len(unit)
        alleles = (max(3, kref + int(rng.integers(-5, 6))), kref + int(rng.integers(6, 25)))
        plan = [(anchor_len + int(rng.integers(0, 501)), anchor_len + int(rng.integers(0, 501)))
                for _ in range(reads_per_region)]
        for o in edge_overlaps:
            plan += [(int(o), anchor_len + int(rng.integers(0, 501))), (anchor_len + int(rng.integers(0, 501)), int(o))]
        for i, (lo, ro) in enumerate(plan):
            k = alleles[i % 2]
            name = f"p{g:04d}_{i:03d}"
            raw.append((name, ref[chrom][st - lo:st] + unit * k + ref[chrom][en:en + ro]))
            truth[name] = (g, k)
            overlap[name] = (min(lo, anchor_len), min(ro, anchor_len))
    seqs = apply_errors_batch(rng, [s for _, s in raw], model) if raw else []
    reads = []
    for i, ((name, _), s) in enumerate(zip(raw, seqs)):
        if rng.random() < 0.5:
            s = revcomp(s)
        if lower_every and i % lower_every == lower_every - 1:
            s = s.lower()
        reads.append((name, s))

    for i in range(n_decoys):
        kind = DECOY_KINDS[i % len(DECOY_KINDS)]
        if kind in ("slice", "lower"):
            chrom, a, b = deserts[int(rng.integers(0, len(deserts)))]
            ln = int(rng.integers(500, b - a))
            p = a + int(rng.integers(0, b - a - ln + 1))
            s = ref[chrom][p:p + ln]
            s = s.lower() if kind == "lower" else s
        elif kind == "random":
            s = rand_seq(rng, int(rng.integers(500, 3000)))
        elif kind == "single":
            chrom, st, en, unit = regions[int(rng.integers(0, n_regions))]
            s = ref[chrom][st - anchor_len:st] + rand_seq(rng, 600)
            s = apply_errors(rng, s, model)
        elif kind == "nrun":
            s = rand_seq(rng, 1500)
            for _ in range(3):
                p = int(rng.integers(0, 1400))
                s = s[:p] + "N" * 50 + s[p + 50:]
        else:
            s = rand_seq(rng, int(rng.integers(1, 11)))
        reads.append((f"decoy_{kind}_{i:04d}", s))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    bed = [f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions]
    return dict(ref=ref, bed=bed, regions=regions, reads=reads, truth=truth, overlap=overlap)


def write_panel(p, directory, fmt="fastq", wrap=80):
    """The panel's files: ref.fa, panel.bed and reads.fastq (Phred 20 qualities) / reads.fasta (lines of `wrap`
    bases) / reads.fastq.gz.  Returns (ref, bed, reads) paths."""
    import gzip
    import os
    ref = os.path.join(directory, "ref.fa")
    with open(ref, "w") as f:
        for name, seq in p["ref"].items():
            f.write(f">{name}\n" + "".join(seq[i:i + 80] + "\n" for i in range(0, len(seq), 80)))
    bed = os.path.join(directory, "panel.bed")
    with open(bed, "w") as f:
        f.write("".join(p["bed"]))
    if fmt == "fasta":
        text = "".join(f">{n} synthetic\n" + "".join(s[i:i + wrap] + "\n" for i in range(0, len(s), wrap))
                       for n, s in p["reads"])
    else:
        text = "".join(f"@{n} synthetic\n{s}\n+\n{'5' * len(s)}\n" for n, s in p["reads"])
    reads = os.path.join(directory, {"fastq": "reads.fastq", "fasta": "reads.fasta", "fastq.gz": "reads.fastq.gz"}[fmt])
    with (gzip.open(reads, "wt") if fmt == "fastq.gz" else open(reads, "w")) as f:
        f.write(text)
    return ref, bed, reads


def structure_panel(reads_per_allele=8, anchor_len=1000, model="hifi", seed=SEED):
    """A small panel whose alleles carry planted interruptions, for the repeat structure (structure.py):
    an HTT-like CAG tract ending in CAA CAG ((CAG)17 CAA CAG and (CAG)36 CAA CAG), an FMR1-like CGG tract with two
    AGG interruptions ((CGG)9 AGG (CGG)9 AGG (CGG)m, m = 10 and 28) and a pure TATTG tract (12 and 30 units).  Reads
    span both anchors, half reverse-complemented, through the `model` error channel.  Its own random stream.

    Returns dict(ref, bed, regions, reads, truth) like panel(), plus planted = [per region, per allele in size order:
    [(bases, first slot)] of the planted interruptions].
    """
    rng = np.random.default_rng(seed)
    loci = [("CAG", [("CAG" * 17 + "CAA" + "CAG", [("CAA", 17)]), ("CAG" * 36 + "CAA" + "CAG", [("CAA", 36)])],
             "CAG" * 20 + "CAA" + "CAG"),
            ("CGG", [("CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * m, [("AGG", 9), ("AGG", 19)]) for m in (10, 28)],
             "CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * 12),
            ("TATTG", [("TATTG" * 12, []), ("TATTG" * 30, [])], "TATTG" * 16)]
    gap, extra = 3000, 800
    parts, regions, at = [], [], 0
    for unit, _, ref_tract in loci:
        left, right = rand_seq(rng, anchor_len + extra), rand_seq(rng, anchor_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(ref_tract), unit))
        parts += [rand_seq(rng, gap), left, ref_tract, right]
        at += gap + len(left) + len(ref_tract) + len(right)
    parts.append(rand_seq(rng, gap))
    chrom = "".join(parts)
    raw, truth = [], {}
    for g, ((unit, alleles, _), (_, st, en, _)) in enumerate(zip(loci, regions)):
        for a, (tract, _) in enumerate(alleles):
            for i in range(reads_per_allele):
                lo, ro = anchor_len + int(rng.integers(0, 301)), anchor_len + int(rng.integers(0, 301))
                name = f"s{g}_{a}_{i:02d}"
                raw.append((name, chrom[st - lo:st] + tract + chrom[en:en + ro]))
                truth[name] = (g, a)
    seqs = apply_errors_batch(rng, [s for _, s in raw], model)
    reads = [(name, revcomp(s) if rng.random() < 0.5 else s) for (name, _), s in zip(raw, seqs)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads, truth=truth, planted=[[inter for _, inter in alleles] for _, alleles, _ in loci])


def motif_panel(reads_per_allele=8, anchor_len=1000, model="hifi", seed=SEED):
    """A small panel whose alleles carry planted motif changes, for the tandem motifs (motifs.py): an RFC1-like locus
    (BED AAAAG; alleles (AAAAG)11 and (AAGGG)200), a period change (BED CAG; (CAG)20 and (CCTG)120), a DAB1-like
    insertion (BED ATTTT; (ATTTT)15 and (ATTTT)60 (ATTTC)40 (ATTTT)20) and a pure TATTG control (12 and 30 units).
    The reference holds the BED motif.  Reads span both anchors, half reverse-complemented, through the `model` error
    channel.  Its own random stream.

    Returns dict(ref, bed, regions, reads, truth) like panel(), plus planted = [per region, per allele in the order
    above: (dominant class, units of it)].
    """
    rng = np.random.default_rng(seed)
    loci = [("AAAAG", "AAAAG" * 11, [("AAAAG" * 11, ("AAAAG", 11)), ("AAGGG" * 200, ("AAGGG", 200))]),
            ("CAG", "CAG" * 20, [("CAG" * 20, ("AGC", 20)), ("CCTG" * 120, ("CCTG", 120))]),
            ("ATTTT", "ATTTT" * 15, [("ATTTT" * 15, ("ATTTT", 15)),
                                     ("ATTTT" * 60 + "ATTTC" * 40 + "ATTTT" * 20, ("ATTTT", 80))]),
            ("TATTG", "TATTG" * 16, [("TATTG" * 12, ("ATTGT", 12)), ("TATTG" * 30, ("ATTGT", 30))])]
    gap, extra = 3000, 800
    parts, regions, at = [], [], 0
    for unit, ref_tract, _ in loci:
        left, right = rand_seq(rng, anchor_len + extra), rand_seq(rng, anchor_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(ref_tract), unit))
        parts += [rand_seq(rng, gap), left, ref_tract, right]
        at += gap + len(left) + len(ref_tract) + len(right)
    parts.append(rand_seq(rng, gap))
    chrom = "".join(parts)
    raw, truth = [], {}
    for g, ((_, _, alleles), (_, st, en, _)) in enumerate(zip(loci, regions)):
        for a, (tract, _) in enumerate(alleles):
            for i in range(reads_per_allele):
                lo, ro = anchor_len + int(rng.integers(0, 301)), anchor_len + int(rng.integers(0, 301))
                name = f"m{g}_{a}_{i:02d}"
                raw.append((name, chrom[st - lo:st] + tract + chrom[en:en + ro]))
                truth[name] = (g, a)
    seqs = apply_errors_batch(rng, [s for _, s in raw], model)
    reads = [(name, revcomp(s) if rng.random() < 0.5 else s) for (name, _), s in zip(raw, seqs)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads, truth=truth, planted=[[want for _, want in alleles] for _, _, alleles in loci])


def split_panel(reads_per_haplotype=8, anchor_len=1000, model="hifi", seed=6):
    """A small panel whose size alleles hold planted pairs of haplotypes of equal size, for the allele split
    (split.py): an HTT-like locus (BED CAG) with one size allele of two sequences, (CAG)20 CAA CAG beside (CAG)22, and a
    homogeneous (CAG)40; an FMR1-like one (BED CGG) with two AGG interruptions beside one in 30 units; an RFC1-like one
    (BED AAAAG) with (AAAAG)18 (AAGGG)4 (AAAAG)18 beside (AAAAG)40 (reads of pure (AAGGG)40 are not sized 40 in an AAAAG
    template, so the size phasing never puts them into one allele with (AAAAG)40); and a TATTG control with two homogeneous alleles (12 and 30 units).
    Every haplotype gets `reads_per_haplotype` reads that span both anchors, half reverse-complemented, through the
    `model` error channel.  Its own random stream; the default seed is one for which the contract's restatement puts
    every read of every pair on its planted haplotype (other seeds leave a read or two undecided or left out).

    Returns dict(ref, bed, regions, reads, truth) like panel() (truth = {name: (region, size allele)}), plus
    haplotype = {name: 0 / 1 within a planted pair, None in a homogeneous allele} and planted = [per region, per size
    allele in size order: (tract of haplotype 0, tract of 1) or None].
    """
    rng = np.random.default_rng(seed)
    fmr = "CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * 10
    loci = [("CAG", "CAG" * 22, [("CAG" * 20 + "CAACAG", "CAG" * 22), ("CAG" * 40,)]),
            ("CGG", "CGG" * 30, [(fmr, "CGG" * 9 + "AGG" + "CGG" * 20)]),
            ("AAAAG", "AAAAG" * 40, [("AAAAG" * 18 + "AAGGG" * 4 + "AAAAG" * 18, "AAAAG" * 40)]),
            ("TATTG", "TATTG" * 16, [("TATTG" * 12,), ("TATTG" * 30,)])]
    gap, extra = 3000, 800
    parts, regions, at = [], [], 0
    for unit, ref_tract, _ in loci:
        left, right = rand_seq(rng, anchor_len + extra), rand_seq(rng, anchor_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(ref_tract), unit))
        parts += [rand_seq(rng, gap), left, ref_tract, right]
        at += gap + len(left) + len(ref_tract) + len(right)
    parts.append(rand_seq(rng, gap))
    chrom = "".join(parts)
    raw, truth, haplotype = [], {}, {}
    for g, ((_, _, alleles), (_, st, en, _)) in enumerate(zip(loci, regions)):
        for a, tracts in enumerate(alleles):
            for h, tract in enumerate(tracts):
                for i in range(reads_per_haplotype):
                    lo, ro = anchor_len + int(rng.integers(0, 301)), anchor_len + int(rng.integers(0, 301))
                    name = f"h{g}_{a}_{h}_{i:02d}"
                    raw.append((name, chrom[st - lo:st] + tract + chrom[en:en + ro]))
                    truth[name] = (g, a)
                    haplotype[name] = h if len(tracts) == 2 else None
    seqs = apply_errors_batch(rng, [s for _, s in raw], model)
    reads = [(name, revcomp(s) if rng.random() < 0.5 else s) for (name, _), s in zip(raw, seqs)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads, truth=truth, haplotype=haplotype,
                planted=[[tr if len(tr) == 2 else None for tr in alleles] for _, _, alleles in loci])


def flank_panel(reads_per_haplotype=8, anchor_len=1000, flank_len=3000, flank_skip=20, model="hifi", seed=1):
    """A small panel whose haplotypes differ in the flanks of the repeat, for the flank haplotypes (flank.py).  Every
    region has at least `flank_len` + 800 reference bases on either side; haplotype 0 is the reference, haplotype 1
    carries substitutions in both flanks, one of them nearer to the repeat than `flank_skip` (never a site).  Regions:
    0 (BED CAG) two alleles of different size, 20 and 45 units, one per haplotype; 1 (TATTG) two alleles of equal size,
    16 units, on different haplotypes; 2 (CGG) a spanned allele of 18 units on haplotype 0 (half as many reads again, so
    that the spanned haplotype holds the most voted base of every site and the other one, none of whose rows covers both
    sides, is linked through the second) and an allele longer than every read on haplotype 1, whose reads hold one anchor
    only (`reads_per_haplotype` left-anchored and as many right-anchored, each with 120 to 200 units); 3 (AAAAG) a control with the same flanks on both haplotypes and two
    size alleles, 12 and 30 units; 4 (GGCCTG) 10 and 25 units, where every other read reaches only 200 to 500 bases into
    one flank.  Reads go through the `model` error channel, half reverse-complemented.  Its own random stream; the
    default seed is one for which the contract's restatement puts every read on its planted haplotype (DESIGN.md section
    25.3 counts the seeds that do).

    Returns dict(ref, bed, regions, reads, truth) like panel() (truth = {name: (region, units)}), plus haplotype =
    {name: 0 / 1, None in region 3}, kind = {name: "spanning" / "left" / "right"} and planted = [per region: (left
    offsets, right offsets) of haplotype 1's substitutions]."""
    rng = np.random.default_rng(seed)
    loci = [("CAG", 20, ((20, "spanning"), (45, "spanning")), True),
            ("TATTG", 16, ((16, "spanning"), (16, "spanning")), True),
            ("CGG", 20, ((18, "spanning"), (400, "one")), True),
            ("AAAAG", 15, ((12, "spanning"), (30, "spanning")), False),
            ("GGCCTG", 10, ((10, "spanning"), (25, "spanning")), True)]
    offsets = ((flank_skip // 4, 150, 420, 900, 1700, 2500), (flank_skip // 2, 90, 300, 800, 1400, 2200))
    gap, extra = 1000, 800
    parts, regions, at = [], [], 0
    for unit, kref, _, _ in loci:
        left, right = rand_seq(rng, flank_len + extra), rand_seq(rng, flank_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(unit) * kref, unit))
        parts += [rand_seq(rng, gap), left, unit * kref, right]
        at += gap + len(left) + len(unit) * kref + len(right)
    parts.append(rand_seq(rng, gap))
    chrom = "".join(parts)

    def sub(seq, at):
        return seq[:at] + "ACGT"[("ACGT".index(seq[at]) + 1 + at % 3) % 4] + seq[at + 1:]

    raw, truth, haplotype, kind, planted = [], {}, {}, {}, []
    reach = flank_len + 300
    for g, ((unit, _, alleles, differ), (_, st, en, _)) in enumerate(zip(loci, regions)):
        offs = tuple(tuple(o for o in side if o < flank_len) for side in offsets) if differ else ((), ())
        planted.append(offs)
        for h, (k, how) in enumerate(alleles):
            left, right = chrom[st - reach:st], chrom[en:en + reach]
            if h == 1:
                for o in offs[0]:
                    left = sub(left, len(left) - 1 - o)
                for o in offs[1]:
                    right = sub(right, o)
            n_reads = 2 * reads_per_haplotype if how == "one" else reads_per_haplotype * 3 // 2 if g == 2 else \
                reads_per_haplotype
            for i in range(n_reads):
                lo, ro = (int(rng.integers(anchor_len, reach + 1)) for _ in range(2))
                if g == 4 and i % 2:
                    short = int(rng.integers(200, 501))
                    lo, ro = (short, ro) if i % 4 == 1 else (lo, short)
                what = "spanning" if how == "spanning" else ("left", "right")[i % 2]
                name = f"f{g}_{h}_{what}_{i:02d}"
                shown = k if how == "spanning" else int(rng.integers(120, 201))
                if what == "spanning":
                    seq = left[len(left) - lo:] + unit * k + right[:ro]
                elif what == "left":
                    seq = left[len(left) - lo:] + unit * shown
                else:
                    seq = unit * shown + right[:ro]
                raw.append((name, seq))
                truth[name] = (g, k)
                haplotype[name] = h if differ else None
                kind[name] = what
    seqs = apply_errors_batch(rng, [s for _, s in raw], model)
    reads = [(name, revcomp(s) if rng.random() < 0.5 else s) for (name, _), s in zip(raw, seqs)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads, truth=truth, haplotype=haplotype, kind=kind, planted=planted)


def primitive_unit(rng, m):
    """A random unit of m bases that is no power of a shorter word."""
    while True:
        u = rand_unit(rng, m)
        if not any(m % d == 0 and u[:d] * (m // d) == u for d in range(1, m)):
            return u


def period_panel(reads_per_allele=8, anchor_len=1000, model="hifi", seed=SEED):
    """A small panel of long-unit loci, for the tandem periods (periods.py): a CSTB-like dodecamer (BED CCCCGCCCCGCG; 4
    and 14 copies), a 30-mer and a 60-mer locus with seeded primitive units (6 and 14, 5 and 11 copies), a locus whose
    BED motif is wrong (BED and reference hold the 30-mer; one allele carries 7 copies of it, the other 15 copies of
    another seeded 30-mer), the TATTG (12 and 30 units) and CAG (15 and 40) controls, and one region whose "tract" is
    200 bases of sequence without a period (BED ACTGG; one allele).  Reads span both anchors, half reverse-complemented,
    through the `model` error channel.  Its own random stream.

    Returns dict(ref, bed, regions, reads, truth) like panel(), plus planted = [per region, per allele in the order
    above: (unit or None, copies)].
    """
    rng = np.random.default_rng(seed)
    cstb = "CCCCGCCCCGCG"
    u30, u60, v30 = primitive_unit(rng, 30), primitive_unit(rng, 60), primitive_unit(rng, 30)
    plain = rand_seq(rng, 200)
    loci = [(cstb, cstb * 3, [(cstb, 4), (cstb, 14)]),
            (u30, u30 * 8, [(u30, 6), (u30, 14)]),
            (u60, u60 * 6, [(u60, 5), (u60, 11)]),
            (u30, u30 * 8, [(u30, 7), (v30, 15)]),
            ("TATTG", "TATTG" * 16, [("TATTG", 12), ("TATTG", 30)]),
            ("CAG", "CAG" * 20, [("CAG", 15), ("CAG", 40)]),
            ("ACTGG", plain, [(None, 0)])]
    gap, extra = 3000, 800
    parts, regions, at = [], [], 0
    for unit, ref_tract, _ in loci:
        left, right = rand_seq(rng, anchor_len + extra), rand_seq(rng, anchor_len + extra)
        start = at + gap + len(left)
        regions.append(("chr1", start, start + len(ref_tract), unit))
        parts += [rand_seq(rng, gap), left, ref_tract, right]
        at += gap + len(left) + len(ref_tract) + len(right)
    parts.append(rand_seq(rng, gap))
    chrom = "".join(parts)
    raw, truth = [], {}
    for g, ((_, _, alleles), (_, st, en, _)) in enumerate(zip(loci, regions)):
        for a, (unit, copies) in enumerate(alleles):
            tract = plain if unit is None else unit * copies
            for i in range(reads_per_allele):
                lo, ro = anchor_len + int(rng.integers(0, 301)), anchor_len + int(rng.integers(0, 301))
                name = f"v{g}_{a}_{i:02d}"
                raw.append((name, chrom[st - lo:st] + tract + chrom[en:en + ro]))
                truth[name] = (g, a)
    seqs = apply_errors_batch(rng, [s for _, s in raw], model)
    reads = [(name, revcomp(s) if rng.random() < 0.5 else s) for (name, _), s in zip(raw, seqs)]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    return dict(ref={"chr1": chrom}, bed=[f"{c}\t{st}\t{en}\t{u}\n" for c, st, en, u in regions], regions=regions,
                reads=reads, truth=truth, planted=[list(alleles) for _, _, alleles in loci])
