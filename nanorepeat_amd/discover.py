"""Tandem-repeat runs of every read of a file, with no catalogue: which reads carry a long run, of which motif class, where
and on which strand.

The scan (nra_scan_repeats) returns per read the islands of periodic k-windows of one class; this module streams a
FASTQ / FASTA / BAM file through it, names the classes, says how a run lies in its read and writes the two files
`<out_prefix>.discovered_runs.tsv` and `<out_prefix>.NanoRepeat_discovered.tsv`.  No counterpart in the reference.
"""
import statistics
import sys

from . import io as nr_io

MAX_ROOT = 6
N_CLASS_IDS = (4 ** (MAX_ROOT + 1) - 4) // 3       # 5460: one id per word of 1..6 bases
_COMP = str.maketrans("ACGT", "TGCA")

RUN_COLUMNS = ("Read_Name", "Read_Len", "Ref", "Ref_Start", "Start", "End", "Span", "Class", "Unit", "Strand", "Copies",
               "Windows", "Density", "Kind")
CLASS_COLUMNS = ("Class", "Period", "Reads", "Runs", "In_Repeat", "Left_Open", "Right_Open", "Spanned", "Max_Span",
                 "Max_Copies", "Median_Spanned_Copies", "Total_Bases", "Catalogued_Regions")
KINDS = ("in_repeat", "left_open", "right_open", "spanned")


def class_word(class_id):
    """The word of an id: ids 0..3 are the 1-mers, 4..19 the 2-mers, ... in base-4 order, A < C < G < T.  The ids the
    scan returns are those of canonical words."""
    if not 0 <= class_id < N_CLASS_IDS:
        raise ValueError(f"class id {class_id!r} outside 0..{N_CLASS_IDS - 1}")
    p = 1
    while class_id >= (4 ** (p + 1) - 4) // 3:
        p += 1
    value = class_id - (4 ** p - 4) // 3
    return "".join("ACGT"[(value >> (2 * (p - 1 - j))) & 3] for j in range(p))


def class_id(word):
    """The class id of a motif: of its primitive root, the smallest word among the root's rotations and those of its
    reverse complement, read as a base-4 number behind the (4^p - 4) / 3 shorter words.  ValueError for a word that is
    not ACGT or whose root is longer than 6 bases."""
    w = (word or "").upper()
    if not w or set(w) - set("ACGT"):
        raise ValueError(f"not an ACGT word: {word!r}")
    root = next(w[:p] for p in range(1, len(w) + 1) if len(w) % p == 0 and w[:p] * (len(w) // p) == w)
    if len(root) > MAX_ROOT:
        raise ValueError(f"the root of {word!r} is longer than {MAX_ROOT} bases")
    rc = root.translate(_COMP)[::-1]
    canon = min(x[i:] + x[:i] for x in (root, rc) for i in range(len(root)))
    value = 0
    for c in canon:
        value = value * 4 + "ACGT".index(c)
    return (4 ** len(root) - 4) // 3 + value


def run_kind(start, end, read_len, edge):
    left, right = start <= edge, end >= read_len - edge
    return KINDS[0] if left and right else KINDS[1] if left else KINDS[2] if right else KINDS[3]


def _bam_chunks(path, chunk_bases):
    """The primary records with a sequence of a BAM file as chunks of (names, seqs, refs): refs = (contig, start), or
    ('*', '*') for an unmapped record."""
    from . import bam as nr_bam
    bam = nr_bam.open_alignment_file(path)
    try:
        records = bam.records() if isinstance(bam, nr_bam.BamFile) else bam.fetch(until_eof=True)
        names, seqs, refs, size = [], [], [], 0
        for rec in records:
            if rec.flag & 0x900 or not rec.query_sequence:
                continue
            names.append(rec.query_name)
            seqs.append(rec.query_sequence)
            mapped = rec.reference_id is not None and rec.reference_id >= 0 and not rec.flag & 0x4
            refs.append((bam.references[rec.reference_id], rec.reference_start) if mapped else ("*", "*"))
            size += len(seqs[-1])
            if size >= chunk_bases:
                yield names, seqs, refs
                names, seqs, refs, size = [], [], [], 0
        if names:
            yield names, seqs, refs
    finally:
        bam.close()


def scan_reads(path, k=11, max_gap=100, min_span=200, chunk_bases=1 << 28, device=0, engine=None, flank_len=0):
    """Streams `path` (FASTQ or FASTA, gzip-aware; a path ending in .bam: the primary records with a sequence) through
    the scan, one call per chunk of about chunk_bases bases.  Returns the runs in file order, then by start: dicts with
    name, read_len, ref, ref_start ('-' for FASTQ / FASTA; the record's contig and start, or '*', for BAM), start, end,
    span, class_id, cls (the class's word), unit (read[start:start + p], upper-cased), strand, copies (span // p),
    windows, density (windows / (span - k + 1)) and kind (run_kind with edge = max_gap).  `engine`: a stand-in for
    _capi.scan_repeats(seqs, k, max_gap, min_span, device).  flank_len > 0 (loci.py): the rows also carry left_flank =
    read[start - flank_len:start] and right_flank = read[end:end + flank_len], cut at the read's ends, and read_index,
    the read's ordinal among the records the scan saw."""
    if engine is None:
        from . import _capi
        engine = _capi.scan_repeats
    if str(path).lower().endswith(".bam"):
        chunks = _bam_chunks(path, chunk_bases)
    else:
        chunks = ((names, seqs, None) for names, seqs, _ in nr_io.iter_reads(path, chunk_bases))
    rows, n_before = [], 0
    for names, seqs, refs in chunks:
        got = engine(seqs, k, max_gap, min_span, device)
        cols = [got[key] for key in ("read", "start", "end", "cls", "windows", "fwd_windows")]
        for r, start, end, cid, windows, fwd in zip(*(c.tolist() if hasattr(c, "tolist") else list(c) for c in cols)):
            word = class_word(cid)
            p, span, seq = len(word), end - start, seqs[r]
            ref, ref_start = refs[r] if refs is not None else ("-", "-")
            rows.append(dict(name=names[r], read_len=len(seq), ref=ref, ref_start=ref_start, start=start, end=end,
                             span=span, class_id=cid, cls=word, unit=seq[start:start + p].upper(),
                             strand="+" if 2 * fwd >= windows else "-", copies=span // p, windows=windows,
                             density=windows / (span - k + 1), kind=run_kind(start, end, len(seq), max_gap)))
            if flank_len > 0:
                rows[-1].update(left_flank=seq[max(0, start - flank_len):start], right_flank=seq[end:end + flank_len],
                                read_index=n_before + r)
        n_before += len(seqs)
    return rows


def catalogue_classes(repeat_region_bed):
    """{class id: number of BED rows whose motif has that class}; rows whose motif has no class are not counted."""
    counts = {}
    for region in nr_io.read_repeat_region_file(repeat_region_bed, True):
        try:
            cid = class_id(region.repeat_unit_seq)
        except ValueError:
            continue
        counts[cid] = counts.get(cid, 0) + 1
    return counts


def class_rows(rows, catalogue=None):
    """One summary row (a dict keyed by CLASS_COLUMNS) per class with a run, by Max_Span descending, then Class."""
    by_class = {}
    for row in rows:
        by_class.setdefault(row["class_id"], []).append(row)
    out = []
    for cid, mine in by_class.items():
        kinds = [sum(r["kind"] == kd for r in mine) for kd in KINDS]
        spanned = [r["copies"] for r in mine if r["kind"] == "spanned"]
        out.append({"Class": class_word(cid), "Period": len(class_word(cid)), "Reads": len({r["name"] for r in mine}),
                    "Runs": len(mine), "In_Repeat": kinds[0], "Left_Open": kinds[1], "Right_Open": kinds[2],
                    "Spanned": kinds[3], "Max_Span": max(r["span"] for r in mine),
                    "Max_Copies": max(r["copies"] for r in mine),
                    "Median_Spanned_Copies": f"{statistics.median(spanned):g}" if spanned else "-",
                    "Total_Bases": sum(r["span"] for r in mine),
                    "Catalogued_Regions": "-" if catalogue is None else catalogue.get(cid, 0)})
    out.sort(key=lambda c: (-c["Max_Span"], c["Class"]))
    return out


def write_runs(rows, path):
    with open(path, "w") as f:
        f.write("\t".join(RUN_COLUMNS) + "\n")
        for r in rows:
            f.write("\t".join(str(x) for x in (
                r["name"], r["read_len"], r["ref"], r["ref_start"], r["start"], r["end"], r["span"], r["cls"], r["unit"],
                r["strand"], r["copies"], r["windows"], f"{r['density']:.3f}", r["kind"])) + "\n")


def write_classes(classes, path):
    with open(path, "w") as f:
        f.write("\t".join(CLASS_COLUMNS) + "\n")
        for c in classes:
            f.write("\t".join(str(c[col]) for col in CLASS_COLUMNS) + "\n")


def fetch_reads(path, indices, chunk_bases=1 << 28):
    """{read_index: (name, sequence)} of the records scan_reads numbered `indices`: one more pass over the file."""
    wanted, out, n_before = set(indices), {}, 0
    if not wanted:
        return out
    if str(path).lower().endswith(".bam"):
        chunks = _bam_chunks(path, chunk_bases)
    else:
        chunks = nr_io.iter_reads(path, chunk_bases)
    for names, seqs, _ in chunks:
        for i in wanted.intersection(range(n_before, n_before + len(seqs))):
            out[i] = (names[i - n_before], seqs[i - n_before])
        n_before += len(seqs)
    return out


def discover_file(reads_path, out_prefix, repeat_region_bed=None, k=11, max_gap=100, min_span=200, no_details=False,
                  device=0, chunk_bases=1 << 28, engine=None, stream=None, group_loci=False, flank_len=500, sketch_k=13,
                  min_shared=None, min_locus_reads=3, sketch_engine=None, place_ref=None, place_options=None,
                  place_engine=None, place_aligner=None):
    """scan_reads of the file -> `<out_prefix>.discovered_runs.tsv` (not with no_details) and
    `<out_prefix>.NanoRepeat_discovered.tsv`, and one NOTICE counting the classes with runs and no BED region.  Returns
    the summary rows (class_rows).  group_loci=True (loci.py) also groups the runs into loci by
    their flanks and writes the four locus files; the two files above are what they are without it.  place_ref (a
    FASTA file; place.py) beside it places the loci on that reference and writes the two placement
    files; place_options are place.check_options' keywords."""
    if place_ref is not None:
        from . import place as nr_place
        if not group_loci:
            raise ValueError("placing loci on a reference needs group_loci=True")
        nr_place.check_options(**(place_options or {}))
    if group_loci:
        from . import loci as nr_loci
        min_shared = nr_loci.check_options(flank_len, sketch_k, min_shared, min_locus_reads)
    rows = scan_reads(reads_path, k, max_gap, min_span, chunk_bases, device, engine,
                      flank_len=flank_len if group_loci else 0)
    catalogue = catalogue_classes(repeat_region_bed) if repeat_region_bed else None
    classes = class_rows(rows, catalogue)
    if not no_details:
        write_runs(rows, f"{out_prefix}.discovered_runs.tsv")
    write_classes(classes, f"{out_prefix}.NanoRepeat_discovered.tsv")
    new = sum(1 for c in classes if c["Catalogued_Regions"] in ("-", 0))
    if new:
        print(f"NOTICE: {new} repeat class(es) have runs of at least {min_span} bases in the reads and no region in "
              f"the BED file", file=stream or sys.stderr)
    if group_loci:
        table, grouped = nr_loci.loci_files(reads_path, out_prefix, rows, catalogue, sketch_k, min_shared,
                                            min_locus_reads, no_details, device, chunk_bases, sketch_engine, stream)
        if place_ref is not None:
            nr_place.place_files(reads_path, out_prefix, rows, grouped, table, place_ref, repeat_region_bed,
                                 device=device, engine=place_engine, aligner=place_aligner, stream=stream,
                                 reads_chunk_bases=chunk_bases, **(place_options or {}))
    return classes
