"""Discovered loci placed on a reference genome.

loci.py says which discovered runs are one locus; this module says where on a reference that locus lies and how many
copies the reference has there.  The sides of every locus's representative (the flank_len bases before and behind its
run) are the queries of nra_place_*: the reference FASTA is streamed past their index contig by contig, chunk by chunk,
and never held whole.  The candidates of a side are clustered, a side with one outstanding cluster is unique, and every
unique side is aligned against the contig window of its cluster (nra_align_pairs) for the tract's boundary.  It writes
`<out_prefix>.discovered_loci_placed.tsv` and, for the placed loci, `<out_prefix>.discovered_loci.ref.bed`: a BED file
on the reference itself that pipeline.quantify_from_bam and quantify_from_reads take unchanged.  No counterpart in the
reference.
"""
import sys

from . import discover
from . import io as nr_io

K = 15                     # the defaults k, bin and min_votes: measured, DESIGN.md section 31.4
BIN = 64
MIN_VOTES = 24
MAX_OCC = 16
MAX_TARGET_OCC = 64        # stated, not measured: no genome to measure it on
FLANK_LEN = 1000           # the pseudo-reference's anchor (loci.ANCHOR)
MAX_REF_SPAN = 50000
MAX_SIDE = 2048            # NRA_PLACE_MAX_QUERY
OCC_CEILING = 1024         # NRA_PLACE_OCC_CEILING
RUNNER_UP = 1.5            # the anchor rule's runner-up factor (upstream.py)
CHUNK_BASES = 1 << 24

PLACED_COLUMNS = ("Locus", "Class", "Unit", "Type", "Status", "Chrom", "Strand", "Ref_Start", "Ref_End", "Ref_Span",
                  "Ref_Copies", "Median_Copies", "Max_Copies", "Left_Votes", "Left_Second", "Right_Votes", "Right_Second",
                  "Catalogued")
STATUSES = ("placed", "left_only", "right_only", "discordant", "ambiguous", "unplaced")
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def check_options(k=K, bin=BIN, min_votes=None, max_occ=MAX_OCC, max_target_occ=MAX_TARGET_OCC, flank_len=FLANK_LEN,
                  max_ref_span=MAX_REF_SPAN):
    """ValueError for a value the placement cannot take; returns min_votes (the default for None)."""
    if min_votes is None:
        min_votes = MIN_VOTES
    if not isinstance(k, int) or k % 2 == 0 or not 11 <= k <= 15:
        raise ValueError(f"place_k must be odd and in 11..15, not {k!r}")
    if not isinstance(bin, int) or not 1 <= bin <= 4096:
        raise ValueError(f"place_bin must be in 1..4096, not {bin!r}")
    if not isinstance(min_votes, int) or min_votes < 1:
        raise ValueError(f"place_min_votes must be at least 1, not {min_votes!r}")
    if not isinstance(max_occ, int) or not 1 <= max_occ <= 255:
        raise ValueError(f"place_max_occ must be in 1..255, not {max_occ!r}")
    if not isinstance(max_target_occ, int) or not 1 <= max_target_occ <= OCC_CEILING:
        raise ValueError(f"place_max_target_occ must be in 1..{OCC_CEILING}, not {max_target_occ!r}")
    if not isinstance(flank_len, int) or not k <= flank_len <= MAX_SIDE:
        raise ValueError(f"place_flank_len must be in place_k..{MAX_SIDE}, not {flank_len!r}")
    if not isinstance(max_ref_span, int) or max_ref_span < 0:
        raise ValueError(f"max_ref_span must be at least 0, not {max_ref_span!r}")
    return min_votes


def locus_sides(rows, grouped, reads, flank_len=FLANK_LEN, k=K):
    """The queries: for every locus, in the order of the grouping, the representative's read[max(0, start - flank_len):
    start] as its side L and read[end:end + flank_len] as its side R; a side of fewer than k bases does not exist.
    reads: {read_index: (name, sequence)}.  Returns (sequences, [(locus id, 'L' | 'R')])."""
    seqs, owner = [], []
    for locus in grouped["loci"]:
        rep = rows[locus["rep"]]
        seq = reads[rep["read_index"]][1]
        for kind, side in (("L", seq[max(0, rep["start"] - flank_len):rep["start"]]),
                           ("R", seq[rep["end"]:rep["end"] + flank_len])):
            if len(side) >= k:
                seqs.append(side)
                owner.append((locus["id"], kind))
    return seqs, owner


def iter_reference(path, chunk_bases=CHUNK_BASES, k=K):
    """The contigs of a FASTA file (gzip-aware) as (contig ordinal, name, pos0, bases): chunks of chunk_bases bases,
    successive chunks of a contig overlapping by k - 1 bases, so that every k-window of a contig lies wholly inside
    exactly one chunk.  A contig is never held whole."""
    if chunk_bases < k:
        raise ValueError(f"chunk_bases must be at least k = {k}")
    t, name, parts, size, pos0 = -1, None, [], 0, 0
    with nr_io.gzopen(path) as fp:
        for line in fp:
            line = line.strip()
            if not line:
                continue
            if line[0] == ">":
                if name is not None and (size > k - 1 or pos0 == 0):
                    yield t, name, pos0, "".join(parts)
                t, name, parts, size, pos0 = t + 1, line[1:].split()[0], [], 0, 0
                continue
            if name is None:
                raise ValueError(f"{path}: sequence before the first FASTA header")
            parts.append(line)
            size += len(line)
            while size >= chunk_bases:
                buf = "".join(parts)
                yield t, name, pos0, buf[:chunk_bases]
                step = chunk_bases - (k - 1)
                parts, size, pos0 = [buf[step:]], len(buf) - step, pos0 + step
        if name is not None and (size > k - 1 or pos0 == 0):
            yield t, name, pos0, "".join(parts)


def fetch_windows(path, wanted):
    """{(name, lo, hi): bases [lo, hi) of contig `name`, upper-cased} for the windows `wanted`: one more pass over the
    FASTA file, keeping only the lines that overlap a window."""
    by_name, got = {}, {w: [] for w in wanted}
    for w in wanted:
        by_name.setdefault(w[0], []).append(w)
    mine, at = (), 0
    with nr_io.gzopen(path) as fp:
        for line in fp:
            line = line.strip()
            if not line:
                continue
            if line[0] == ">":
                mine, at = by_name.get(line[1:].split()[0], ()), 0
                continue
            for w in mine:
                lo, hi = max(w[1], at), min(w[2], at + len(line))
                if lo < hi:
                    got[w].append(line[lo - at:hi - at])
            at += len(line)
    return {w: "".join(parts).upper() for w, parts in got.items()}


def side_clusters(cands, n_queries):
    """Per query the clusters of its candidates: the candidates of one (contig, strand) in adjacent bins are one cluster
    (contig, strand, first bin, last bin, the largest votes among them); the clusters by votes, descending, the earlier
    (contig, strand, bin) first on a tie.  cands: dict(query, contig, strand, bin, votes) ordered by the first four."""
    cols = [cands[key].tolist() if hasattr(cands[key], "tolist") else list(cands[key])
            for key in ("query", "contig", "strand", "bin", "votes")]
    out = [[] for _ in range(n_queries)]
    last = None
    for q, t, s, b, v in zip(*cols):
        if last == (q, t, s, b - 1):
            c = out[q][-1]
            c[3], c[4] = b, max(c[4], v)
        else:
            out[q].append([t, s, b, b, v])
        last = (q, t, s, b)
    return [sorted(clusters, key=lambda c: -c[4]) for clusters in out]


def unique_side(clusters, min_votes):
    """(best votes, second votes, the best cluster when the side is unique, else None)."""
    best = clusters[0][4] if clusters else 0
    second = clusters[1][4] if len(clusters) > 1 else 0
    return best, second, clusters[0] if best >= min_votes and best > RUNNER_UP * second else None


def scan_reference(ref_fasta, queries, k, max_occ, bin, max_target_occ, min_votes, device=0, chunk_bases=CHUNK_BASES,
                   engine=None):
    """The reference streamed past the index of the queries.  `engine`: a stand-in for _capi with place_create,
    place_scan, place_candidates, place_stats and place_destroy.  The candidates are asked for down to two thirds of
    min_votes: a smaller runner-up cannot make a side with min_votes votes ambiguous.  Returns (candidates, [contig
    names], {name: length}, stats)."""
    if engine is None:
        from . import _capi
        engine = _capi
    names, lengths = [], {}
    h = engine.place_create(queries, k, max_occ, device)
    try:
        for t, name, pos0, bases in iter_reference(ref_fasta, chunk_bases, k):
            if t == len(names):
                if name in lengths:
                    raise ValueError(f"duplicate sequence name in {ref_fasta}: {name}")
                names.append(name)
            lengths[name] = pos0 + len(bases)
            engine.place_scan(h, t, pos0, bases)
        cands = engine.place_candidates(h, bin, max_target_occ, max(1, (2 * min_votes) // 3))
        stats = engine.place_stats(h)
    finally:
        engine.place_destroy(h)
    return cands, names, lengths, stats


def _bare(chrom):
    return chrom[3:] if chrom.startswith("chr") else chrom


def catalogued(regions, chrom, lo, hi):
    """The BED rows on `chrom` (either naming convention) that overlap [lo, hi)."""
    return sum(1 for r in regions if _bare(r.chrom) == _bare(chrom) and r.start_pos < hi and r.end_pos > lo)


def place_sides(queries, owner, cands, names, lengths, ref_fasta, bin, min_votes, aligner=None, device=0):
    """The side rule and the refinement.  Returns {(locus id, 'L' | 'R'): dict(votes, second, and for a unique side chrom,
    strand, edge)}: edge is the tract's boundary on the contig, the end of the side's alignment that faces the tract."""
    if aligner is None:
        from . import _capi
        aligner = _capi.align_pairs
    sides, jobs = {}, []
    for q, clusters in enumerate(side_clusters(cands, len(queries))):
        best, second, hit = unique_side(clusters, min_votes)
        sides[owner[q]] = dict(votes=best, second=second)
        if hit is not None:
            t, s, b_lo, b_hi, _ = hit
            lo = max(0, (b_lo - 2) * bin)
            hi = min(lengths[names[t]], (b_hi + 2 + 2) * bin + len(queries[q]))
            if lo < hi:
                jobs.append((q, s, (names[t], lo, hi)))
    windows = fetch_windows(ref_fasta, {w for _, _, w in jobs})
    if jobs:
        seqs = []
        for q, s, w in jobs:
            side = queries[q].upper()
            seqs += [revcomp(side) if s else side, windows[w]]
        got = aligner(seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2)), device=device)
        for (q, s, w), score, tstart, tend in zip(jobs, *(got[key].tolist() for key in ("score", "tstart", "tend"))):
            if score < 0:
                continue                                   # no alignment above the aligner's floor: not a unique side
            # the tract lies behind a + strand L side and a - strand R side, before the other two
            behind = (owner[q][1] == "L") == (s == 0)
            sides[owner[q]].update(chrom=w[0], strand="-" if s else "+", edge=w[1] + (tend if behind else tstart))
    return sides


def locus_status(left, right, bin, min_votes, max_ref_span):
    """(status, chrom, strand, ref_start, ref_end) of a locus from its two sides (None: the side does not exist); the
    fields that are not known are None."""
    lu, ru = (side is not None and "edge" in side for side in (left, right))
    if lu and ru:
        start, end = (left["edge"], right["edge"]) if left["strand"] == "+" else (right["edge"], left["edge"])
        if (left["chrom"], left["strand"]) == (right["chrom"], right["strand"]) and -bin <= end - start <= max_ref_span:
            return "placed", left["chrom"], left["strand"], start, end
        return "discordant", None, None, None, None
    if lu or ru:
        side = left if lu else right
        first = (side["strand"] == "+") == lu               # the known boundary is the tract's start
        return ("left_only" if lu else "right_only", side["chrom"], side["strand"], side["edge"] if first else None,
                None if first else side["edge"])
    if any(side is not None and side["votes"] >= min_votes for side in (left, right)):
        return "ambiguous", None, None, None, None
    return "unplaced", None, None, None, None


def placed_rows(table, sides, bin=BIN, min_votes=MIN_VOTES, max_ref_span=MAX_REF_SPAN, regions=None):
    """One row (a dict keyed by PLACED_COLUMNS) per locus of the locus table with a side, in the table's order."""
    show = lambda x: "-" if x is None else x
    out = []
    for c in table:
        left, right = sides.get((c["Locus"], "L")), sides.get((c["Locus"], "R"))
        if left is None and right is None:
            continue
        status, chrom, strand, start, end = locus_status(left, right, bin, min_votes, max_ref_span)
        span = end - start if status == "placed" else None
        known = [x for x in (start, end) if x is not None]
        out.append({"Locus": c["Locus"], "Class": c["Class"], "Unit": c["Unit"], "Type": c["Type"], "Status": status,
                    "Chrom": show(chrom), "Strand": show(strand), "Ref_Start": show(start), "Ref_End": show(end),
                    "Ref_Span": show(span), "Ref_Copies": show(None if span is None else max(0, span) // len(c["Unit"])),
                    "Median_Copies": c["Median_Copies"], "Max_Copies": c["Max_Copies"],
                    "Left_Votes": show(left and left["votes"]), "Left_Second": show(left and left["second"]),
                    "Right_Votes": show(right and right["votes"]), "Right_Second": show(right and right["second"]),
                    "Catalogued": "-" if regions is None or not known else
                    catalogued(regions, chrom, min(known) - 2 * bin, max(known) + 2 * bin),
                    "Bed_Unit": bed_unit(c["Unit"], max(0, span or 0), strand)})
    return out


def bed_unit(unit, ref_span, strand):
    """The unit as the reference's + strand has it at the tract's start.  `unit` is the representative's read at the
    start of its run; for a - strand read that is the reverse complement of the reference's tract at its end, and the
    tract starts in that phase only when its span is a whole number of units: else the unit is rotated by the rest."""
    if strand != "-":
        return unit
    w = revcomp(unit)
    r = -ref_span % len(unit)
    return w[r:] + w[:r]


def write_placed(rows, path):
    with open(path, "w") as f:
        f.write("\t".join(PLACED_COLUMNS) + "\n")
        for c in rows:
            f.write("\t".join(str(c[col]) for col in PLACED_COLUMNS) + "\n")


def write_ref_bed(rows, path):
    """The placed loci as BED rows on the reference: chrom, start, end, the unit as the reference's + strand has it
    (bed_unit).  A
    negative span (the two flanks overlap on the reference by a few bases) is written as start = end."""
    with open(path, "w") as f:
        for c in rows:
            if c["Status"] == "placed":
                start = min(c["Ref_Start"], c["Ref_End"])
                f.write(f"{c['Chrom']}\t{start}\t{c['Ref_End']}\t{c['Bed_Unit']}\n")


def place_files(reads_path, out_prefix, rows, grouped, table, ref_fasta, repeat_region_bed=None, k=K, bin=BIN,
                min_votes=None, max_occ=MAX_OCC, max_target_occ=MAX_TARGET_OCC, flank_len=FLANK_LEN,
                max_ref_span=MAX_REF_SPAN, device=0, chunk_bases=CHUNK_BASES, engine=None, aligner=None, stream=None,
                reads_chunk_bases=1 << 28):
    """rows, grouped, table: what loci.loci_files worked with and returned.  Places every locus's representative on
    ref_fasta -> `<out_prefix>.discovered_loci_placed.tsv`, `<out_prefix>.discovered_loci.ref.bed` and one NOTICE
    counting the statuses.  Returns the placed rows."""
    min_votes = check_options(k, bin, min_votes, max_occ, max_target_occ, flank_len, max_ref_span)
    reads = discover.fetch_reads(reads_path, {rows[l["rep"]]["read_index"] for l in grouped["loci"]}, reads_chunk_bases)
    queries, owner = locus_sides(rows, grouped, reads, flank_len, k)
    cands, names, lengths, _ = scan_reference(ref_fasta, queries, k, max_occ, bin, max_target_occ, min_votes, device,
                                              chunk_bases, engine)
    sides = place_sides(queries, owner, cands, names, lengths, ref_fasta, bin, min_votes, aligner, device)
    regions = nr_io.read_repeat_region_file(repeat_region_bed, True) if repeat_region_bed else None
    placed = placed_rows(table, sides, bin, min_votes, max_ref_span, regions)
    write_placed(placed, f"{out_prefix}.discovered_loci_placed.tsv")
    write_ref_bed(placed, f"{out_prefix}.discovered_loci.ref.bed")
    counts = ", ".join(f"{sum(c['Status'] == s for c in placed)} {s}" for s in STATUSES)
    print(f"NOTICE: of {len(placed)} locus/loci with a side to place on {ref_fasta}: {counts}", file=stream or sys.stderr)
    return placed
