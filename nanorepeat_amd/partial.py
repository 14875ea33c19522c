"""One-anchor reads (no counterpart in the reference): a read that contains one anchor only
starts in one flank and ends inside the repeat.  It cannot be sized, but it shows how many repeat units follow its
anchor, and that number bounds from below the allele it came from.  When no read spans a long allele, these reads are
the only evidence that it exists.

`upstream.find_anchor_locations_for1read` keeps such reads on `region.one_anchor_reads` = {name: (side, AnchorHit)}.
For each, on the read oriented like the hit (`rev_comp` for `-`):

* left anchor:  tail = oriented[hit.qend:], motif u;
* right anchor: tail = oriented[:hit.qstart] reversed, motif u reversed

and the tail is extended along the motif from its anchored end (nra_extend_tracts, one call for all regions).
`Min_Repeat_Size = motif_bases // p` is what the read shows: a bound from one read, up to sequencing error, not an
allele call.  `Exceeds_Spanning` marks a read that shows more units than the largest round-3 size of the region's
spanning reads (strictly; every read with Min_Repeat_Size > 0 when the region has no spanning read).

In-repeat reads: a read without a hit of either anchor (`region.no_anchor_reads`, kept by upstream
when asked) may lie wholly inside the repeat.  It is extended four times with the same scores -- from its first base
along u, from its first base along revcomp(u), from its last base backwards along reversed u, from its last base
backwards along reversed revcomp(u) -- and the best score wins, the earliest of these on a tie.  `Repeat_Units =
motif_bases // p` is a lower bound like Min_Repeat_Size, and `Exceeds_Spanning` follows the same strict rule.
`in_repeat_regions` fills `region.in_repeat_reads`; `write_in_repeat_reads` and `write_in_repeat_summary` write
`<region>.in_repeat_reads.tsv` and `<out_prefix>.NanoRepeat_in_repeat.tsv`; `report_exceeding_in_repeat_reads` prints
one NOTICE per region with such reads.

`partial_regions` fills `region.partial_reads`; `write_partial_reads` and `write_partial_summary` write
`<region>.partial_reads.tsv` and `<out_prefix>.NanoRepeat_partial.tsv`; `report_exceeding_reads` prints one NOTICE
per region with such reads.
"""
import sys

import numpy as np

from . import upstream
from .structure import MAX_TRACT_LEN, motif_supported

DEFAULT_SCORES = (2, 4, 6)          # match, mismatch, gap_open1 + gap_ext1 of nra_default_scoring


class PartialRead:
    """One one-anchor read: its anchor, its tail, and the extension's outputs (None: the tail was not extended)."""

    def __init__(self, side, strand, tail_bases):
        self.side, self.strand, self.tail_bases = side, strand, tail_bases
        self.extended_bases = self.motif_bases = self.min_repeat_size = self.score = None
        self.exceeds_spanning = None

    def fields(self):
        vals = (self.extended_bases, self.motif_bases, self.min_repeat_size, self.score, self.exceeds_spanning)
        return [self.side, self.strand, str(self.tail_bases)] + ["-" if v is None else str(int(v)) for v in vals]


def extension_scores(scoring=None):
    """(match, mismatch, gap) of the extension for the scoring in use: a one-base gap costs gap_open1 + gap_ext1."""
    if scoring is None:
        return DEFAULT_SCORES
    return int(scoring.match), int(scoring.mismatch), int(scoring.gap_open1) + int(scoring.gap_ext1)


def tail_of(side, hit, read_seq):
    """The bases that follow the anchor, read away from it, on the read oriented like the hit."""
    seq = read_seq.strip()
    oriented = upstream.rev_comp(seq) if hit.strand == "-" else seq
    return oriented[hit.qend:] if side == "left" else oriented[:hit.qstart][::-1]


def max_spanning_size(region):
    """The largest round-3 size of the region's spanning reads, or None."""
    sizes = [r.round3_repeat_size for r in region.read_dict.values() if r.round3_repeat_size is not None]
    return max(sizes) if sizes else None


def partial_regions(repeat_regions, reads_by_region, device=0, scoring=None, engine=None):
    """The extension of every one-anchor read of every region, in one call of `engine` (default _capi.extend_tracts;
    tests pass a restatement with the same signature).  A region whose motif is longer than 64 bases or not ACGT,
    and a tail over 200 000 bases, are not extended: `-` fields.  Sets `region.partial_reads` =
    {read_name: PartialRead} and returns the regions."""
    if engine is None:
        from . import _capi
        engine = _capi.extend_tracts
    match, mismatch, gap = extension_scores(scoring)
    motifs, motif_of, tails, read_motif, owners = [], {}, [], [], []
    for region, reads in zip(repeat_regions, reads_by_region):
        region.partial_reads = {}
        unit = region.repeat_unit_seq.upper()
        ok = motif_supported(unit)
        for name, (side, hit) in (getattr(region, "one_anchor_reads", None) or {}).items():
            tail = tail_of(side, hit, reads[name])
            region.partial_reads[name] = PartialRead(side, hit.strand, len(tail))
            if ok and len(tail) <= MAX_TRACT_LEN:
                u = unit if side == "left" else unit[::-1]
                if u not in motif_of:
                    motif_of[u] = len(motifs)
                    motifs.append(u)
                tails.append(tail.upper())
                read_motif.append(motif_of[u])
                owners.append((region, name, len(unit)))
    if tails:
        out = engine(motifs, tails, np.array(read_motif, np.int32), match=match, mismatch=mismatch, gap=gap,
                     device=device)
        for i, (region, name, p) in enumerate(owners):
            pr = region.partial_reads[name]
            pr.score, pr.extended_bases = int(out["score"][i]), int(out["end"][i])
            pr.motif_bases = int(out["motif_bases"][i])
            pr.min_repeat_size = pr.motif_bases // p
    for region in repeat_regions:
        top = max_spanning_size(region)
        for pr in region.partial_reads.values():
            if pr.min_repeat_size is not None:
                pr.exceeds_spanning = int(pr.min_repeat_size > (0 if top is None else top))
    return repeat_regions


def _sorted_reads(region):
    """Min_Repeat_Size descending (reads without one last), then name."""
    pr = getattr(region, "partial_reads", None) or {}
    return sorted(pr, key=lambda n: (-(pr[n].min_repeat_size if pr[n].min_repeat_size is not None else -1), n))


def partial_reads_text(region):
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "#Read_Name\tAnchor\tStrand\tTail_Bases\tExtended_Bases\tMotif_Bases\tMin_Repeat_Size\tScore\t"
             "Exceeds_Spanning\n"]
    for name in _sorted_reads(region):
        lines.append("\t".join([name] + region.partial_reads[name].fields()) + "\n")
    return "".join(lines)


def write_partial_reads(region):
    """`<region out_prefix>.partial_reads.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.partial_reads.tsv"
    with open(path, "w") as f:
        f.write(partial_reads_text(region))
    return path


def region_counts(region):
    """(spanning reads, largest spanning size or None, left-anchored, right-anchored, largest Min_Repeat_Size or None,
    reads that exceed the spanning reads)."""
    pr = list((getattr(region, "partial_reads", None) or {}).values())
    spanning = sum(r.round3_repeat_size is not None for r in region.read_dict.values())
    shown = [r.min_repeat_size for r in pr if r.min_repeat_size is not None]
    return (spanning, max_spanning_size(region), sum(r.side == "left" for r in pr), sum(r.side == "right" for r in pr),
            max(shown) if shown else None, sum(bool(r.exceeds_spanning) for r in pr))


def partial_summary_row(region):
    spanning, top, n_left, n_right, shown, exceeding = region_counts(region)
    start = max(0, region.start_pos)
    return (f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t{spanning}\t"
            f"{'-' if top is None else f'{top:.1f}'}\t{n_left}\t{n_right}\t{'-' if shown is None else shown}\t"
            f"{exceeding}\n")


def write_partial_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_partial.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_partial.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Spanning\tMax_Spanning_Size\tNum_Partial_Left\tNum_Partial_Right\t"
                "Max_Min_Repeat_Size\tNum_Exceeding\n")
        f.write("".join(partial_summary_row(region) for region in regions))
    return path


def report_exceeding_reads(repeat_regions, stream=None):
    """One NOTICE per region where one-anchor reads show more repeat units than any spanning read: the sizes reported
    for that region may miss a longer allele.  Returns the number of such reads."""
    stream = stream or sys.stderr
    total = 0
    for region in repeat_regions:
        spanning, top, _, _, shown, exceeding = region_counts(region)
        if exceeding:
            total += exceeding
            than = "there is no spanning read" if top is None else f"the largest spanning read has {top:.1f}"
            print(f"NOTICE: {region.to_unique_id()}: {exceeding} one-anchor read(s) show up to {shown} repeat units; "
                  f"{than}: an allele longer than the reads' reach may be missing from the sizes", file=stream)
    return total


# ----------------------------------------------------------------------------------- in-repeat reads
IN_REPEAT_ATTEMPTS = (("+", "start"), ("-", "start"), ("+", "end"), ("-", "end"))


class InRepeatRead:
    """One read without an anchor: the winning extension's outputs (None: the read was not extended)."""

    def __init__(self, read_len):
        self.read_len = read_len
        self.strand = self.end = None
        self.extended_bases = self.motif_bases = self.repeat_units = self.score = self.exceeds_spanning = None

    def fields(self):
        vals = (self.extended_bases, self.motif_bases, self.repeat_units, self.score, self.exceeds_spanning)
        return [self.strand or "-", self.end or "-", str(self.read_len)] + \
            ["-" if v is None else str(int(v)) for v in vals]


def in_repeat_attempts(seq, unit):
    """The four (tract, motif) of one read, in IN_REPEAT_ATTEMPTS' order."""
    s, rc = seq.upper(), upstream.rev_comp(unit)
    return [(s, unit), (s, rc), (s[::-1], unit[::-1]), (s[::-1], rc[::-1])]


def in_repeat_regions(repeat_regions, reads_by_region, device=0, scoring=None, engine=None, keep=None):
    """The four extensions of every no-anchor read of every region, in one call of `engine` (default
    _capi.extend_tracts).  `keep(region, sequence)`: a read it refuses is no in-repeat read of that region (the FASTQ
    command passes the motif screen's count rule, so that the exhaustive form sees the reads the screen offers).  A
    region whose motif is longer than 64 bases or not ACGT, and a read over 200 000 bases, are not extended: `-`
    fields.  Sets `region.in_repeat_reads` = {read_name: InRepeatRead} and returns the regions."""
    if engine is None:
        from . import _capi
        engine = _capi.extend_tracts
    match, mismatch, gap = extension_scores(scoring)
    motifs, motif_of, tracts, read_motif, owners = [], {}, [], [], []
    for region, reads in zip(repeat_regions, reads_by_region):
        region.in_repeat_reads = {}
        unit = region.repeat_unit_seq.upper()
        ok = motif_supported(unit)
        for name in (getattr(region, "no_anchor_reads", None) or {}):
            seq = reads[name].strip()
            if keep is not None and not keep(region, seq):
                continue
            region.in_repeat_reads[name] = InRepeatRead(len(seq))
            if ok and len(seq) <= MAX_TRACT_LEN:
                for tract, u in in_repeat_attempts(seq, unit):
                    if u not in motif_of:
                        motif_of[u] = len(motifs)
                        motifs.append(u)
                    tracts.append(tract)
                    read_motif.append(motif_of[u])
                owners.append((region, name, len(unit)))
    if tracts:
        out = engine(motifs, tracts, np.array(read_motif, np.int32), match=match, mismatch=mismatch, gap=gap,
                     device=device)
        for i, (region, name, p) in enumerate(owners):
            scores = [int(out["score"][4 * i + a]) for a in range(4)]
            a = scores.index(max(scores))                        # the earliest attempt on a tie
            ir = region.in_repeat_reads[name]
            ir.strand, ir.end = IN_REPEAT_ATTEMPTS[a]
            ir.score, ir.extended_bases = scores[a], int(out["end"][4 * i + a])
            ir.motif_bases = int(out["motif_bases"][4 * i + a])
            ir.repeat_units = ir.motif_bases // p
    for region in repeat_regions:
        top = max_spanning_size(region)
        for ir in region.in_repeat_reads.values():
            if ir.repeat_units is not None:
                ir.exceeds_spanning = int(ir.repeat_units > (0 if top is None else top))
    return repeat_regions


def in_repeat_reads_text(region):
    ir = getattr(region, "in_repeat_reads", None) or {}
    order = sorted(ir, key=lambda n: (-(ir[n].repeat_units if ir[n].repeat_units is not None else -1), n))
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "#Read_Name\tStrand\tEnd\tRead_Len\tExtended_Bases\tMotif_Bases\tRepeat_Units\tScore\tExceeds_Spanning\n"]
    return "".join(lines + ["\t".join([name] + ir[name].fields()) + "\n" for name in order])


def write_in_repeat_reads(region):
    """`<region out_prefix>.in_repeat_reads.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.in_repeat_reads.tsv"
    with open(path, "w") as f:
        f.write(in_repeat_reads_text(region))
    return path


def in_repeat_counts(region):
    """(spanning reads, largest spanning size or None, in-repeat reads, largest Repeat_Units or None, reads that
    exceed the spanning reads)."""
    ir = list((getattr(region, "in_repeat_reads", None) or {}).values())
    spanning = sum(r.round3_repeat_size is not None for r in region.read_dict.values())
    shown = [r.repeat_units for r in ir if r.repeat_units is not None]
    return (spanning, max_spanning_size(region), len(ir), max(shown) if shown else None,
            sum(bool(r.exceeds_spanning) for r in ir))


def write_in_repeat_summary(regions, out_prefix, shared=None, unscreened=()):
    """`<out_prefix>.NanoRepeat_in_repeat.tsv`: one row per BED region, in BED order.  `shared[i]`: the number of BED
    regions of region i's motif class (the FASTQ command; `-` for the BAM command, whose reads the mapper chose);
    `unscreened`: the regions (by id) whose motif has no class, so that the FASTQ command cannot look for their
    in-repeat reads: `-` counts."""
    path = f"{out_prefix}.NanoRepeat_in_repeat.tsv"
    with open(path, "w") as f:
        f.write("##Shared_Motif_Regions: the BED regions whose motif is of this region's class (rotations, reverse "
                "complement).  An in-repeat read of a FASTQ / FASTA file holds no anchor and cannot be told apart among "
                "them: it is counted in each.\n")
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Spanning\tMax_Spanning_Size\tNum_In_Repeat\tMax_Repeat_Units\t"
                "Num_Exceeding\tShared_Motif_Regions\n")
        for i, region in enumerate(regions):
            spanning, top, n, shown, exceeding = in_repeat_counts(region)
            counts = ["-", "-", "-"] if id(region) in unscreened else \
                [str(n), "-" if shown is None else str(shown), str(exceeding)]
            f.write("\t".join([region.chrom, str(max(0, region.start_pos)), str(region.end_pos), region.repeat_unit_seq,
                               str(spanning), "-" if top is None else f"{top:.1f}"] + counts +
                              ["-" if shared is None else str(shared[i])]) + "\n")
    return path


def report_exceeding_in_repeat_reads(repeat_regions, stream=None):
    """One NOTICE per region where in-repeat reads show more repeat units than any spanning read.  Returns the number
    of such reads."""
    stream = stream or sys.stderr
    total = 0
    for region in repeat_regions:
        spanning, top, _, shown, exceeding = in_repeat_counts(region)
        if exceeding:
            total += exceeding
            than = "there is no spanning read" if top is None else f"the largest spanning read has {top:.1f}"
            print(f"NOTICE: {region.to_unique_id()}: {exceeding} in-repeat read(s) show up to {shown} repeat units; "
                  f"{than}: an allele longer than the reads' reach may be missing from the sizes", file=stream)
    return total
