"""Flank haplotypes (no counterpart in the reference): the size phasing groups reads by repeat size
alone, and the allele split tells two sequences of one size apart only when the tracts differ.  The flanks of the repeat
carry the haplotype whatever the tract does: every read that reaches an anchor shows the variants next to it.  One call
of nra_flank_phase piles the reads' flank segments up on the two reference flanks of every region, calls the columns
where the reads disagree systematically and sorts the reads on two haplotypes (the contract is
include/nanorepeat_amd.h).  That answers what the tract cannot: which haplotype an allele that no read spans belongs
to (its one-anchor reads carry a whole flank), whether two alleles of one size are two haplotypes, and whether the size
phasing agrees with a phasing that never looked at a size.  It is reported beside the size phasing and never replaces
it.

Everything is written from the repeat outward: the left side is chrom[start - flank_len : start] reversed, the right
side chrom[end : end + flank_len], both upper-cased and cut at the first base other than A, C, G, T.  A spanning read
gives its row two segments, a one-anchor read (when partial.partial_regions has run) one; in-repeat reads have no
flank.

`flank_regions` fills `region.flank_phase`; `write_flank_phase` writes `<region>.flank_phase.tsv`,
`write_flank_summary` `<out_prefix>.NanoRepeat_flank_phase.tsv`; `report_unspanned_haplotypes` prints one NOTICE per
region with a haplotype whose one-anchor reads show more than its spanning reads.
"""
import sys

import numpy as np

from . import consensus, upstream
from .split import SYMBOLS

HAP_NAMES = "ab"
MAX_SEGMENT_LEN = 200000


def flank_sides(chrom_seq, start, end, flank_len):
    """(left side, right side) of the region [start, end) of a chromosome, from the repeat outward."""
    start = max(0, start)
    left = chrom_seq[max(0, start - flank_len):start][::-1].upper()
    right = chrom_seq[end:end + flank_len].upper()
    return tuple(_acgt_prefix(s) for s in (left, right))


def _acgt_prefix(s):
    for i, ch in enumerate(s):
        if ch not in "ACGT":
            return s[:i]
    return s


def set_flank_sides(region, ref_fasta_dict, flank_len):
    from . import io as nr_io
    chrom = nr_io._lookup_chromosome(ref_fasta_dict, region.chrom)
    region.flank_sides = flank_sides(chrom, region.start_pos, region.end_pos, flank_len)


def cut_of(flank_len):
    """The most bases of a read taken for a side: room for a read's net deletions on the reference flank."""
    return flank_len - flank_len // 16


def spanning_segments(read, read_seq, cut):
    """(sL, sR) of a read with both anchors; none when the anchors lie on opposite strands."""
    left, right = read.left_anchor_paf, read.right_anchor_paf
    if left.strand != right.strand:
        return "", ""
    seq = read_seq.strip()
    oriented = upstream.rev_comp(seq) if read.strand == "-" else seq
    return oriented[max(0, left.qend - cut):left.qend][::-1], oriented[right.qstart:right.qstart + cut]


def one_anchor_segments(side, hit, read_seq, cut):
    seq = read_seq.strip()
    oriented = upstream.rev_comp(seq) if hit.strand == "-" else seq
    if side == "left":
        return oriented[max(0, hit.qend - cut):hit.qend][::-1], ""
    return "", oriented[hit.qstart:hit.qstart + cut]


class HaplotypeCounts:
    """One flank haplotype: its spanning reads and their median size, its one-anchor reads and the most units one of
    them shows, and whether that is more than every spanning read of this haplotype."""

    def __init__(self):
        self.spanning = self.partial = self.unspanned = 0
        self.median_size = self.max_min_repeat_size = None

    def fields(self):
        return [str(self.spanning), "-" if self.median_size is None else f"{self.median_size:.1f}", str(self.partial),
                "-" if self.max_min_repeat_size is None else str(self.max_min_repeat_size), str(self.unspanned)]


class FlankPhase:
    """One region: the verdict, the sites, every read's label, symbols, distances and ends, the table size allele x
    haplotype and the two haplotypes' counts."""

    def __init__(self, names, kinds, flank_len, t_left):
        self.read_names, self.kinds, self.flank_len, self.t_left = names, kinds, flank_len, t_left
        self.phased = self.n0 = self.n1 = self.undecided = self.left_out = 0
        self.n_sites = self.n_supported = self.iterations = 0
        self.sites = np.zeros((0, 12), np.int32)
        self.labels = np.full(len(names), -1, np.int32)
        self.dist = np.full((len(names), 2), -2, np.int32)
        self.end = np.zeros((len(names), 2), np.int32)
        self.site_sym = np.zeros((0, len(names)), np.uint8)
        self.allele_by_haplotype = []          # [(allele id, reads on a, reads on b)]
        self.haplotypes = [HaplotypeCounts(), HaplotypeCounts()]

    def haplotype_of(self, i):
        """`a` / `b` for a read on a haplotype, `-` for an undecided one, `.` for one without an aligned side."""
        l = int(self.labels[i])
        return HAP_NAMES[l] if l in (0, 1) else "-" if l == 2 else "."

    def symbols_of(self, i):
        return "".join(SYMBOLS[c] for c in self.site_sym[:, i]) or "-"

    def site_names(self):
        """L<offset>:X/Y or R<offset>:X/Y per site, X the base of haplotype a."""
        out = []
        for s in self.sites:
            col = int(s[0])
            side, o = ("L", col) if col < self.t_left else ("R", col - self.t_left)
            out.append(f"{side}{o}:{'ACGT'[s[1]]}/{'ACGT'[s[2]]}")
        return out


def flank_regions(repeat_regions, reads_by_region, flank_len=3000, device=0, engine=None, **thresholds):
    """The flank haplotypes of every region in one call of `engine` (default _capi.flank_phase; tests pass a restatement
    with the same signature; `thresholds` are its keywords).  Every region needs `region.flank_sides`
    (set_flank_sides).  Rows: every read of `region.read_dict` with a round-3 size, then every read of
    `region.partial_reads` where partial.partial_regions has run.  Sets `region.flank_phase` = FlankPhase and returns the
    regions."""
    if engine is None:
        from . import _capi
        engine = _capi.flank_phase
    cut = cut_of(flank_len)
    groups, backbones, owners = [], [], []
    for region, reads in zip(repeat_regions, reads_by_region):
        names, kinds, rows = [], [], []
        for name, read in region.read_dict.items():
            if read.round3_repeat_size is None or name not in reads:
                continue
            names.append(name)
            kinds.append("spanning")
            rows.append(spanning_segments(read, reads[name], cut))
        one = getattr(region, "one_anchor_reads", None) or {}
        for name in getattr(region, "partial_reads", None) or {}:
            if name in one and name in reads:
                side, hit = one[name]
                names.append(name)
                kinds.append(side)
                rows.append(one_anchor_segments(side, hit, reads[name], cut))
        rows = [tuple(s.upper() if len(s) <= MAX_SEGMENT_LEN else "" for s in row) for row in rows]
        fp = FlankPhase(names, kinds, flank_len, len(region.flank_sides[0]))
        region.flank_phase = fp
        groups.append(rows)
        backbones.append(region.flank_sides)
        owners.append((region, fp))
    if not groups:
        return repeat_regions
    out = engine(groups, backbones, device=device, **thresholds)
    for g, (region, fp) in enumerate(owners):
        for k in ("phased", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations"):
            setattr(fp, k, int(out[k][g]))
        m = len(fp.read_names)
        fp.sites = np.asarray(out["sites"][g], np.int32).reshape(-1, 12)
        fp.labels = np.asarray(out["label"][g], np.int32)
        fp.dist = np.asarray(out["dist"][g], np.int32).reshape(m, 2)
        fp.end = np.asarray(out["end"][g], np.int32).reshape(m, 2)
        fp.site_sym = np.asarray(out["site_sym"][g], np.uint8).reshape(fp.n_sites, m)
        _count_haplotypes(region, fp)
    return repeat_regions


def _count_haplotypes(region, fp):
    label = {n: int(l) for n, l in zip(fp.read_names, fp.labels)}
    fp.allele_by_haplotype = [(allele, sum(label.get(n) == 0 for n, _ in named), sum(label.get(n) == 1 for n, _ in named))
                              for allele, named in consensus.named_allele_groups(region)]
    partial = getattr(region, "partial_reads", None) or {}
    for h, hc in enumerate(fp.haplotypes):
        sizes, shown = [], []
        for name, kind in zip(fp.read_names, fp.kinds):
            if label[name] != h:
                continue
            if kind == "spanning":
                sizes.append(float(region.read_dict[name].round3_repeat_size))
            else:
                hc.partial += 1
                if partial[name].min_repeat_size is not None:
                    shown.append(int(partial[name].min_repeat_size))
        hc.spanning = len(sizes)
        hc.median_size = float(np.median(sizes)) if sizes else None
        hc.max_min_repeat_size = max(shown) if shown else None
        hc.unspanned = int(bool(shown) and (not sizes or max(shown) > max(sizes)))


def _allele_of(region):
    from . import phasing
    return {n: q.allele_id for n, q in phasing.results_of(region).quantified_read_dict.items()}


def flank_text(region):
    fp = region.flank_phase
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Flank_Len={fp.flank_len}\n",
             f"##Sites={','.join(fp.site_names()) or '-'}\n",
             "#Read_Name\tKind\tSize_Allele\tRepeat_Size\tMin_Repeat_Size\tHaplotype\tSite_Symbols\tLeft_Dist\tLeft_End\t"
             "Right_Dist\tRight_End\n"]
    allele = _allele_of(region)
    partial = getattr(region, "partial_reads", None) or {}
    for i, (name, kind) in enumerate(zip(fp.read_names, fp.kinds)):
        if kind == "spanning":
            a = allele.get(name, -1)
            size_allele, size, shown = (str(a) if a >= 1 else "."), f"{region.read_dict[name].round3_repeat_size:.1f}", "-"
        else:
            v = partial[name].min_repeat_size
            size_allele, size, shown = ".", "-", "-" if v is None else str(int(v))
        lines.append("\t".join([name, kind, size_allele, size, shown, fp.haplotype_of(i), fp.symbols_of(i),
                                str(fp.dist[i, 0]), str(fp.end[i, 0]), str(fp.dist[i, 1]), str(fp.end[i, 1])]) + "\n")
    return "".join(lines)


def write_flank_phase(region):
    """`<region out_prefix>.flank_phase.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix or getattr(region, "flank_phase", None) is None:
        return None
    path = f"{region.out_prefix}.flank_phase.tsv"
    with open(path, "w") as f:
        f.write(flank_text(region))
    return path


SUMMARY_HEADER = ("#Chrom\tStart\tEnd\tMotif\tPhased\tNum_Sites\tNum_Supported\tReads_a\tReads_b\tUndecided\tLeft_Out\t"
                  "Allele_By_Haplotype\t" +
                  "\t".join(f"{k}_{h}" for h in HAP_NAMES
                            for k in ("Spanning", "Median_Size", "Partial", "Max_Min_Repeat_Size", "Unspanned")) + "\n")


def flank_summary_row(region):
    start = max(0, region.start_pos)
    head = f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t"
    fp = getattr(region, "flank_phase", None)
    if fp is None:
        return head + "\t".join(["-"] * 18) + "\n"
    table = ",".join(f"{a}:{x}/{y}" for a, x, y in fp.allele_by_haplotype) or "-"
    cells = [fp.phased, fp.n_sites, fp.n_supported, fp.n0, fp.n1, fp.undecided, fp.left_out, table]
    return head + "\t".join([str(c) for c in cells] + [f for hc in fp.haplotypes for f in hc.fields()]) + "\n"


def write_flank_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_flank_phase.tsv`: one row per BED region, in BED order; a region without a call has `-`
    fields."""
    path = f"{out_prefix}.NanoRepeat_flank_phase.tsv"
    with open(path, "w") as f:
        f.write(SUMMARY_HEADER)
        f.write("".join(flank_summary_row(region) for region in regions))
    return path


def report_unspanned_haplotypes(repeat_regions, stream=None):
    """One NOTICE per region with a haplotype whose one-anchor reads show more repeat units than every spanning read of
    that haplotype (or that has none).  Returns the number of such haplotypes."""
    stream = stream or sys.stderr
    total = 0
    for region in repeat_regions:
        fp = getattr(region, "flank_phase", None)
        said = []
        for h, hc in enumerate(fp.haplotypes if fp is not None else ()):
            if hc.unspanned:
                has = "no spanning read" if not hc.spanning else f"{hc.spanning} spanning read(s) of median size " \
                                                                 f"{hc.median_size:.1f}"
                said.append(f"haplotype {HAP_NAMES[h]} has {has} and {hc.partial} one-anchor read(s) that show at least "
                            f"{hc.max_min_repeat_size} repeat units")
        if said:
            total += len(said)
            print(f"NOTICE: {region.to_unique_id()}: flank {'; '.join(said)}"
                  f"{'' if fp.phased else ' (the flanks do not phase: the haplotypes are tentative)'}", file=stream)
    return total
