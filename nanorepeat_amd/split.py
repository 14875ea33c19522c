"""Two haplotypes inside one size allele (no counterpart in the reference): phasing groups reads by
repeat size alone, so an allele may hold two sequences of equal size (HTT with and without its CAA interruption, FMR1
with one or two AGG, RFC1 AAGGG beside AAAAG).  For every allele of every region one call of nra_allele_split piles the
allele's tracts up on its consensus, calls the columns where the reads disagree systematically, and sorts the reads on
two haplotypes (the contract is include/nanorepeat_amd.h).  The alleles that split get a consensus and a structure per
sub-allele, by one more call of nra_tract_consensus and one of nra_read_structure, exactly as consensus.py describes
alleles.  The split is reported beside the size phasing and never replaces it.

`split_regions` fills `region.allele_split`; `write_allele_split` writes `<region>.allele_split.tsv` and
`<region>.allele_split.fasta`, `write_split_summary` `<out_prefix>.NanoRepeat_split.tsv`; `report_split_alleles` counts
the alleles split.
"""
import numpy as np

from . import consensus, structure

SYMBOLS = "ACGTN-."            # row symbols 0..5, and 6: the read has no row
SUB_NAMES = "ab"


class AlleleSplit:
    """One size allele: the verdict, its sites, every read's label and symbols, and, when it splits, the two
    sub-alleles as consensus.AlleleConsensus objects (allele_id `<id>a` is the larger one)."""

    def __init__(self, allele_id, names):
        self.allele_id = allele_id
        self.read_names = names
        self.split = self.n0 = self.n1 = self.undecided = self.left_out = 0
        self.n_sites = self.n_supported = self.iterations = 0
        self.sites = np.zeros((0, 12), np.int32)
        self.labels = np.zeros(len(names), np.int32)
        self.site_sym = np.zeros((0, len(names)), np.uint8)
        self.sub_alleles = []

    def sub_allele_of(self, i):
        """`a` / `b` for a read on a haplotype of an allele that splits, else `-`."""
        return SUB_NAMES[self.labels[i]] if self.split and self.labels[i] in (0, 1) else "-"

    def symbols_of(self, i):
        return "".join(SYMBOLS[c] for c in self.site_sym[:, i]) or "-"

    def supported_sites(self):
        """[(column, base of haplotype 0, base of 1)] of the supported sites."""
        return [(int(s[0]), "ACGT"[s[1]], "ACGT"[s[2]]) for s in self.sites if s[11]]


def split_regions(repeat_regions, device=0, engine=None, consensus_engine=None, structure_engine=None, **thresholds):
    """The split of every allele of every region in one call of `engine` (default _capi.allele_split; tests pass a
    restatement with the same signature; `thresholds` are its keywords).  The backbone of an allele is its consensus:
    `region.allele_consensus` where consensus.consensus_regions has run, else it runs here (no consensus file is written
    on that account).  The alleles that split then get their sub-alleles' consensuses in one call of `consensus_engine`
    and their structure in one of `structure_engine`.  Sets `region.allele_split` = [AlleleSplit] and returns the
    regions."""
    from . import _capi
    if engine is None:
        engine = _capi.allele_split
    if consensus_engine is None:
        consensus_engine = _capi.tract_consensus
    if structure_engine is None:
        structure_engine = _capi.read_structure
    todo = [r for r in repeat_regions if getattr(r, "allele_consensus", None) is None]
    if todo:
        consensus.consensus_regions(todo, device=device, engine=consensus_engine, structure_engine=structure_engine)
    groups, backbones, owners = [], [], []
    for region in repeat_regions:
        region.allele_split = []
        for (label, named), ac in zip(consensus.named_allele_groups(region), region.allele_consensus):
            sp = AlleleSplit(label, [n for n, _ in named])
            region.allele_split.append(sp)
            groups.append([t for _, t in named])
            backbones.append(ac.sequence)
            owners.append((region, sp))
    if not groups:
        return repeat_regions
    out = engine(groups, backbones, device=device, **thresholds)
    sub_groups, sub_owners = [], []
    for g, (region, sp) in enumerate(owners):
        for k in ("split", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations"):
            setattr(sp, k, int(out[k][g]))
        sp.sites = np.asarray(out["sites"][g], np.int32).reshape(-1, 12)
        sp.labels = np.asarray(out["label"][g], np.int32)
        sp.site_sym = np.asarray(out["site_sym"][g], np.uint8).reshape(sp.n_sites, len(sp.read_names))
        if sp.split:
            for h in (0, 1):
                tracts = [t for t, l in zip(groups[g], sp.labels) if l == h]
                sub = consensus.AlleleConsensus(f"{sp.allele_id}{SUB_NAMES[h]}", len(tracts))
                sp.sub_alleles.append(sub)
                sub_groups.append(tracts)
                sub_owners.append((region, sub))
    if sub_groups:
        consensus.fill_consensuses(sub_owners, consensus_engine(sub_groups, max_rounds=8, device=device))
        consensus.describe_consensuses(sub_owners, structure_engine, device)
    return repeat_regions


def split_text(region):
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "##Symbols=ACGT: base; N: other base; -: deleted; .: read left out\n"]
    for sp in getattr(region, "allele_split", None) or []:
        cols = ",".join(str(int(s[0])) for s in sp.sites) or "-"
        lines.append(f"##Allele={sp.allele_id} split={sp.split} site_columns={cols}\n")
    lines.append("#Read_Name\tAllele_ID\tSub_Allele\tSite_Symbols\n")
    for sp in getattr(region, "allele_split", None) or []:
        for i, name in enumerate(sp.read_names):
            lines.append(f"{name}\t{sp.allele_id}\t{sp.sub_allele_of(i)}\t{sp.symbols_of(i)}\n")
    return "".join(lines)


def split_fasta_text(region):
    subs = [sub for sp in getattr(region, "allele_split", None) or [] for sub in sp.sub_alleles]
    return consensus.fasta_records(subs, len(region.repeat_unit_seq))


def write_allele_split(region):
    """`<region out_prefix>.allele_split.tsv` and `.allele_split.fasta` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    paths = (f"{region.out_prefix}.allele_split.tsv", f"{region.out_prefix}.allele_split.fasta")
    for path, text in zip(paths, (split_text(region), split_fasta_text(region))):
        with open(path, "w") as f:
            f.write(text)
    return paths


def split_summary_row(region):
    cells = []
    for sp in getattr(region, "allele_split", None) or []:
        sites = ",".join(f"{c}:{x}/{y}" for c, x, y in sp.supported_sites()) or "-"
        cells.append(f"{sp.allele_id}:{sp.split}:{sp.n0}:{sp.n1}:{sp.undecided}:{sp.left_out}:{sp.n_sites}:{sites}")
    start = max(0, region.start_pos)
    return (f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t{len(cells)}\t"
            f"{'|'.join(cells) or '-'}\n")


def write_split_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_split.tsv`: one row per BED region, in BED order; per allele
    id:split:reads in a:in b:undecided:left out:sites:supported sites as column:base/base."""
    path = f"{out_prefix}.NanoRepeat_split.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Split\n")
        f.write("".join(split_summary_row(region) for region in regions))
    return path


def report_split_alleles(repeat_regions, stream=None):
    """One NOTICE for the command: how many alleles hold two sequences.  Returns (split, alleles)."""
    import sys
    stream = stream or sys.stderr
    alleles = [sp for region in repeat_regions for sp in getattr(region, "allele_split", None) or []]
    n = sum(sp.split for sp in alleles)
    print(f"NOTICE: allele split: {n} of {len(alleles)} allele(s) hold two sequences of one size.  With ONT reads of an "
          f"A/G-rich motif (such as AAGGG) a split may be false: indel errors shift bases across the A and G runs "
          f"(DESIGN.md section 19.3)", file=stream)
    return n, len(alleles)
