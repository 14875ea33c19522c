"""Consensus sequence of the repeat tract per allele (no counterpart in the reference): after
phasing, the tracts (structure.tract_of) of the reads of every allele of every region form one group each, and one
call of nra_tract_consensus returns every group's consensus: rounds of banded alignment to a backbone, column votes and
a new backbone, in integer arithmetic (the contract is include/nanorepeat_amd.h).  The consensuses then go through
nra_read_structure in one call, and structure.derive_units describes each one in its region's motif.

`consensus_regions` fills `region.allele_consensus`; `write_allele_consensus` and `write_consensus_summary` write
`<region>.allele_consensus.fasta` and `<out_prefix>.NanoRepeat_consensus.tsv`; `report_unsettled_alleles` counts the
alleles that did not converge or left reads out.
"""
import numpy as np

from . import phasing, structure

MAX_TRACT_LEN = 200000


class AlleleConsensus:
    """One allele's consensus and the structure fields of that sequence (None where the motif cannot be aligned)."""

    def __init__(self, allele_id, n_reads):
        self.allele_id = allele_id
        self.n_reads = n_reads                # reads of the allele with a tract
        self.sequence = ""
        self.support = np.zeros(0, np.int32)
        self.n_rounds = self.converged = self.voted = self.left_out = 0
        self.purity = self.pure_units = self.longest_pure_run = None
        self.interruptions = []

    def units(self, p):
        return len(self.sequence) / p

    def min_support(self):
        """The weakest base's share of the reads that voted (None without a consensus)."""
        if not len(self.sequence) or not self.voted:
            return None
        return int(self.support.min()) / self.voted


def named_allele_groups(region):
    """[(allele id, [(read name, tract) of each read of the allele, phased_reads.txt order, empty tracts dropped])] in
    phasing order."""
    res = phasing.results_of(region)
    ordered = structure._ordered_reads(region)
    out = []
    for label in range(1, len(res.quantified_allele_list) + 1):
        tracts = [(name, structure.tract_of(region, name).upper()) for name, allele in ordered if allele == str(label)]
        out.append((label, [(n, t) for n, t in tracts if 0 < len(t) <= MAX_TRACT_LEN]))
    return out


def allele_groups(region):
    """named_allele_groups without the names: [(allele id, [tract])]."""
    return [(label, [t for _, t in tracts]) for label, tracts in named_allele_groups(region)]


def consensus_regions(repeat_regions, device=0, engine=None, structure_engine=None, max_dist=None, max_rounds=8):
    """The consensus of every allele of every region, in one call of `engine` (default _capi.tract_consensus; tests
    pass a restatement with the same signature), then the structure of all consensuses in one call of
    `structure_engine` (default _capi.read_structure).  Regions whose motif is longer than 64 bases or not ACGT keep
    None in the structure fields.  Sets `region.allele_consensus` = [AlleleConsensus] and returns the regions."""
    from . import _capi
    if engine is None:
        engine = _capi.tract_consensus
    if structure_engine is None:
        structure_engine = _capi.read_structure
    groups, owners = [], []
    for region in repeat_regions:
        region.allele_consensus = []
        for label, tracts in allele_groups(region):
            ac = AlleleConsensus(label, len(tracts))
            region.allele_consensus.append(ac)
            groups.append(tracts)
            owners.append((region, ac))
    if not groups:
        return repeat_regions
    kw = {} if max_dist is None else dict(max_dist=max_dist)
    out = engine(groups, max_rounds=max_rounds, device=device, **kw)
    fill_consensuses(owners, out)
    describe_consensuses(owners, structure_engine, device)
    return repeat_regions


def fill_consensuses(owners, out):
    """Result g of a tract_consensus call into the AlleleConsensus of owners[g] = (region, consensus)."""
    for g, (_, ac) in enumerate(owners):
        ac.sequence = out["consensus"][g]
        ac.support = np.asarray(out["support"][g], np.int32)
        ac.n_rounds, ac.converged = int(out["n_rounds"][g]), int(out["converged"][g])
        ac.voted, ac.left_out = int(out["voted"][g]), int(out["left_out"][g])


def describe_consensuses(owners, structure_engine, device=0):
    """The structure fields of every consensus of owners = [(region, consensus)] in the region's motif, in one call of
    `structure_engine` (none when no motif can be aligned)."""
    motifs, motif_of, seqs, seq_motif, described = [], {}, [], [], []
    for region, ac in owners:
        unit = region.repeat_unit_seq.upper()
        if structure.motif_supported(unit) and ac.sequence:
            if unit not in motif_of:
                motif_of[unit] = len(motifs)
                motifs.append(unit)
            seqs.append(ac.sequence)
            seq_motif.append(motif_of[unit])
            described.append((ac, len(unit)))
    if seqs:
        st = structure_engine(motifs, seqs, np.array(seq_motif, np.int32), device=device)
        off = st["path_off"]
        for i, (ac, p) in enumerate(described):
            ac.purity, ac.pure_units, ac.longest_pure_run, ac.interruptions = structure.derive_units(
                seqs[i], p, int(st["start_phase"][i]), st["path"][off[i]:off[i + 1]])


def fasta_records(consensuses, p):
    """FASTA text of AlleleConsensus objects in a motif of p bases."""
    lines = []
    for ac in consensuses:
        lines.append(f">allele{ac.allele_id} reads={ac.voted} left_out={ac.left_out} len={len(ac.sequence)} "
                     f"units={ac.units(p):.1f} rounds={ac.n_rounds} converged={ac.converged}\n")
        lines += [ac.sequence[i:i + 80] + "\n" for i in range(0, len(ac.sequence), 80)]
    return "".join(lines)


def consensus_fasta_text(region):
    return fasta_records(getattr(region, "allele_consensus", None) or [], len(region.repeat_unit_seq))


def write_allele_consensus(region):
    """`<region out_prefix>.allele_consensus.fasta` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.allele_consensus.fasta"
    with open(path, "w") as f:
        f.write(consensus_fasta_text(region))
    return path


def consensus_summary_row(region):
    p = len(region.repeat_unit_seq)
    cells = []
    for ac in getattr(region, "allele_consensus", None) or []:
        ms = ac.min_support()
        purity = "-" if ac.purity is None else f"{ac.purity:.4f}"
        inter = "-" if ac.purity is None else (",".join(f"{k}:{b}" for k, b in ac.interruptions) or "-")
        cells.append(f"{ac.allele_id}:{ac.voted}:{ac.left_out}:{len(ac.sequence)}:{ac.units(p):.1f}:"
                     f"{'-' if ms is None else format(ms, '.2f')}:{purity}:{inter}")
    start = max(0, region.start_pos)
    return (f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t{len(cells)}\t"
            f"{'|'.join(cells) or '-'}\n")


def write_consensus_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_consensus.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_consensus.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Consensus\n")
        f.write("".join(consensus_summary_row(region) for region in regions))
    return path


def report_unsettled_alleles(repeat_regions, stream=None):
    """One NOTICE for the command: the alleles whose consensus did not converge within the rounds, and those that left
    reads out of their last vote.  Returns (not converged, with reads left out)."""
    import sys
    stream = stream or sys.stderr
    alleles = [ac for region in repeat_regions for ac in getattr(region, "allele_consensus", None) or []]
    open_ = sum(1 for ac in alleles if ac.n_reads and not ac.converged)
    left = sum(1 for ac in alleles if ac.left_out)
    if open_ or left:
        print(f"NOTICE: allele consensus: {open_} of {len(alleles)} allele(s) did not converge, {left} left "
              f"{sum(ac.left_out for ac in alleles)} read(s) out of the last vote", file=stream)
    return open_, left
