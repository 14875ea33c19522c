"""Motif runs per read and per allele (no counterpart in the reference): a tract made of several
motifs -- (ATTTT)60 (ATTTC)40 (ATTTT)20, (AAAAG)n (AAGGG)m, (CAG)n ... (CCG)m (CCT)k -- is aligned against a *set* of
motifs, each repeated without end, with a price W for changing motif (nra_tract_segments; the contract is
include/nanorepeat_amd.h).  On the host the alignment is cut into runs: the maximal stretches of tract bases that one
motif consumed or inserted.

The motif set of a region: the BED motif first (a region whose BED motif is not ACGT or exceeds 32 bases is not
segmented); then `segment_motifs[region key]` when given; else the classes section 15 calls for the region (its
Motif_Groups classes and every allele's dominant and secondary classes, classes of period 1 left out unless the BED
motif is one), ordered by read support, then class, while the set stays within 8 motifs and 32 states.

One call segments the tracts of all reads with a core over all regions, a second one the allele consensuses (section
18).  `segments_regions` fills `region.motif_set`, `region.read_runs` and `region.allele_runs`; `write_read_runs`
writes `<region>.read_runs.tsv`, `write_runs_summary` `<out_prefix>.NanoRepeat_runs.tsv`; `report_multi_run_alleles`
counts the alleles whose consensus has more than one run.
"""
import numpy as np

from . import consensus, motifs as nr_motifs, phasing, structure

MATCH, MISMATCH, INSERTION = 0, 1, 2
MAX_MOTIFS = 8
MAX_STATES = 32
MAX_TRACT_LEN = 200000
MAX_SWITCH_COST = 1000
DEFAULT_SWITCH_COST = 2         # chosen from the table of DESIGN.md section 20.3


class Run:
    """One run: `motif` (index in the set), first tract base, tract bases, motif bases consumed, edits."""

    __slots__ = ("motif", "first", "bases", "consumed", "edits")

    def __init__(self, motif, first):
        self.motif, self.first = motif, first
        self.bases = self.consumed = self.edits = 0

    def as_tuple(self):
        return self.motif, self.first, self.bases, self.consumed, self.edits


def derive_runs(path, motif_of):
    """(path bytes, motif index per base) -> [Run]: the maximal stretches of tract bases with one motif index.  A match,
    a mismatch and every motif base deleted right after a base count as consumed; mismatches, insertions and deleted
    bases as edits."""
    runs = []
    for i in range(len(path)):
        b, m = int(path[i]), int(motif_of[i])
        if not runs or runs[-1].motif != m:
            runs.append(Run(m, i))
        r = runs[-1]
        op, nd = b & 3, b >> 2
        r.bases += 1
        r.consumed += nd + (op != INSERTION)
        r.edits += nd + (op != MATCH)
    return runs


def runs_text(runs, motif_set):
    """`(ATTTT)60.0(ATTTC)40.0(ATTTT)20.0` (`-` without a run)."""
    return "".join(f"({motif_set[r.motif]}){r.consumed / len(motif_set[r.motif]):.1f}" for r in runs) or "-"


def units_per_motif(runs, motif_set):
    """The units of every motif of the set over all of its runs, in set order."""
    total = [0] * len(motif_set)
    for r in runs:
        total[r.motif] += r.consumed
    return [t / len(u) for t, u in zip(total, motif_set)]


class TractRuns:
    """One tract's segmentation (edits and runs None: an empty tract, one beyond the limits, or a region that is not
    segmented)."""

    def __init__(self, tract_len, motif_set=None):
        self.tract_len = tract_len
        self.motif_set = motif_set
        self.edits = self.runs = None

    def units(self):
        return None if self.runs is None else units_per_motif(self.runs, self.motif_set)

    def fields(self):
        if self.runs is None:
            return [str(self.tract_len), "-", "-", "-"]
        per = ",".join(f"{u}={x:.1f}" for u, x in zip(self.motif_set, self.units()))
        return [str(self.tract_len), str(self.edits), runs_text(self.runs, self.motif_set), per]


def motif_supported(unit):
    u = unit.upper()
    return 1 <= len(u) <= MAX_STATES and not set(u) - set("ACGT")


def nearest_rotation(cls, unit):
    """The rotation of `cls` nearest to `unit` (of the same length) in Hamming distance, the smallest one on ties."""
    rots = sorted({cls[r:] + cls[:r] for r in range(len(cls))})
    return min(rots, key=lambda w: sum(a != b for a, b in zip(w, unit)))


def discovered_classes(region):
    """The classes section 15 calls for the region, [(class, read support)] by support descending, then class: the
    Motif_Groups classes and every allele's dominant and secondary classes; the support of a class is the number of the
    region's reads that show it with at least 10 % of their top count."""
    classes = {c for c, _, _ in nr_motifs.motif_groups(region)}
    for _, dom, _, second in nr_motifs.allele_motifs(region):
        classes |= {c for c in [dom] + list(second) if c}
    support = dict.fromkeys(classes, 0)
    for rm in (getattr(region, "read_motifs", None) or {}).values():
        if rm.top:
            floor = 0.1 * rm.top[0][1]
            for c in {c for c, k in rm.top if k >= floor} & classes:
                support[c] += 1
    return sorted(support.items(), key=lambda kv: (-kv[1], kv[0]))


def region_motif_set(region, given=None):
    """The motif set of a region (None: not segmented).  `given`: the caller's motifs for it, or None for the
    discovered classes (region.read_motifs must be filled then)."""
    unit = region.repeat_unit_seq.upper()
    if not motif_supported(unit):
        return None
    out = [unit]
    if given is not None:
        for u in given:
            u = u.upper()
            if not u or set(u) - set("ACGT"):
                raise ValueError(f"segment_motifs: {u!r} is not a motif of A, C, G, T")
            if u not in out:
                out.append(u)
        if len(out) > MAX_MOTIFS or sum(len(u) for u in out) > MAX_STATES:
            raise ValueError(f"segment_motifs: {out} exceeds {MAX_MOTIFS} motifs or {MAX_STATES} bases in all")
        return out
    bed = nr_motifs.bed_class(unit)
    for cls, _ in discovered_classes(region):
        if cls == bed or (len(cls) == 1 and len(unit) != 1):
            continue
        u = nearest_rotation(cls, unit) if len(cls) == len(unit) else cls
        if u in out or len(out) >= MAX_MOTIFS or sum(len(x) for x in out) + len(u) > MAX_STATES:
            continue
        out.append(u)
    return out


def _segment(owners, engine, switch_cost, device):
    """owners = [(TractRuns, tract)] with a motif set each: one call of `engine`, results into the TractRuns."""
    sets, set_of, tracts, tract_set = [], {}, [], []
    for tr, tract in owners:
        key = tuple(tr.motif_set)
        if key not in set_of:
            set_of[key] = len(sets)
            sets.append(list(key))
        tracts.append(tract)
        tract_set.append(set_of[key])
    if not tracts:
        return
    out = engine(sets, tracts, np.array(tract_set, np.int32), switch_cost, device=device)
    off = out["path_off"]
    for i, (tr, _) in enumerate(owners):
        tr.edits = int(out["edits"][i])
        tr.runs = derive_runs(out["path"][off[i]:off[i + 1]], out["motif_of"][off[i]:off[i + 1]])


def segments_regions(repeat_regions, device=0, engine=None, segment_motifs=None, switch_cost=None, motif_engine=None,
                     consensus_engine=None, structure_engine=None):
    """The runs of every read with a core and of every allele consensus of every region, in two calls of `engine`
    (default _capi.tract_segments; tests pass a restatement with the same signature).  The discovered classes come from
    `region.read_motifs` where motifs.motif_regions has run, else nra_tract_motifs runs here (`motif_engine`) without
    re-sizing any read; the consensuses from `region.allele_consensus` where consensus.consensus_regions has run, else
    it runs here (`consensus_engine`, `structure_engine`).  No file of those steps is written on that account.  Sets
    `region.motif_set`, `region.read_runs` = {read name: TractRuns}, `region.allele_runs` = [(allele id, TractRuns)]
    and `region.switch_cost`; returns the regions."""
    from . import _capi
    engine = engine or _capi.tract_segments
    W = DEFAULT_SWITCH_COST if switch_cost is None else int(switch_cost)
    if not 1 <= W <= MAX_SWITCH_COST:
        raise ValueError(f"switch_cost must be 1..{MAX_SWITCH_COST}")
    segment_motifs = segment_motifs or {}
    need = [r for r in repeat_regions if r.to_unique_id() not in segment_motifs
            and motif_supported(r.repeat_unit_seq) and getattr(r, "read_motifs", None) is None]
    if need:
        nr_motifs.motif_regions(need, device=device, engine=motif_engine, resize=False)
    todo = [r for r in repeat_regions if getattr(r, "allele_consensus", None) is None]
    if todo:
        consensus.consensus_regions(todo, device=device, engine=consensus_engine, structure_engine=structure_engine)
    read_owners, allele_owners = [], []
    for region in repeat_regions:
        region.switch_cost = W
        region.motif_set = mset = region_motif_set(region, segment_motifs.get(region.to_unique_id()))
        region.read_runs, region.allele_runs = {}, []
        for name in region.read_dict:
            if name not in region.read_core_seq_dict:
                continue
            tract = structure.tract_of(region, name).upper()
            region.read_runs[name] = tr = TractRuns(len(tract), mset)
            if mset is not None and 0 < len(tract) <= MAX_TRACT_LEN:
                read_owners.append((tr, tract))
        for ac in region.allele_consensus:
            tr = TractRuns(len(ac.sequence), mset)
            region.allele_runs.append((ac.allele_id, tr))
            if mset is not None and 0 < len(ac.sequence) <= MAX_TRACT_LEN:
                allele_owners.append((tr, ac.sequence))
    _segment(read_owners, engine, W, device)
    _segment(allele_owners, engine, W, device)
    return repeat_regions


def _ordered_reads(region):
    """phased_reads.txt order (allele by allele), then the other reads with a core by name: [(name, allele id)]."""
    res = phasing.results_of(region)
    cored = list(getattr(region, "read_runs", None) or {})
    label = {n: q.allele_id for n, q in res.quantified_read_dict.items()}
    phased = sorted((n for n in cored if label.get(n, -1) >= 1), key=lambda n: label[n])   # stable: file order
    rest = sorted(n for n in cored if label.get(n, -1) < 1)
    return [(n, str(label[n])) for n in phased] + [(n, ".") for n in rest]


def read_runs_text(region):
    mset = getattr(region, "motif_set", None)
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motifs={','.join(mset) if mset else '-'}\n",
             f"##Switch_Cost={getattr(region, 'switch_cost', DEFAULT_SWITCH_COST)}\n",
             "#Read_Name\tAllele_ID\tTract_Len\tEdits\tRuns\tUnits_Per_Motif\n"]
    runs = getattr(region, "read_runs", None) or {}
    for name, allele in _ordered_reads(region):
        lines.append("\t".join([name, allele] + runs[name].fields()) + "\n")
    return "".join(lines)


def write_read_runs(region):
    """`<region out_prefix>.read_runs.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.read_runs.tsv"
    with open(path, "w") as f:
        f.write(read_runs_text(region))
    return path


def allele_units(region):
    """Per allele, in phasing order: (id, reads with runs, [median units per motif of the set] or None, TractRuns of the
    allele's consensus)."""
    res = phasing.results_of(region)
    runs = getattr(region, "read_runs", None) or {}
    out = []
    for label, cons in getattr(region, "allele_runs", None) or []:
        reads = [runs[n] for n, q in res.quantified_read_dict.items()
                 if q.allele_id == label and n in runs and runs[n].runs is not None]
        med = [float(x) for x in np.median([r.units() for r in reads], axis=0)] if reads else None
        out.append((label, len(reads), med, cons))
    return out


def runs_summary_row(region):
    mset = getattr(region, "motif_set", None)
    cells = []
    for label, n, med, cons in allele_units(region):
        per = "-" if med is None else ",".join(f"{u}={x:.1f}" for u, x in zip(mset, med))
        cells.append(f"{label}:{n}:{per}:{'-' if cons.runs is None else runs_text(cons.runs, mset)}")
    start = max(0, region.start_pos)
    return (f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t{len(cells)}\t"
            f"{','.join(mset) if mset else '-'}\t{'|'.join(cells) or '-'}\n")


def write_runs_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_runs.tsv`: one row per BED region, in BED order; per allele
    id:reads:motif=median units over the allele's reads, per motif of the set:runs of the allele's consensus."""
    path = f"{out_prefix}.NanoRepeat_runs.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tMotif_Set\tAllele_Runs\n")
        f.write("".join(runs_summary_row(region) for region in regions))
    return path


def report_multi_run_alleles(repeat_regions, stream=None):
    """One NOTICE for the command: how many alleles have a consensus of more than one run.  Returns (such, alleles)."""
    import sys
    stream = stream or sys.stderr
    alleles = [tr for region in repeat_regions for _, tr in getattr(region, "allele_runs", None) or []]
    n = sum(1 for tr in alleles if tr.runs is not None and len(tr.runs) > 1)
    print(f"NOTICE: motif runs: the consensus of {n} of {len(alleles)} allele(s) has more than one motif run",
          file=stream)
    return n, len(alleles)
