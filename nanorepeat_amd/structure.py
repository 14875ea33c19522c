"""Repeat structure per read and per allele (no counterpart in the reference): every quantified
read's tract -- the oriented core between its two anchors -- is aligned against the region's motif repeated without
end (nra_read_structure, one call for all regions), and the alignment is cut into motif units on the host:

* a counter c starts at the start phase; each match, mismatch and deleted motif base belongs to slot c // p and
  advances c, an insertion belongs to slot c // p without advancing it;
* a slot is complete when it holds all p motif positions, pure when it is complete and holds exactly p matches;
* Purity = matches / (matches + mismatches + insertions + deletions), Pure_Units, Longest_Pure_Run (consecutive pure
  slots) and Interruptions: the maximal runs of consecutive complete, non-pure slots as `<first slot>:<read bases>`.

`structure_regions` fills `region.read_structure`; `write_read_structure` and `write_structure_summary` write
`<region>.read_structure.tsv` and `<out_prefix>.NanoRepeat_structure.tsv`.
"""
import numpy as np

from . import phasing

MATCH, MISMATCH, INSERTION = 0, 1, 2
MAX_MOTIF_LEN = 64
MAX_TRACT_LEN = 200000


class ReadStructure:
    """One read's alignment and the fields derived from it (None: an empty tract, or a read left out)."""

    def __init__(self, tract_len, edits=None, purity=None, pure_units=None, longest_pure_run=None, interruptions=()):
        self.tract_len = tract_len
        self.edits = edits
        self.purity = purity
        self.pure_units = pure_units
        self.longest_pure_run = longest_pure_run
        self.interruptions = list(interruptions)      # [(first slot, read bases or "-")]

    def fields(self):
        if self.purity is None:
            edits = "-" if self.edits is None else str(self.edits)
            return [str(self.tract_len), edits, "-", "-", "-", "-"]
        inter = ",".join(f"{k}:{b}" for k, b in self.interruptions) or "-"
        return [str(self.tract_len), str(self.edits), f"{self.purity:.4f}", str(self.pure_units),
                str(self.longest_pure_run), inter]


def derive_units(tract, p, start_phase, path):
    """(tract, motif length, start phase, path bytes) -> (purity, pure_units, longest_pure_run, interruptions) or
    None for an empty tract."""
    n = len(path)
    if n == 0:
        return None
    pos, matches, bases = {}, {}, {}            # per slot: motif positions, matches, read bases
    c = start_phase
    n_match = n_other = 0
    for i in range(n):
        b = int(path[i])
        op, nd = b & 3, b >> 2
        k = c // p
        bases[k] = bases.get(k, "") + tract[i]
        if op == INSERTION:
            n_other += 1
        else:
            pos[k] = pos.get(k, 0) + 1
            if op == MATCH:
                matches[k] = matches.get(k, 0) + 1
                n_match += 1
            else:
                n_other += 1
            c += 1
        for _ in range(nd):
            k = c // p
            pos[k] = pos.get(k, 0) + 1
            n_other += 1
            c += 1
    last = max(max(pos, default=0), max(bases, default=0))
    pure_units = longest = run = 0
    interruptions, cur = [], None
    for k in range(start_phase // p, last + 1):
        complete = pos.get(k, 0) == p
        pure = complete and matches.get(k, 0) == p and len(bases.get(k, "")) == p
        run = run + 1 if pure else 0
        pure_units += pure
        longest = max(longest, run)
        if complete and not pure:
            cur = cur or [k, ""]
            cur[1] += bases.get(k, "")
        elif cur is not None:
            interruptions.append((cur[0], cur[1] or "-"))
            cur = None
    if cur is not None:
        interruptions.append((cur[0], cur[1] or "-"))
    return n_match / (n_match + n_other), pure_units, longest, interruptions


def tract_of(region, read_name):
    """The oriented read between the two anchors: core[left_buffer_len : len(core) - right_buffer_len]."""
    core = region.read_core_seq_dict[read_name].strip()
    read = region.read_dict[read_name]
    lo, hi = read.left_buffer_len, len(core) - read.right_buffer_len
    return core[lo:hi] if hi > lo else ""


def motif_supported(unit):
    u = unit.upper()
    return 1 <= len(u) <= MAX_MOTIF_LEN and not set(u) - set("ACGT")


def structure_regions(repeat_regions, device=0, engine=None):
    """The structure of every read with a round-3 size in every region, in one call of `engine` (default
    _capi.read_structure; tests pass a restatement with the same signature).  Regions whose motif is longer than 64
    bases or not ACGT are not aligned: their reads get `-` fields.  Sets `region.read_structure` =
    {read_name: ReadStructure} and returns the regions."""
    if engine is None:
        from . import _capi
        engine = _capi.read_structure
    motifs, motif_of, tracts, read_motif, owners = [], {}, [], [], []
    for region in repeat_regions:
        region.read_structure = {}
        unit = region.repeat_unit_seq.upper()
        ok = motif_supported(unit)
        if ok and unit not in motif_of:
            motif_of[unit] = len(motifs)
            motifs.append(unit)
        for name, read in region.read_dict.items():
            if read.round3_repeat_size is None:
                continue
            tract = tract_of(region, name)
            region.read_structure[name] = ReadStructure(len(tract))
            if ok and 0 < len(tract) <= MAX_TRACT_LEN:
                tracts.append(tract.upper())
                read_motif.append(motif_of[unit])
                owners.append((region, name, len(unit)))
    if not tracts:
        return repeat_regions
    out = engine(motifs, tracts, np.array(read_motif, np.int32), device=device)
    off = out["path_off"]
    for i, (region, name, p) in enumerate(owners):
        path = out["path"][off[i]:off[i + 1]]
        purity, pure_units, longest, inter = derive_units(tracts[i], p, int(out["start_phase"][i]), path)
        rs = region.read_structure[name]
        rs.edits, rs.purity, rs.pure_units, rs.longest_pure_run, rs.interruptions = \
            int(out["edits"][i]), purity, pure_units, longest, inter
    return repeat_regions


def _ordered_reads(region):
    """phased_reads.txt order (allele by allele), then the other reads with a size by name: [(name, allele id)]."""
    res = phasing.results_of(region)
    sized = [n for n, r in region.read_dict.items() if r.round3_repeat_size is not None]
    label = {n: q.allele_id for n, q in res.quantified_read_dict.items()}
    phased = sorted((n for n in sized if label.get(n, -1) >= 1), key=lambda n: label[n])   # stable: file order
    rest = sorted(n for n in sized if label.get(n, -1) < 1)
    return [(n, str(label[n])) for n in phased] + [(n, ".") for n in rest]


def read_structure_text(region):
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tEdits\tPurity\tPure_Units\tLongest_Pure_Run\t"
             "Interruptions\n"]
    rs = getattr(region, "read_structure", None) or {}
    for name, allele in _ordered_reads(region):
        size = region.read_dict[name].round3_repeat_size
        lines.append("\t".join([name, allele, f"{size:.1f}"] + rs[name].fields()) + "\n")
    return "".join(lines)


def write_read_structure(region):
    """`<region out_prefix>.read_structure.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.read_structure.tsv"
    with open(path, "w") as f:
        f.write(read_structure_text(region))
    return path


def allele_structures(region):
    """Per allele, in phasing order: (id, n reads, median purity, median Pure_Units, median Longest_Pure_Run,
    [(bases, median first slot)] recurrent interruptions).  Reads with an empty tract (or left out) do not count."""
    res = phasing.results_of(region)
    rs = getattr(region, "read_structure", None) or {}
    out = []
    for label in range(1, len(res.quantified_allele_list) + 1):
        reads = [rs[n] for n, q in res.quantified_read_dict.items()
                 if q.allele_id == label and n in rs and rs[n].purity is not None]
        if not reads:
            out.append((label, 0, None, None, None, []))
            continue
        slots = {}
        for r in reads:
            seen = {}
            for k, b in r.interruptions:
                rank = seen.get(b, 0)
                seen[b] = rank + 1
                slots.setdefault((b, rank), []).append(k)
        recurrent = sorted(((b, float(np.median(ks))) for (b, _), ks in slots.items() if 2 * len(ks) >= len(reads)),
                           key=lambda t: (t[1], t[0]))
        out.append((label, len(reads), float(np.median([r.purity for r in reads])),
                    float(np.median([r.pure_units for r in reads])),
                    float(np.median([r.longest_pure_run for r in reads])), recurrent))
    return out


def structure_summary_row(region):
    alleles = allele_structures(region)
    start = max(0, region.start_pos)
    cells = []
    for label, n, purity, pure, longest, recurrent in alleles:
        if n == 0:
            cells.append(f"{label}:0:-:-:-:-")
            continue
        rec = ";".join(f"{b}@{k:.1f}" for b, k in recurrent) or "-"
        cells.append(f"{label}:{n}:{purity:.4f}:{pure:.1f}:{longest:.1f}:{rec}")
    return (f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}\t{len(alleles)}\t"
            f"{'|'.join(cells) or '-'}\n")


def write_structure_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_structure.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_structure.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Structure\n")
        f.write("".join(structure_summary_row(region) for region in regions))
    return path
