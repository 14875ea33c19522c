"""Tandem motifs per read, per motif group and per allele (no counterpart in the reference): every
read with a core has its tract -- the oriented core between its two anchors -- screened for tandem motifs of period 1..6
(nra_tract_motifs, one call for all regions).  On the host:

* a read's dominant motif is its top class when that class's count is >= max(min_motif_count, min_motif_share x tract
  length); otherwise the read has no call;
* the BED class is the class of the BED motif's primitive root when that root is 1..6 bases of ACGT, else none (no
  read of the region is re-sized);
* a read whose call differs from the BED class is sized again in its own motif: region (left anchor, u', right anchor)
  with u' the rotation of the class whose doubled word occurs first in the tract, window round3_window(tract length /
  |u'|), all such reads of all regions in one call of the round-3 scorer; its size is sum_k / n_ties when READ_OK.
  A read whose call is the BED class keeps its round-3 size.

Nothing here changes read_dict, the phasing or any other output.  `motif_regions` fills `region.read_motifs`;
`write_read_motifs` and `write_motif_summary` write `<region>.read_motifs.tsv` and `<out_prefix>.NanoRepeat_motifs.tsv`.
"""
import numpy as np

from . import _capi, phasing, round3, structure

BASES = "ACGT"
MAX_PERIOD = 6
TOP_N = 4
MAX_TRACT_LEN = 200000
MIN_MOTIF_COUNT = 4
MIN_MOTIF_SHARE = 0.1


def class_string(p, code):
    """(p, base-4 code, first base most significant) -> the bases."""
    return "".join(BASES[(code >> (2 * (p - 1 - j))) & 3] for j in range(p))


def motif_class(word):
    """The smallest rotation of an ACGT word (A < C < G < T)."""
    w = word.upper()
    return min(w[r:] + w[:r] for r in range(len(w))) if w else w


def primitive_root(word):
    """The shortest x with word == x^m."""
    p = len(word)
    for d in range(1, p + 1):
        if p % d == 0 and word[:d] * (p // d) == word:
            return word[:d]
    return word


def bed_class(unit):
    """The class of the BED motif's primitive root when that root is 1..6 bases of ACGT, else None."""
    root = primitive_root(unit.upper())
    if not 1 <= len(root) <= MAX_PERIOD or set(root) - set(BASES):
        return None
    return motif_class(root)


def in_phase_unit(tract, cls):
    """The rotation of `cls` whose doubled word occurs first in the tract (None when none does)."""
    best, at = None, -1
    for r in range(len(cls)):
        u = cls[r:] + cls[:r]
        i = tract.find(u + u)
        if i >= 0 and (at < 0 or i < at):
            best, at = u, i
    return best


def dominant_call(top, tract_len, min_motif_count=MIN_MOTIF_COUNT, min_motif_share=MIN_MOTIF_SHARE):
    """top = [(class, count)] by count descending -> the dominant class or None."""
    if not top:
        return None
    cls, count = top[0]
    return cls if count > 0 and count >= max(min_motif_count, min_motif_share * tract_len) else None


class ReadMotifs:
    """One read's tract motifs, its call and its size in that motif (None: no call, or no size)."""

    def __init__(self, tract_len, top=(), call=None):
        self.tract_len = tract_len
        self.top = list(top)                 # [(class, count)], count descending
        self.call = call
        self.differs = None                  # True / False, None when there is no call or no BED class
        self.size_in_motif = None

    def fields(self):
        differs = "-" if self.differs is None else "yes" if self.differs else "no"
        size = "-" if self.size_in_motif is None else f"{self.size_in_motif:.1f}"
        top = ",".join(f"{c}:{k}" for c, k in self.top) or "-"
        return [str(self.tract_len), self.call or "-", differs, size, top]


def motif_regions(repeat_regions, fast_mode=False, device=0, engine=None, scorer=None, scoring=None,
                  max_period=MAX_PERIOD, top_n=TOP_N, min_motif_count=MIN_MOTIF_COUNT,
                  min_motif_share=MIN_MOTIF_SHARE, resize=True):
    """The motifs of every read with a core in every region (one call of `engine`, default _capi.tract_motifs; tests
    pass a restatement with the same signature), the calls, and the re-sizing of the reads whose call is not the BED
    class (one call of `scorer`, default _capi.round3_1d, as round 3 uses it; not with resize=False, which leaves
    every Size_In_Motif empty: segments.py wants the classes only).  Sets `region.read_motifs` =
    {read_name: ReadMotifs} and `region.motif_bed_class`; returns the regions."""
    engine = engine or _capi.tract_motifs
    scorer = scorer or _capi.round3_1d
    tracts, owners = [], []
    for region in repeat_regions:
        region.read_motifs = {}
        region.motif_bed_class = bed_class(region.repeat_unit_seq)
        for name in region.read_dict:
            if name not in region.read_core_seq_dict:
                continue
            tract = structure.tract_of(region, name).upper()
            region.read_motifs[name] = ReadMotifs(len(tract))
            if len(tract) <= MAX_TRACT_LEN:
                tracts.append(tract)
                owners.append((region, name))
    if tracts:
        out = engine(tracts, max_period=max_period, top_n=top_n, device=device)
        for i, (region, name) in enumerate(owners):
            rm = region.read_motifs[name]
            rm.top = [(class_string(int(p), int(c)), int(k))
                      for p, c, k in zip(out["top_p"][i], out["top_code"][i], out["top_count"][i]) if k > 0]
            rm.call = dominant_call(rm.top, rm.tract_len, min_motif_count, min_motif_share)
    if resize:
        _resize(repeat_regions, fast_mode, device, scorer, scoring)
    return repeat_regions


def _resize(repeat_regions, fast_mode, device, scorer, scoring):
    units, reads, kmin, kmax, rr, owners = [], [], [], [], [], []
    unit_of = {}
    for g, region in enumerate(repeat_regions):
        bed = region.motif_bed_class
        for name, rm in region.read_motifs.items():
            if rm.call is None or bed is None:
                continue
            rm.differs = rm.call != bed
            if not rm.differs:
                rm.size_in_motif = region.read_dict[name].round3_repeat_size
                continue
            tract = structure.tract_of(region, name).upper()
            unit = in_phase_unit(tract, rm.call)
            if unit is None:
                continue
            lo, hi = round3.round3_window(len(tract) / len(unit), fast_mode)
            seq = region.read_core_seq_dict[name].strip()
            template_len = len(region.left_anchor_seq) + len(unit) * hi + len(region.right_anchor_seq)
            if len(seq) > round3.MAX_CORE_LEN or template_len > round3.MAX_TEMPLATE_LEN:
                continue
            key = (g, unit)
            if key not in unit_of:
                unit_of[key] = len(units)
                units.append((region.left_anchor_seq, unit, region.right_anchor_seq))
            reads.append(seq); kmin.append(lo); kmax.append(hi); rr.append(unit_of[key]); owners.append(rm)
    if not reads:
        return
    out = scorer(units, reads, np.array(kmin, np.int32), np.array(kmax, np.int32), read_region=np.array(rr, np.int32),
                 sc=scoring, device=device, per_candidate=False)
    for i, rm in enumerate(owners):
        if int(out["status"][i]) == _capi.READ_OK:
            rm.size_in_motif = np.float64(out["sum_k"][i]) / np.float64(out["n_ties"][i])


def _ordered_reads(region, per_read="read_motifs"):
    """phased_reads.txt order (allele by allele), then the other reads with a core by name: [(name, allele id)].  The
    reads with a core are the keys of the region's `per_read` dict."""
    res = phasing.results_of(region)
    cored = list(getattr(region, per_read, None) or {})
    label = {n: q.allele_id for n, q in res.quantified_read_dict.items()}
    phased = sorted((n for n in cored if label.get(n, -1) >= 1), key=lambda n: label[n])   # stable: file order
    rest = sorted(n for n in cored if label.get(n, -1) < 1)
    return [(n, str(label[n])) for n in phased] + [(n, ".") for n in rest]


def read_motifs_text(region):
    bed = getattr(region, "motif_bed_class", None)
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             f"##BED_Class={bed or '-'}\n",
             "#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tDominant_Motif\tDiffers\tSize_In_Motif\tTop_Motifs\n"]
    rms = getattr(region, "read_motifs", None) or {}
    for name, allele in _ordered_reads(region):
        size = region.read_dict[name].round3_repeat_size
        lines.append("\t".join([name, allele, "-" if size is None else f"{size:.1f}"] + rms[name].fields()) + "\n")
    return "".join(lines)


def write_read_motifs(region):
    """`<region out_prefix>.read_motifs.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.read_motifs.tsv"
    with open(path, "w") as f:
        f.write(read_motifs_text(region))
    return path


def motif_groups(region):
    """Every called class dominant in at least max(2, 10 %) of the region's called reads, independent of phasing:
    [(class, reads, median Size_In_Motif or None)] by reads descending, then class."""
    rms = getattr(region, "read_motifs", None) or {}
    called = [rm for rm in rms.values() if rm.call is not None]
    by = {}
    for rm in called:
        by.setdefault(rm.call, []).append(rm)
    need = max(2, 0.1 * len(called))
    out = []
    for cls, members in by.items():
        if len(members) < need:
            continue
        sizes = [rm.size_in_motif for rm in members if rm.size_in_motif is not None]
        out.append((cls, len(members), float(np.median(sizes)) if sizes else None))
    return sorted(out, key=lambda t: (-t[1], t[0]))


def allele_motifs(region):
    """Per allele, in phasing order: (id, dominant class or None, share of the allele's reads, [secondary classes]).
    Secondary: the other classes in the top T of at least half of the allele's reads with a count of at least 10 % of
    that read's top count."""
    res = phasing.results_of(region)
    rms = getattr(region, "read_motifs", None) or {}
    out = []
    for label in range(1, len(res.quantified_allele_list) + 1):
        reads = [rms[n] for n, q in res.quantified_read_dict.items() if q.allele_id == label and n in rms]
        calls = {}
        for rm in reads:
            if rm.call is not None:
                calls[rm.call] = calls.get(rm.call, 0) + 1
        if not calls:
            out.append((label, None, 0.0, []))
            continue
        dom = sorted(calls.items(), key=lambda kv: (-kv[1], kv[0]))[0][0]
        seen = {}
        for rm in reads:
            if not rm.top:
                continue
            floor = 0.1 * rm.top[0][1]
            for cls in {c for c, k in rm.top if k >= floor}:
                seen[cls] = seen.get(cls, 0) + 1
        second = sorted((c for c, k in seen.items() if c != dom and 2 * k >= len(reads)), key=lambda c: (-seen[c], c))
        out.append((label, dom, calls[dom] / len(reads), second))
    return out


def motif_summary_row(region):
    start = max(0, region.start_pos)
    head = f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}"
    rms = getattr(region, "read_motifs", None) or {}
    if not rms:
        return f"{head}\t0\t-\t-\n"
    groups = ",".join(f"{c}:{n}:{'-' if m is None else f'{m:.1f}'}" for c, n, m in motif_groups(region)) or "-"
    alleles = "|".join(f"{label}:{dom or '-'}:{share:.2f}:{','.join(sec) or '-'}"
                       for label, dom, share, sec in allele_motifs(region)) or "-"
    return f"{head}\t{len(rms)}\t{groups}\t{alleles}\n"


def write_motif_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_motifs.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_motifs.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Reads\tMotif_Groups\tAllele_Motifs\n")
        f.write("".join(motif_summary_row(region) for region in regions))
    return path
