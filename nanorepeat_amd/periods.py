"""Tandem periods up to 64 bases per allele and per read (no counterpart in the reference): the
statistic is the lag-match spectrum of a tract, match[p] / valid[p] for p = 1..64 (nra_tract_periods, one call for all
regions over every read's tract and every allele's consensus tract).  All rules are functions of those integers:

* the period of a sequence (`call_period`): share[p] = match[p] / valid[p] where valid[p] >= max(min_valid, p); no call
  when the largest share is below min_share; else the smallest p whose share is within tol of the largest (5 before 10
  and 15, 12 before 24);
* an allele's period is the period of its consensus tract (consensus.py); its unit (`unit_of`) is the first exact
  tandem copy of that length in the consensus -- ACGT, primitive -- rotated into phase with the tract's first base;
* a read's evidence: its own call, its support -- the largest share over the lags p - 1, p, p + 1 of its allele's
  period p, the window that absorbs an indel -- and its top three lags;
* when the allele's unit is of another class than the BED motif's primitive root, the allele's reads are sized in that
  unit by the round-3 scorer, as motifs.py re-sizes: region (left anchor, unit, right anchor), window
  round3_window(tract length / p), all such reads of all regions in one call; the size is sum_k / n_ties when READ_OK.
  Where the classes agree a read keeps its round-3 size.

Nothing here changes read_dict, the phasing or any other output.  `period_regions` fills `region.read_periods` and
`region.allele_periods`; `write_read_periods` and `write_period_summary` write `<region>.read_periods.tsv` and
`<out_prefix>.NanoRepeat_periods.tsv`; `report_foreign_units` counts the alleles whose unit is not the BED motif's.
"""
import numpy as np

from . import _capi, consensus, motifs, phasing, round3, structure

MAX_PERIOD = 64
MAX_TRACT_LEN = 200000
MIN_SHARE = 0.6          # the thresholds are section 22.3's: what was tried, and what each achieves
TOL = 0.05
MIN_VALID = 12
TOP_LAGS = 3


def shares_of(match, valid, min_valid=MIN_VALID):
    """share[p - 1] = match / valid where valid >= max(min_valid, p, 1), NaN elsewhere."""
    match, valid = np.asarray(match, np.int64), np.asarray(valid, np.int64)
    need = np.maximum(np.arange(1, len(valid) + 1), max(int(min_valid), 1))
    out = np.full(len(valid), np.nan)
    ok = valid >= need
    out[ok] = match[ok] / valid[ok]
    return out


def call_period(match, valid, min_share=MIN_SHARE, tol=TOL, min_valid=MIN_VALID):
    """-> (period or None, its share; without a call the largest share, None when no lag has a share)."""
    sh = shares_of(match, valid, min_valid)
    if np.isnan(sh).all():
        return None, None
    best = float(np.nanmax(sh))
    if best < min_share:
        return None, best
    p = int(np.nonzero(sh >= best - tol)[0][0]) + 1          # NaN compares false
    return p, float(sh[p - 1])


def unit_of(cons, p):
    """The first ACGT, primitive word w = cons[i:i+p] == cons[i+p:i+2p], rotated back by i mod p (in phase with the
    tract's first base); None when there is none."""
    cons = cons.upper()
    for i in range(0, len(cons) - 2 * p + 1):
        w = cons[i:i + p]
        if cons[i + p:i + 2 * p] == w and not set(w) - set("ACGT") and motifs.primitive_root(w) == w:
            r = i % p
            return w[p - r:] + w[:p - r]
    return None


def root_class(unit):
    """The class of the primitive root of an ACGT word of any length, else None."""
    root = motifs.primitive_root(unit.upper())
    if not root or set(root) - set("ACGT"):
        return None
    return motifs.motif_class(root)


def support_of(match, valid, period, min_valid=MIN_VALID):
    """The largest share over the lags period - 1, period, period + 1 (None when none of them has a share)."""
    sh = shares_of(match, valid, min_valid)
    window = [sh[p - 1] for p in (period - 1, period, period + 1) if 1 <= p <= len(sh) and not np.isnan(sh[p - 1])]
    return float(max(window)) if window else None


def top_lags(match, valid, top=TOP_LAGS, min_valid=MIN_VALID):
    """[(lag, share)] of the `top` largest shares, share descending, then lag ascending."""
    sh = shares_of(match, valid, min_valid)
    lags = [p for p in range(1, len(sh) + 1) if not np.isnan(sh[p - 1])]
    return [(p, float(sh[p - 1])) for p in sorted(lags, key=lambda p: (-sh[p - 1], p))[:top]]


def _f2(x):
    return "-" if x is None else f"{x:.2f}"


class ReadPeriods:
    """One read's call and its evidence for its allele's period (None: no call, no allele period, or no size)."""

    def __init__(self, tract_len):
        self.tract_len = tract_len
        self.call = self.share = self.support = self.size_in_unit = None
        self.top = []

    def fields(self):
        size = "-" if self.size_in_unit is None else f"{self.size_in_unit:.1f}"
        top = ",".join(f"{p}:{s:.2f}" for p, s in self.top) or "-"
        return [str(self.tract_len), "-" if self.call is None else str(self.call), _f2(self.share),
                _f2(self.support), size, top]


class AllelePeriods:
    """One allele: the period and the unit of its consensus tract, and whether the unit is of the BED motif's class."""

    def __init__(self, allele_id, read_names, sequence):
        self.allele_id = allele_id
        self.read_names = read_names
        self.sequence = sequence             # the allele's consensus tract
        self.period = self.share = self.unit = None
        self.differs = None                  # True / False, None without a unit

    def cell(self, read_periods):
        rps = [read_periods[n] for n in self.read_names if n in read_periods]
        called = [rp for rp in rps if rp.call is not None]
        same = sum(rp.call == self.period for rp in called) if self.period is not None else 0
        support = [rp.support for rp in rps if rp.support is not None]
        sizes = [rp.size_in_unit for rp in rps if rp.size_in_unit is not None]
        return (f"{self.allele_id}:{'-' if self.period is None else self.period}:{self.unit or '-'}:{_f2(self.share)}:"
                f"{same}/{len(called)}:{_f2(float(np.median(support)) if support else None)}:"
                f"{f'{float(np.median(sizes)):.1f}' if sizes else '-'}")


def period_regions(repeat_regions, fast_mode=False, device=0, engine=None, scorer=None, scoring=None,
                   consensus_engine=None, structure_engine=None, max_period=MAX_PERIOD, min_share=MIN_SHARE, tol=TOL,
                   min_valid=MIN_VALID):
    """The spectra of every read's tract and of every allele's consensus tract in one call of `engine` (default
    _capi.tract_periods; tests pass a restatement with the same signature), the calls, and the sizing of the reads of
    the alleles whose unit is not of the BED motif's class (one call of `scorer`, default _capi.round3_1d).  The
    consensus of an allele is `region.allele_consensus` where consensus.consensus_regions has run, else it runs here (no
    consensus file is written on that account).  Sets `region.read_periods` = {read name: ReadPeriods} and
    `region.allele_periods` = [AllelePeriods]; returns the regions."""
    engine = engine or _capi.tract_periods
    scorer = scorer or _capi.round3_1d
    todo = [r for r in repeat_regions if getattr(r, "allele_consensus", None) is None]
    if todo:
        consensus.consensus_regions(todo, device=device, engine=consensus_engine or _capi.tract_consensus,
                                    structure_engine=structure_engine or _capi.read_structure)
    tracts, owners = [], []
    for region in repeat_regions:
        region.read_periods, region.allele_periods = {}, []
        for name in region.read_dict:
            if name not in region.read_core_seq_dict:
                continue
            tract = structure.tract_of(region, name).upper()
            region.read_periods[name] = ReadPeriods(len(tract))
            if len(tract) <= MAX_TRACT_LEN:
                tracts.append(tract)
                owners.append(region.read_periods[name])
        res = phasing.results_of(region)
        for label, ac in zip(range(1, len(res.quantified_allele_list) + 1), region.allele_consensus):
            names = [n for n, q in res.quantified_read_dict.items() if q.allele_id == label]
            ap = AllelePeriods(label, names, ac.sequence)
            region.allele_periods.append(ap)
            tracts.append(ac.sequence)
            owners.append(ap)
    if not tracts:
        return repeat_regions
    out = engine(tracts, max_period=max_period, device=device)
    spectrum = {id(o): (out["match"][i], out["valid"][i]) for i, o in enumerate(owners)}
    for region in repeat_regions:
        bed = root_class(region.repeat_unit_seq)
        for ap in region.allele_periods:
            ap.period, ap.share = call_period(*spectrum[id(ap)], min_share=min_share, tol=tol, min_valid=min_valid)
            if ap.period is not None:
                ap.unit = unit_of(ap.sequence, ap.period)
            if ap.unit is not None:
                ap.differs = motifs.motif_class(ap.unit) != bed
            for name in ap.read_names:
                rp = region.read_periods.get(name)
                if rp is not None and id(rp) in spectrum and ap.period is not None:
                    rp.support = support_of(*spectrum[id(rp)], ap.period, min_valid=min_valid)
        for rp in region.read_periods.values():
            if id(rp) in spectrum:
                m, v = spectrum[id(rp)]
                rp.call, rp.share = call_period(m, v, min_share=min_share, tol=tol, min_valid=min_valid)
                rp.top = top_lags(m, v, min_valid=min_valid)
    _size_in_unit(repeat_regions, fast_mode, device, scorer, scoring)
    return repeat_regions


def _size_in_unit(repeat_regions, fast_mode, device, scorer, scoring):
    units, reads, kmin, kmax, rr, owners = [], [], [], [], [], []
    unit_at = {}
    for g, region in enumerate(repeat_regions):
        for ap in region.allele_periods:
            if ap.unit is None:
                continue
            for name in ap.read_names:
                rp = region.read_periods.get(name)
                if rp is None:
                    continue
                if not ap.differs:
                    rp.size_in_unit = region.read_dict[name].round3_repeat_size
                    continue
                tract = structure.tract_of(region, name)
                lo, hi = round3.round3_window(len(tract) / ap.period, fast_mode)
                seq = region.read_core_seq_dict[name].strip()
                template_len = len(region.left_anchor_seq) + len(ap.unit) * hi + len(region.right_anchor_seq)
                if len(seq) > round3.MAX_CORE_LEN or template_len > round3.MAX_TEMPLATE_LEN:
                    continue
                key = (g, ap.unit)
                if key not in unit_at:
                    unit_at[key] = len(units)
                    units.append((region.left_anchor_seq, ap.unit, region.right_anchor_seq))
                reads.append(seq); kmin.append(lo); kmax.append(hi); rr.append(unit_at[key]); owners.append(rp)
    if not reads:
        return
    out = scorer(units, reads, np.array(kmin, np.int32), np.array(kmax, np.int32), read_region=np.array(rr, np.int32),
                 sc=scoring, device=device, per_candidate=False)
    for i, rp in enumerate(owners):
        if int(out["status"][i]) == _capi.READ_OK:
            rp.size_in_unit = np.float64(out["sum_k"][i]) / np.float64(out["n_ties"][i])


def read_periods_text(region):
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n"]
    for ap in getattr(region, "allele_periods", None) or []:
        lines.append(f"##Allele={ap.allele_id} period={'-' if ap.period is None else ap.period} "
                     f"unit={ap.unit or '-'}\n")
    lines.append("#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tPeriod\tShare\tSupport\tSize_In_Unit\tTop_Lags\n")
    rps = getattr(region, "read_periods", None) or {}
    for name, allele in motifs._ordered_reads(region, "read_periods"):
        size = region.read_dict[name].round3_repeat_size
        lines.append("\t".join([name, allele, "-" if size is None else f"{size:.1f}"] + rps[name].fields()) + "\n")
    return "".join(lines)


def write_read_periods(region):
    """`<region out_prefix>.read_periods.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.read_periods.tsv"
    with open(path, "w") as f:
        f.write(read_periods_text(region))
    return path


def period_summary_row(region):
    start = max(0, region.start_pos)
    head = f"{region.chrom}\t{start}\t{region.end_pos}\t{region.repeat_unit_seq}"
    rps = getattr(region, "read_periods", None) or {}
    if not rps:
        return f"{head}\t0\t-\n"
    cells = "|".join(ap.cell(rps) for ap in getattr(region, "allele_periods", None) or []) or "-"
    return f"{head}\t{len(rps)}\t{cells}\n"


def write_period_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_periods.tsv`: one row per BED region, in BED order; per allele id:period:unit:consensus
    share:reads that call the same period/reads called:median support:median Size_In_Unit."""
    path = f"{out_prefix}.NanoRepeat_periods.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Reads\tAllele_Periods\n")
        f.write("".join(period_summary_row(region) for region in regions))
    return path


def report_foreign_units(repeat_regions, stream=None):
    """One NOTICE for the command: the alleles whose unit is of another class than the BED motif.  Returns (such
    alleles, alleles)."""
    import sys
    stream = stream or sys.stderr
    alleles = [ap for region in repeat_regions for ap in getattr(region, "allele_periods", None) or []]
    n = sum(1 for ap in alleles if ap.differs)
    print(f"NOTICE: tandem periods: {n} of {len(alleles)} allele(s) carry a unit that differs from the BED motif; "
          f"their reads are sized in that unit (Size_In_Unit)", file=stream)
    return n, len(alleles)
