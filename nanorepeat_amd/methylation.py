"""CpG methylation per read and per allele from the MM / ML tags (no counterpart in the reference).

A basecaller writes its 5mC calls into the MM / ML tags of every record: MM lists modified bases as "the k-th C of the
strand that was sequenced", ML holds one probability byte per listed base.  `parse_mm` turns the tag text of a read into
arrays on the host; nra_read_methylation (one call for all regions) ranks every read's bases from the 5' end of the
sequenced strand, looks the CpG sites of the repeat tract and of the flank bins on either side up in the list, and
counts them: sites, called sites, methylated (call byte >= meth_hi), unmethylated (<= meth_lo) and the sum of the call
bytes.  The sums per allele follow the phasing labels.

An ML byte b stands for a probability in [b / 256, (b + 1) / 256).  Frac = meth / (meth + unmeth); Mean =
(sum + called / 2) / (256 called), the mean of the bytes' interval midpoints.

`methylation_regions` fills `region.read_methylation`; `write_read_methylation`, `write_allele_methylation` and
`write_methylation_summary` write `<region>.read_methylation.tsv`, `<region>.allele_methylation.tsv` and
`<out_prefix>.NanoRepeat_methylation.tsv`.
"""
import re
import sys

import numpy as np

from . import phasing
from .structure import _ordered_reads

OK, NO_TAG, NO_MOD, BAD_TAG, CLIPPED = "OK", "NO_TAG", "NO_MOD", "BAD_TAG", "CLIPPED"
SITES, CALLED, METH, UNMETH, SUM = range(5)
MAX_FLANK, MAX_BINS = 100000, 64
DEVICE_BAD_TAG = 1                    # NRA_METH_BAD_TAG
F_REVERSED, F_IMPLICIT = 1, 2         # the flag bits of nra_read_methylation

_ENTRY = re.compile(r"^([A-Z])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[^,]*)*)$")


def parse_mm(mm_text, ml_bytes, base="C", mod_code="m"):
    """The list of one modification from a read's MM text and ML bytes -> (deltas int32[], probs uint8[], implicit), or
    a status.  Entries are separated by `;`, each `<base><strand><codes><flag>?(,<delta>)*` with codes one or more
    letters (`m`, `mh`) or one ChEBI number; the first entry with `base`, strand `+` and `mod_code` among its codes is
    taken.  ML is the concatenation over the entries in order: an entry of c codes and k deltas owns k c bytes,
    interleaved per position in the order of its codes.  Flag `?`: a skipped base is unknown (implicit False); `.` or
    none: it is unmodified.  NO_TAG: no MM at all; BAD_TAG: a malformed entry, a delta that is no number in 0..2^31-1,
    or an ML of another length than the entries ask for; NO_MOD: no entry matches."""
    if mm_text is None:
        return NO_TAG
    ml = bytes(ml_bytes) if ml_bytes is not None else b""
    found, at = None, 0
    for entry in mm_text.strip().split(";"):
        if not entry.strip():
            continue
        m = _ENTRY.match(entry.strip())
        if m is None:
            return BAD_TAG
        b, strand, codes, flag, rest = m.groups()
        words = rest.split(",")[1:]
        if any(not w.isdigit() or not w.isascii() or int(w) > 0x7fffffff for w in words):
            return BAD_TAG
        n_codes = 1 if codes[0].isdigit() else len(codes)
        has = codes == mod_code if codes[0].isdigit() else (len(mod_code) == 1 and mod_code in codes)
        if found is None and b == base and strand == "+" and has:
            found = (words, at + (0 if codes[0].isdigit() else codes.index(mod_code)), n_codes, flag != "?")
        at += len(words) * n_codes
    if at != len(ml):
        return BAD_TAG
    if found is None:
        return NO_MOD
    words, first, n_codes, implicit = found
    deltas = np.array([int(w) for w in words], np.int32)
    probs = np.frombuffer(ml, np.uint8)[first:first + len(words) * n_codes:n_codes].copy()
    return deltas, probs, implicit


def decode_read_tags(entry, mod_code="m"):
    """A read's (mm_text, ml_bytes, stored_reversed, usable), or None -> (status, deltas, probs, flag bits)."""
    if entry is None or (entry[0] is None and entry[1] is None):
        return NO_TAG, None, None, 0
    mm, ml, stored_reversed, usable = entry
    if not usable:
        return CLIPPED, None, None, 0
    got = parse_mm(mm, ml, "C", mod_code)
    if isinstance(got, str):
        return got, None, None, 0
    deltas, probs, implicit = got
    return OK, deltas, probs, (F_REVERSED if stored_reversed else 0) | (F_IMPLICIT if implicit else 0)


def check_options(flank, bin_len, hi, lo, mod_code):
    """ValueError for values nra_read_methylation would refuse, or that name no modification code."""
    for name, v in (("meth_flank", flank), ("meth_bin", bin_len), ("meth_hi", hi), ("meth_lo", lo)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, not {v!r}")
    if not 1 <= flank <= MAX_FLANK:
        raise ValueError(f"meth_flank must be in 1..{MAX_FLANK}, not {flank!r}")
    if not 1 <= bin_len <= flank:
        raise ValueError(f"meth_bin must be in 1..meth_flank, not {bin_len!r}")
    if n_bins(flank, bin_len) > MAX_BINS:
        raise ValueError(f"meth_flank / meth_bin gives more than {MAX_BINS} bins per flank")
    if not 0 <= lo < hi <= 255:
        raise ValueError(f"the call bytes must satisfy 0 <= meth_lo < meth_hi <= 255, not {lo!r}, {hi!r}")
    if not isinstance(mod_code, str) or not re.fullmatch(r"[a-z]|[0-9]+", mod_code):
        raise ValueError(f"meth_mod_code must be one lower-case letter or a ChEBI number, not {mod_code!r}")


def n_bins(flank, bin_len):
    return (flank + bin_len - 1) // bin_len


def stored_tract(read):
    """The tract of a placed read in the coordinates of its stored sequence: the oriented interval between the anchors
    (core_seq_start_pos + left_buffer_len, core_seq_end_pos - right_buffer_len), mirrored with full_read_len on strand
    `-`; an inverted interval (anchors that overlap) is empty at the lower of its two ends."""
    n = read.full_read_len
    lo, hi = read.core_seq_start_pos + read.left_buffer_len, read.core_seq_end_pos - read.right_buffer_len
    if read.strand == "-":
        lo, hi = n - hi, n - lo
    lo, hi = max(0, min(lo, n)), max(0, min(hi, n))
    if hi < lo:
        lo = hi
    return lo, hi


class ReadMethylation:
    """One read's status, strand and counters: `counts` int64 [2 nb + 1][5] ordered by the reference (left bins from
    the farthest to the nearest, the tract, right bins from the nearest to the farthest), None unless status is OK."""

    def __init__(self, status, strand, counts=None):
        self.status, self.strand, self.counts = status, strand, counts

    def totals(self):
        """(tract, left flank, right flank), each the five counters, or None."""
        if self.counts is None:
            return None
        nb = (len(self.counts) - 1) // 2
        return self.counts[nb], self.counts[:nb].sum(axis=0), self.counts[nb + 1:].sum(axis=0)


def frac_text(c):
    d = int(c[METH]) + int(c[UNMETH])
    return f"{int(c[METH]) / d:.4f}" if d else "-"


def mean_text(c):
    called = int(c[CALLED])
    return f"{(int(c[SUM]) + called / 2) / (256 * called):.4f}" if called else "-"


def _fields(c):
    if c is None:
        return ["-"] * 6
    return [str(int(c[SITES])), str(int(c[CALLED])), str(int(c[METH])), str(int(c[UNMETH])), frac_text(c), mean_text(c)]


def methylation_regions(repeat_regions, reads_by_region, tags_by_region, flank=2000, bin_len=200, hi=192, lo=63,
                        mod_code="m", device=0, engine=None, stream=None):
    """The methylation counters of every read with a round-3 size in every region, in one call of `engine` (default
    _capi.read_methylation; tests pass a restatement with the same signature).  reads_by_region: one {read_name: stored
    sequence} per region (a placed read has at most 4 000 000 bases: upstream.MAX_READ_LEN); tags_by_region: one
    {read_name: (mm_text, ml_bytes, stored_reversed, usable)} per region.  Reads whose tags do not decode get a status other than OK and never reach the engine; one NOTICE counts them.
    Sets `region.read_methylation` = {read_name: ReadMethylation} and `region.methylation_bins` = (flank, bin) and
    returns the regions."""
    check_options(flank, bin_len, hi, lo, mod_code)
    if engine is None:
        from . import _capi
        engine = _capi.read_methylation
    nb = n_bins(flank, bin_len)
    seqs, mods, flags, tract_lo, tract_hi, owners = [], [], [], [], [], []
    for region, reads, tags in zip(repeat_regions, reads_by_region, tags_by_region):
        region.read_methylation = {}
        region.methylation_bins = (flank, bin_len)
        for name, read in region.read_dict.items():
            if read.round3_repeat_size is None:
                continue
            status, deltas, probs, bits = decode_read_tags((tags or {}).get(name), mod_code)
            region.read_methylation[name] = ReadMethylation(status, read.strand)
            if status != OK:
                continue
            a, b = stored_tract(read)
            seqs.append(reads[name].strip()); mods.append((deltas, probs)); flags.append(bits)
            tract_lo.append(a); tract_hi.append(b)
            owners.append((region, name))
    if seqs:
        out = engine(seqs, mods, np.array(flags, np.uint8), np.array(tract_lo, np.int32), np.array(tract_hi, np.int32),
                     flank=flank, bin=bin_len, lo_byte=lo, hi_byte=hi, device=device)
        counts = np.asarray(out["counts"]).reshape(len(seqs), 2 * nb + 1, 5)
        for i, (region, name) in enumerate(owners):
            rm = region.read_methylation[name]
            if int(out["status"][i]) == DEVICE_BAD_TAG:
                rm.status = BAD_TAG
                continue
            c = counts[i].astype(np.int64)
            before, tract, after = c[:nb], c[nb:nb + 1], c[nb + 1:]
            if rm.strand == "-":          # stored "before" is the reference's right side
                before, after = after, before
            rm.counts = np.concatenate([before[::-1], tract, after])
    report_undecoded_reads(repeat_regions, stream)
    return repeat_regions


def report_undecoded_reads(repeat_regions, stream=None):
    """One NOTICE counting the reads with a size by status other than OK (none: no NOTICE).  Returns the counts."""
    tally = {}
    for region in repeat_regions:
        for rm in (getattr(region, "read_methylation", None) or {}).values():
            if rm.status != OK:
                tally[rm.status] = tally.get(rm.status, 0) + 1
    if tally:
        text = ", ".join(f"{k} {tally[k]}" for k in (NO_TAG, NO_MOD, BAD_TAG, CLIPPED) if k in tally)
        print(f"NOTICE: methylation: {sum(tally.values())} read(s) with a size have no usable calls ({text})",
              file=stream or sys.stderr)
    return tally


def read_methylation_text(region):
    head = "\t".join(f"{s}_{f}" for s in ("Tract", "Left", "Right")
                     for f in ("CpG", "Called", "Meth", "Unmeth", "Frac", "Mean"))
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "#Read_Name\tAllele_ID\tRepeat_Size\tStrand\tStatus\t" + head + "\n"]
    rms = getattr(region, "read_methylation", None) or {}
    for name, allele in _ordered_reads(region):
        rm = rms[name]
        totals = rm.totals() or (None, None, None)
        size = region.read_dict[name].round3_repeat_size
        lines.append("\t".join([name, allele, f"{size:.1f}", rm.strand, rm.status] +
                               [x for t in totals for x in _fields(t)]) + "\n")
    return "".join(lines)


def allele_methylation(region):
    """Per allele, in phasing order: (id, reads with status OK, counts int64 [2 nb + 1][5] summed over them, reads with
    a called site per segment [2 nb + 1])."""
    res = phasing.results_of(region)
    rms = getattr(region, "read_methylation", None) or {}
    flank, bin_len = getattr(region, "methylation_bins", (1, 1))
    rows = 2 * n_bins(flank, bin_len) + 1
    out = []
    for label in range(1, len(res.quantified_allele_list) + 1):
        got = [rms[n].counts for n, q in res.quantified_read_dict.items()
               if q.allele_id == label and n in rms and rms[n].counts is not None]
        total = np.sum(got, axis=0) if got else np.zeros((rows, 5), np.int64)
        reads = np.sum([c[:, CALLED] > 0 for c in got], axis=0) if got else np.zeros(rows, np.int64)
        out.append((label, len(got), total, reads))
    return out


def segment_names(flank, bin_len):
    """[(segment, dist_from, dist_to)] in file order: left bins from the farthest, TRACT, right bins from the nearest."""
    nb = n_bins(flank, bin_len)
    bins = [(k * bin_len, min((k + 1) * bin_len, flank)) for k in range(nb)]
    return ([("LEFT", str(a), str(b)) for a, b in bins[::-1]] + [("TRACT", "-", "-")] +
            [("RIGHT", str(a), str(b)) for a, b in bins])


def allele_methylation_text(region):
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Motif={region.repeat_unit_seq}\n",
             "#Allele_ID\tSegment\tDist_From\tDist_To\tReads\tCpG\tCalled\tMeth\tUnmeth\tFrac\tMean\n"]
    names = segment_names(*getattr(region, "methylation_bins", (1, 1)))
    for label, _, total, reads in allele_methylation(region):
        for k, (seg, a, b) in enumerate(names):
            lines.append("\t".join([str(label), seg, a, b, str(int(reads[k]))] + _fields(total[k])) + "\n")
    return "".join(lines)


def _write(region, suffix, text):
    if region.no_details or not region.out_prefix:
        return None
    path = f"{region.out_prefix}.{suffix}"
    with open(path, "w") as f:
        f.write(text(region))
    return path


def write_read_methylation(region):
    """`<region out_prefix>.read_methylation.tsv` (not with no_details)."""
    return _write(region, "read_methylation.tsv", read_methylation_text)


def write_allele_methylation(region):
    """`<region out_prefix>.allele_methylation.tsv` (not with no_details)."""
    return _write(region, "allele_methylation.tsv", allele_methylation_text)


def methylation_summary_row(region):
    rms = getattr(region, "read_methylation", None) or {}
    alleles = allele_methylation(region) if rms else []
    n_alleles = len(phasing.results_of(region).quantified_allele_list)
    cells = []
    for label, n, total, _ in alleles:
        nb = (len(total) - 1) // 2
        cells.append(f"{label}:{n}:{frac_text(total[nb])}:{frac_text(total[:nb].sum(axis=0))}:"
                     f"{frac_text(total[nb + 1:].sum(axis=0))}")
    with_calls = sum(rm.status == OK for rm in rms.values())
    return (f"{region.chrom}\t{max(0, region.start_pos)}\t{region.end_pos}\t{region.repeat_unit_seq}\t{n_alleles}\t"
            f"{with_calls}\t{len(rms) - with_calls}\t{'|'.join(cells) or '-'}\n")


def write_methylation_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_methylation.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_methylation.tsv"
    with open(path, "w") as f:
        f.write("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tReads_With_Calls\tReads_Without\tAllele_Methylation\n")
        f.write("".join(methylation_summary_row(region) for region in regions))
    return path
