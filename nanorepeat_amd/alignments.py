"""The round-3 alignment file: for every read with a round-3 size of its own, the alignment of its core to the
template it was called at, as one PAF row of `<region>.round3.paf`.

The reference leaves the aligner's PAF of every round behind; here round 3 exchanges integers, so the one alignment
a user wants to look at -- the read against the template of its size -- is computed once more with its path, for
all reads of all regions in one chunked nra_align_paths call.  The template is left anchor + unit * k + right anchor
with k the smallest candidate that holds the read's best round-3 score."""
import sys

from . import _capi, paf, structure

MAX_QUERY = _capi.PATHS_MAX_QUERY
MAX_TARGET = _capi.PATHS_MAX_TARGET
MAX_TRACE = _capi.PATHS_MAX_TRACE


def smallest_best_k(kmin, cand_score, best_score):
    """The smallest candidate k whose score is the read's best one; None when no candidate holds it."""
    for i, s in enumerate(cand_score):
        if int(s) == int(best_score):
            return int(kmin) + i
    return None


def keep_candidates(read, kmin, cand_score):
    """What round 3 leaves on a read for this file: its window's first k and its candidate scores."""
    read.round3_candidates = (int(kmin), [int(s) for s in cand_score])


def template_of(region, k):
    return region.left_anchor_seq + region.repeat_unit_seq * k + region.right_anchor_seq


def _ok_reads(region):
    """The READ_OK reads of a region in phased_reads.txt order: [(name, k)]."""
    out = []
    for name, _ in structure._ordered_reads(region):
        read = region.read_dict[name]
        cand = getattr(read, "round3_candidates", None)
        if read.round3_status != _capi.READ_OK or cand is None:
            continue
        k = smallest_best_k(cand[0], cand[1], read.round3_best_score)
        if k is not None:
            out.append((name, k))
    return out


def alignment_regions(repeat_regions, device=0, scoring=None, engine=None):
    """Fills region.round3_alignments = [(read name, k, core, template length, result dict)] in file order, and
    region.round3_alignments_left_out = {read name: reason} for the pairs beyond nra_align_paths' limits.
    `engine` stands in for _capi.align_paths_chunked (tests)."""
    engine = engine or _capi.align_paths_chunked
    seqs, index, pq, pt, owners = [], {}, [], [], []

    def seq_id(s):
        if s not in index:
            index[s] = len(seqs)
            seqs.append(s)
        return index[s]

    for region in repeat_regions:
        region.round3_alignments, region.round3_alignments_left_out = [], {}
        flank = len(region.left_anchor_seq) + len(region.right_anchor_seq)
        for name, k in _ok_reads(region):
            core = region.read_core_seq_dict[name].strip()
            tlen = flank + len(region.repeat_unit_seq) * k
            if len(core) > MAX_QUERY or tlen > MAX_TARGET or len(core) * tlen > MAX_TRACE:
                region.round3_alignments_left_out[name] = "core, template or their trace beyond the path call's limits"
                continue
            pq.append(seq_id(core)); pt.append(seq_id(template_of(region, k)))
            owners.append((region, name, k, core, tlen))
    if not owners:
        return repeat_regions
    out = engine(seqs, pq, pt, sc=scoring, device=device)
    for i, (region, name, k, core, tlen) in enumerate(owners):
        res = {key: int(out[key][i]) for key in ("score", "tstart", "tend", "qstart", "qend")}
        res["cigar"] = out["cigar"][i]
        region.round3_alignments.append((name, k, core, tlen, res))
    return repeat_regions


def alignment_text(region):
    """The rows of `<region>.round3.paf`.  A read whose alignment came back without a record (a score below
    min_dp_score cannot be a read's best score) has no row."""
    lines = []
    for name, k, core, tlen, r in getattr(region, "round3_alignments", None) or []:
        if r["score"] < 0:
            continue
        size = region.read_dict[name].round3_repeat_size
        lines.append(paf.format_paf_line(name, len(core), r["qstart"], r["qend"], "+", f"{region.to_unique_id()}|k={k}",
                                         tlen, r["tstart"], r["tend"], r["score"], r["cigar"]) + f"\trs:f:{size:.1f}\n")
    return "".join(lines)


def write_read_alignments(region):
    if region.no_details or not region.out_prefix:
        return
    with open(f"{region.out_prefix}.round3.paf", "w") as f:
        f.write(alignment_text(region))


def report_left_out_reads(repeat_regions, stream=None):
    """One NOTICE per region that left reads out of its alignment file.  Returns the number of such reads."""
    stream = stream or sys.stderr
    total = 0
    for region in repeat_regions:
        left = getattr(region, "round3_alignments_left_out", None) or {}
        if left:
            total += len(left)
            some = ", ".join(list(left)[:5]) + (" ..." if len(left) > 5 else "")
            print(f"NOTICE: {region.to_unique_id()}: {len(left)} read(s) beyond the path call's limits have no row in "
                  f"the round-3 alignment file ({some})", file=stream)
    return total
