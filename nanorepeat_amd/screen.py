"""Reads of a FASTQ / FASTA file -> the reads each repeat region sees, without a genome mapper.

The reference maps every read to the whole genome (preprocess_fastq, nanoRepeat.py:41-76) and then fetches the reads
overlapping each region +- anchor_len from the BAM (nanoRepeat_bam.py:577-600), in front of the anchor check that
really decides (find_anchor_locations_in_reads).  Here that coarse prefilter is an anchor k-mer screen on the GPU
(nra_screen_*): a read is offered to a region when enough of its k-mers are in each of the
region's two anchors.  Reads are assigned by their anchors, not by a genome-wide mapping.

With `partial=True` the motif screen (nra_screen_reads_partial) also offers, as candidates, the
reads that carry one anchor only and the reads made of a region's motif.
"""
import sys

import numpy as np

from . import _capi, io as nr_io


class Screen:
    """One nra_screen handle: the anchor index of a set of regions, on one device.  `anchors` = [(left, right)];
    `motifs` = one repeat motif per region, for screen_reads_partial's in-repeat pairs."""

    def __init__(self, anchors, k=15, max_occ=16, device=0, motifs=None):
        self.n_regions = len(anchors)
        self._h = _capi.screen_create(anchors, k=k, max_occ=max_occ, device=device)
        if motifs is not None:
            try:
                self.set_motifs(motifs)
            except Exception:
                self.close()
                raise

    def set_motifs(self, motifs):
        _capi.screen_set_motifs(self._h, motifs)

    def screen_reads(self, seqs, min_hits=4):
        """-> dict(read, region, hits_left, hits_right) of the passing pairs, sorted by read then region."""
        return _capi.screen_reads(self._h, seqs, min_hits)

    def screen_reads_partial(self, seqs, min_hits=4, motif_share_pct=5):
        """-> dict(read, region, hits_left, hits_right, motif_windows, kind) of the pairs of kind 0 (both anchors),
        1 (left only), 2 (right only) and 3 (in repeat), sorted by read then region."""
        return _capi.screen_reads_partial(self._h, seqs, min_hits, motif_share_pct)

    def stats(self):
        return _capi.screen_stats(self._h)

    def close(self):
        if self._h:
            _capi.screen_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _keep(per_region, g, name, seq, qual):
    """First record of a name wins in a region, as extract_fastq_from_bam writes each name once."""
    if name not in per_region[g]:
        per_region[g][name] = (seq, qual)


KIND_SPANNING, KIND_LEFT, KIND_RIGHT, KIND_IN_REPEAT = 0, 1, 2, 3


def screenable_motif(motif):
    """A region's motif as the motif screen takes it (ACGT in either case, 1..64 bases), else None."""
    m = (motif or "").upper()
    return m if 1 <= len(m) <= 64 and not set(m) - set("ACGT") else None


_COMP = str.maketrans("ACGT", "TGCA")
_CODES = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODES[_c] = _CODES[_c + 32] = _i


def motif_class(motif):
    """The words of the motif's class (the rotations of its root and of the root's reverse complement), or None when
    the root is longer than 6 bases or the motif is not ACGT."""
    m = screenable_motif(motif)
    if m is None:
        return None
    root = next(m[:p] for p in range(1, len(m) + 1) if len(m) % p == 0 and m[:p] * (len(m) // p) == m)
    if len(root) > 6:
        return None
    rc = root.translate(_COMP)[::-1]
    return {w[i:] + w[:i] for w in (root, rc) for i in range(len(root))}


def _runs_of(flags, width):
    """For every start i: flags[i:i + width] all true."""
    c = np.concatenate(([0], np.cumsum(~flags)))
    return (c[width:] - c[:-width]) == 0


def class_windows(seq, motif, k=15):
    """m(r, C) of the motif screen's contract for one read and the class of `motif`, computed on the host: the window
    positions whose k bases are ACGT, whose smallest period p in 1..6 is the root's length and whose first p bases are
    a word of the class.  The exhaustive form (screen=False) applies the in-repeat rule with it."""
    words = motif_class(motif)
    codes = _CODES[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)]
    n = len(codes) - k + 1
    if words is None or n <= 0:
        return 0
    p = len(next(iter(words)))
    ok = _runs_of(codes != 255, k)
    ok &= _runs_of(codes[:-p] == codes[p:], k - p)[:n]
    for q in range(1, p):
        ok &= ~_runs_of(codes[:-q] == codes[q:], k - q)[:n]
    first = np.zeros(n, np.int64)
    for j in range(p):
        first = first * 4 + (codes[j:j + n] & 3)
    table = np.zeros(4 ** p, bool)
    for w in words:
        table[sum("ACGT".index(ch) * 4 ** (p - 1 - j) for j, ch in enumerate(w))] = True
    return int((ok & table[first]).sum())


def in_repeat_rule(seq, motif, k=15, min_hits=4, motif_share_pct=5):
    """Kind 3's count rule for one read and one motif: m >= max(min_hits, ceil(motif_share_pct * W / 100)), W >= 1."""
    w = max(0, len(seq) - k + 1)
    return w >= 1 and class_windows(seq, motif, k) >= max(max(1, min_hits), -(-motif_share_pct * w // 100))


def _keep_candidate(candidates, g, name, seq, qual, kind):
    if name not in candidates[g]:
        candidates[g][name] = (seq, qual, kind)


def reads_by_region(path, regions, k=15, max_occ=16, min_hits=4, chunk_bases=1 << 28, device=0, screener=None,
                    partial=False, motif_share_pct=5):
    """Streams `path` (FASTQ / FASTA, gzip-aware) through the anchor screen of `regions` (anchors set by
    io.extract_ref_sequence).  Returns one {name: (seq, qual)} per region, in file order; qual is None for FASTA.
    Only passing reads are kept.  `screener`: a stand-in for Screen with the same constructor and screen_reads.

    partial=True: returns (per_region, candidates).  per_region is the same as without it; candidates[g] =
    {name: (seq, qual, kind)} holds the reads with one anchor only (kind 1 left, 2 right) and the reads made of the
    region's motif (kind 3).  A region whose motif the motif screen cannot take (screenable_motif) has no kind 3."""
    factory = screener or Screen
    per_region = [dict() for _ in regions]
    candidates = [dict() for _ in regions]
    if not regions:
        return (per_region, candidates) if partial else per_region
    anchors = [(r.left_anchor_seq or "", r.right_anchor_seq or "") for r in regions]
    more = {}
    if partial:
        # a motif the screen cannot take stands in as a 7-base primitive word: it has no class
        more["motifs"] = [screenable_motif(r.repeat_unit_seq) or "AAAAAAC" for r in regions]
    with factory(anchors, k=k, max_occ=max_occ, device=device, **more) as scr:
        stats = scr.stats()
        if stats.get("n_empty_regions"):
            print(f"NOTICE: {stats['n_empty_regions']} region(s) have no anchor k-mer left to screen with (periodic, "
                  f"shared by more than {max_occ} anchors, or too short): every read is offered to them",
                  file=sys.stderr)
        for names, seqs, quals in nr_io.iter_reads(path, chunk_bases):
            keep = [i for i, s in enumerate(seqs) if s]
            if len(keep) != len(seqs):
                names, seqs, quals = [names[i] for i in keep], [seqs[i] for i in keep], [quals[i] for i in keep]
            if not seqs:
                continue
            if partial:
                got = scr.screen_reads_partial(seqs, min_hits, motif_share_pct)
                for r, g, kd in zip(got["read"].tolist(), got["region"].tolist(), got["kind"].tolist()):
                    if kd == KIND_SPANNING:
                        _keep(per_region, g, names[r], seqs[r], quals[r])
                    else:
                        _keep_candidate(candidates, g, names[r], seqs[r], quals[r], kd)
                continue
            got = scr.screen_reads(seqs, min_hits)
            for r, g in zip(got["read"].tolist(), got["region"].tolist()):
                _keep(per_region, g, names[r], seqs[r], quals[r])
    return (per_region, candidates) if partial else per_region


def all_reads_by_region(path, n_regions, chunk_bases=1 << 28, partial=False):
    """Every non-empty read offered to every region (no screen): the exhaustive form, exact and slow.
    partial=True: returns (per_region, candidates), every read also a candidate (kind None) of every region."""
    per_region = [dict() for _ in range(n_regions)]
    for names, seqs, quals in nr_io.iter_reads(path, chunk_bases):
        for name, seq, qual in zip(names, seqs, quals):
            if seq:
                for g in range(n_regions):
                    _keep(per_region, g, name, seq, qual)
    if partial:
        return per_region, [{n: (s, q, None) for n, (s, q) in d.items()} for d in per_region]
    return per_region
