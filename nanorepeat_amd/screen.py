"""Reads of a FASTQ / FASTA file -> the reads each repeat region sees, without a genome mapper.

The reference maps every read to the whole genome (preprocess_fastq, nanoRepeat.py:41-76) and then fetches the reads
overlapping each region +- anchor_len from the BAM (nanoRepeat_bam.py:577-600), in front of the anchor check that
really decides (find_anchor_locations_in_reads).  Here that coarse prefilter is an anchor k-mer screen on the GPU
(nra_screen_*): a read is offered to a region when enough of its k-mers are in each of the
region's two anchors.  Reads are assigned by their anchors, not by a genome-wide mapping.
"""
import sys

from . import _capi, io as nr_io


class Screen:
    """One nra_screen handle: the anchor index of a set of regions, on one device.  `anchors` = [(left, right)]."""

    def __init__(self, anchors, k=15, max_occ=16, device=0):
        self.n_regions = len(anchors)
        self._h = _capi.screen_create(anchors, k=k, max_occ=max_occ, device=device)

    def screen_reads(self, seqs, min_hits=4):
        """-> dict(read, region, hits_left, hits_right) of the passing pairs, sorted by read then region."""
        return _capi.screen_reads(self._h, seqs, min_hits)

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


def reads_by_region(path, regions, k=15, max_occ=16, min_hits=4, chunk_bases=1 << 28, device=0, screener=None):
    """Streams `path` (FASTQ / FASTA, gzip-aware) through the anchor screen of `regions` (anchors set by
    io.extract_ref_sequence).  Returns one {name: (seq, qual)} per region, in file order; qual is None for FASTA.
    Only passing reads are kept.  `screener`: a stand-in for Screen with the same constructor and screen_reads."""
    factory = screener or Screen
    per_region = [dict() for _ in regions]
    if not regions:
        return per_region
    anchors = [(r.left_anchor_seq or "", r.right_anchor_seq or "") for r in regions]
    with factory(anchors, k=k, max_occ=max_occ, device=device) as scr:
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
            got = scr.screen_reads(seqs, min_hits)
            for r, g in zip(got["read"].tolist(), got["region"].tolist()):
                _keep(per_region, g, names[r], seqs[r], quals[r])
    return per_region


def all_reads_by_region(path, n_regions, chunk_bases=1 << 28):
    """Every non-empty read offered to every region (no screen): the exhaustive form, exact and slow."""
    per_region = [dict() for _ in range(n_regions)]
    for names, seqs, quals in nr_io.iter_reads(path, chunk_bases):
        for name, seq, qual in zip(names, seqs, quals):
            if seq:
                for g in range(n_regions):
                    _keep(per_region, g, name, seq, qual)
    return per_region
