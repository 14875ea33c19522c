"""One-anchor reads without a GPU: the two restatements of the extension contract against each other, hand cases, the
classification of reads in upstream, the BAM command with partial_reads=True on a panel with a long allele that no read
spans (restatement as engine, oracle as aligner and scorer), and the argument checks of nra_extend_tracts."""
import ctypes as C
import struct
import sys
import zlib

import numpy as np
import pytest

from nanorepeat_amd import bam as B, partial, synth, upstream as U, round3 as R3
from extend_ref import plain_extend, numpy_extend_same_p, ref_extend_tracts

KINDS = ("pure", "interrupted", "ont", "hifi", "random", "n", "lower")


def _motif(rng, p):
    return synth.rand_unit(rng, p) if p > 1 else "ACGT"[int(rng.integers(0, 4))]


def _tract(rng, u, kind, n_units):
    """The tract kinds of test_structure_gpu.py."""
    p = len(u)
    phase = int(rng.integers(0, p))
    pure = (u * (n_units + 2))[phase:phase + n_units * p + int(rng.integers(0, p))]
    if kind == "pure":
        return pure
    if kind == "interrupted":
        s = pure
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + synth.rand_seq(rng, int(rng.integers(1, p + 3))) + s[at:]
        return s
    if kind in ("ont", "hifi"):
        return synth.apply_errors(rng, pure, kind)
    if kind == "random":
        return synth.rand_seq(rng, len(pure))
    if kind == "n":
        s = list(synth.apply_errors(rng, pure, "ont"))
        for _ in range(max(1, len(s) // 50)):
            if s:
                s[int(rng.integers(0, len(s)))] = "NRY-"[int(rng.integers(0, 4))]
        return "".join(s)
    if kind == "lower":
        s = synth.apply_errors(rng, pure, "hifi")
        return s.lower() if rng.random() < 0.5 else s[:len(s) // 2].lower() + s[len(s) // 2:]
    raise ValueError(kind)


SCORES = ((2, 4, 6), (1, 0, 1), (3, 2, 127), (127, 127, 5), (5, 7, 3))


# ---------------------------------------------------------------------------- the contract
@pytest.mark.parametrize("seed", [1, 2])
def test_numpy_form_equals_closed_form(seed):
    rng = np.random.default_rng(seed)
    n = 0
    for p in (1, 2, 3, 4, 5, 6, 7, 8, 11, 16, 17, 31, 32, 33, 64):
        u = _motif(rng, p)
        tracts = []
        for i, kind in enumerate(KINDS * 2):
            t = _tract(rng, u, kind, int(rng.integers(0, max(2, 160 // p))))
            if i % 3 == 0:
                t += synth.rand_seq(rng, int(rng.integers(0, 60)))          # the repeat ends, other sequence follows
            tracts.append(t)
        tracts += ["", u[0], u[:2], "N", "n" + u[0].lower()]
        for a, b, g in SCORES[:3] if p > 8 else SCORES:
            got = numpy_extend_same_p(tracts, [u] * len(tracts), a, b, g)
            for i, t in enumerate(tracts):
                assert tuple(int(x[i]) for x in got) == plain_extend(t, u, a, b, g), (u, t, (a, b, g))
                n += 1
    assert n > 700
    mixed = ref_extend_tracts(["CAG", "TATTG"], ["CAGCAGCA", "TATTGTAT", "cagcag"], [0, 1, 0])
    plain = ref_extend_tracts(["CAG", "TATTG"], ["CAGCAGCA", "TATTGTAT", "cagcag"], [0, 1, 0], vectorised=False)
    for k in mixed:
        assert np.array_equal(mixed[k], plain[k]) and mixed[k].dtype == np.int32


def test_hand_cases():
    # a pure prefix of L bases, from any start phase: every base matches, the best cell is the last row
    for u, a in (("CAG", 2), ("TATTG", 3), ("A", 1), ("GGCCCC", 2)):
        p = len(u)
        for phase in range(p):
            for L in (p, 4 * p + 2, 61):                  # from p bases on only one start phase fits a primitive motif
                s = (u * (L // p + 3))[phase:phase + L]
                assert plain_extend(s, u, a, 4, 6) == (a * L, L, (phase + L) % p, L), (u, phase, L)
    # the repeat ends and other sequence follows: the extension stops where the score peaks
    assert plain_extend("CAG" * 10 + "TTTTTTTTTT", "CAG") == (60, 30, 0, 30)
    # only mismatching bases: nothing is positive
    assert plain_extend("TTTTTT", "CAG") == (0, 0, 0, 0)
    assert plain_extend("", "CAG") == (0, 0, 0, 0)
    assert plain_extend("NNNN", "A") == (0, 0, 0, 0)
    # lower case is upper-cased first; N mismatches every motif base
    assert plain_extend("cagcagcag", "CAG") == plain_extend("CAGCAGCAG", "CAG") == (18, 9, 0, 9)
    assert plain_extend("CAGCAGNAGCAGCAG", "CAG") == (2 * 14 - 4, 15, 0, 15)
    # a lost base: one motif base deleted, the count goes on (14 read bases show 15 motif bases)
    assert plain_extend("CAGCAG" + "CG" + "CAGCAG", "CAG") == (2 * 14 - 6, 14, 0, 15)
    # an extra base: an insertion, the count does not move
    assert plain_extend("CAGCAG" + "T" + "CAGCAGCAG", "CAG") == (2 * 15 - 6, 16, 0, 15)
    # a tie between two rows keeps the first: -4 then +2 +2 comes back to 6 at row 6, row 3 already had it
    assert plain_extend("CAGTAG", "CAG")[:2] == (6, 3)


# ---------------------------------------------------------------------------- classification
def _region():
    rr = R3.RepeatRegion("chr1\t1000\t1030\tCAG")
    rr.left_anchor_seq, rr.right_anchor_seq = "A" * 400, "C" * 400
    return rr


def _hit(name, side, score, qs, qe, strand="+", length=None):
    return U.AnchorHit(name, 3000, qs, qe, strand, side + "_anchor", score, length if length is not None else qe - qs)


def test_upstream_keeps_one_anchor_reads_and_nothing_else_changes():
    cases = {
        "placed": [_hit("placed", "left", 700, 100, 500), _hit("placed", "right", 690, 560, 960)],
        "left_only": [_hit("left_only", "left", 700, 2200, 2600)],
        "right_only": [_hit("right_only", "right", 650, 300, 700, "-")],
        # the best left hit beats its runner-up 1.5-fold: the side passes with two hits
        "left_two_hits": [_hit("left_two_hits", "left", 700, 10, 410), _hit("left_two_hits", "left", 100, 900, 960, "-")],
        # the other side has hits that fail the check: ambiguous, not a partial read
        "ambiguous_other": [_hit("ambiguous_other", "left", 700, 100, 500),
                            _hit("ambiguous_other", "right", 300, 560, 960), _hit("ambiguous_other", "right", 290, 40, 90, "-")],
        # its own side fails the check
        "ambiguous_own": [_hit("ambiguous_own", "left", 300, 100, 500), _hit("ambiguous_own", "left", 290, 700, 1100, "-")],
        # two good anchors in the wrong order
        "order_failed": [_hit("order_failed", "left", 700, 600, 1000), _hit("order_failed", "right", 690, 100, 500)],
        "no_hits": [],
    }
    rr, plain = _region(), _region()
    for hits in cases.values():
        U.find_anchor_locations_for1read(hits, rr)
    assert list(rr.read_dict) == ["placed"]
    kept = rr.one_anchor_reads
    assert sorted(kept) == ["left_only", "left_two_hits", "right_only"]
    assert kept["left_only"][0] == "left" and kept["left_only"][1] is cases["left_only"][0]
    assert kept["right_only"][0] == "right" and kept["right_only"][1].strand == "-"
    assert kept["left_two_hits"][1].align_score == 700
    # what a region holds for the placed read does not depend on the other reads having been seen
    U.find_anchor_locations_for1read(cases["placed"], plain)
    assert not hasattr(plain, "one_anchor_reads")
    assert vars(plain.read_dict["placed"]) == vars(rr.read_dict["placed"])


def test_tails_and_motifs_by_anchor_and_strand():
    flank_l, flank_r = "ACGTTGCAAC", "GGATCCATAG"
    calls = []

    def engine(motifs, tracts, read_motif, **kw):
        calls.append((list(motifs), list(tracts), list(read_motif), kw))
        return ref_extend_tracts(motifs, tracts, read_motif, **kw)

    rr = _region()
    left_read = flank_l + "CAG" * 7 + "CA"                       # ends inside the tract
    right_read = "G" + "CAG" * 5 + flank_r                        # starts inside the tract
    reads = {"l+": left_read, "l-": U.rev_comp(left_read), "r+": right_read, "r-": U.rev_comp(right_read)}
    rr.one_anchor_reads = {"l+": ("left", _hit("l+", "left", 20, 0, 10)), "l-": ("left", _hit("l-", "left", 20, 0, 10, "-")),
                           "r+": ("right", _hit("r+", "right", 20, 16, 26)),
                           "r-": ("right", _hit("r-", "right", 20, 16, 26, "-"))}

    class Sized:
        round3_repeat_size = 6.0

    rr.read_dict = {"s": Sized()}
    partial.partial_regions([rr], [reads], engine=engine)
    motifs, tracts, rm, kw = calls[0]
    assert kw == dict(match=2, mismatch=4, gap=6, device=0)
    assert [motifs[i] for i in rm] == ["CAG", "CAG", "GAC", "GAC"]
    assert tracts == ["CAG" * 7 + "CA"] * 2 + [("G" + "CAG" * 5)[::-1]] * 2
    pr = rr.partial_reads
    assert [pr[n].fields() for n in ("l+", "l-")] == [["left", "+", "23", "23", "23", "7", "46", "1"],
                                                      ["left", "-", "23", "23", "23", "7", "46", "1"]]
    assert pr["r+"].fields() == ["right", "+", "16", "16", "16", "5", "32", "0"]       # 5 is not above 6.0
    assert partial.region_counts(rr) == (1, 6.0, 2, 2, 7, 2)
    assert partial.partial_summary_row(rr) == "chr1\t1000\t1030\tCAG\t1\t6.0\t2\t2\t7\t2\n"
    lines = partial.partial_reads_text(rr).split("\n")
    assert [l.split("\t")[0] for l in lines[3:7]] == ["l+", "l-", "r+", "r-"]          # size descending, then name
    # without a spanning read every read that shows a unit exceeds
    rr.read_dict = {}
    partial.partial_regions([rr], [reads], engine=engine)
    assert partial.region_counts(rr) == (0, None, 2, 2, 7, 4)
    # the scoring in use sets the scores: a one-base gap costs gap_open1 + gap_ext1

    class Scoring:
        match, mismatch, gap_open1, gap_ext1 = 3, 5, 4, 3

    partial.partial_regions([rr], [reads], scoring=Scoring, engine=engine)
    assert calls[-1][3] == dict(match=3, mismatch=5, gap=7, device=0)


def test_unsupported_motif_and_over_long_tail_get_dash_fields():
    rr = _region()
    rr.repeat_unit_seq = "CAGN"
    rr.one_anchor_reads = {"a": ("left", _hit("a", "left", 20, 0, 4))}
    calls = []
    partial.partial_regions([rr], [{"a": "ACGTCAGCAG"}], engine=lambda *a, **k: calls.append(a))
    assert not calls and rr.partial_reads["a"].fields() == ["left", "+", "6", "-", "-", "-", "-", "-"]
    assert partial.region_counts(rr) == (0, None, 1, 0, None, 0)
    rr.repeat_unit_seq = "CAG"
    partial.partial_regions([rr], [{"a": "ACGT" + "CAG" * 66667}], engine=lambda *a, **k: calls.append(a))
    assert not calls and rr.partial_reads["a"].fields()[2:4] == ["200001", "-"]


# ---------------------------------------------------------------------------- a tiny BAM writer (as tests/test_bam.py)
def _bgzf_block(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    bsize = 12 + 6 + len(data) + 8 - 1
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) +
            data + struct.pack("<II", zlib.crc32(payload), len(payload)))


def _record(name, seq, quals, tid, pos, ref_len, flag=0):
    cigar = [(ref_len << 4) | 0] if ref_len and seq else []
    codes = [B._SEQ_CODES.index(c) for c in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    q = bytes(quals) if quals is not None else b"\xff" * len(seq)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 60, 0, len(cigar), flag, len(seq), -1, -1, 0)
    body += name.encode() + b"\x00" + b"".join(struct.pack("<I", c) for c in cigar) + packed + q
    return struct.pack("<i", len(body)) + body


def write_bam(path, refs, records, block=3000):
    """records: (name, seq, quals, ref name, pos, end) sorted by (ref, pos); writes `path` and a linear `path`.bai."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(f"@SQ\tSN:{n}\tLN:{l}\n".encode() for n, l in refs)
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", l)
    names = [n for n, _ in refs]
    chunks, starts, upos = [head], [], len(head)
    for name, seq, quals, ref, pos, end in records:
        starts.append(upos)
        rec = _record(name, seq, quals, names.index(ref), pos, end - pos)
        chunks.append(rec); upos += len(rec)
    raw = b"".join(chunks)
    blocks, block_at, coff = [], {}, 0
    for u in range(0, len(raw), block):
        block_at[u] = coff
        bl = _bgzf_block(raw[u:u + block]); blocks.append(bl); coff += len(bl)
    blocks.append(_bgzf_block(b""))
    with open(path, "wb") as f:
        f.write(b"".join(blocks))
    linear = [[] for _ in refs]
    for (name, seq, quals, ref, pos, end), u in zip(records, starts):
        v = (block_at[u - u % block] << 16) | (u % block)
        iv = linear[names.index(ref)]
        for w in range(pos >> 14, (max(end, pos + 1) - 1 >> 14) + 1):
            while len(iv) <= w:
                iv.append(0)
            if iv[w] == 0:
                iv[w] = v
    with open(path + ".bai", "wb") as f:
        f.write(b"BAI\x01" + struct.pack("<i", len(refs)))
        for iv in linear:
            f.write(struct.pack("<i", 0) + struct.pack("<i", len(iv)) + b"".join(struct.pack("<Q", v) for v in iv))


# ---------------------------------------------------------------------------- the panel
LONG_UNITS = 400          # the long allele: 1200 tract bases, more than any read of the panel holds


def partial_panel(tmp_path, seed=5):
    """ref.fa, r.bed, in.bam under tmp_path.  Region 0 (CAG): reads with sequencing errors span a 10-unit allele; a
    400-unit allele is seen only by error-free reads cut inside the tract, 8 anchored left and 8 right, half of each
    stored reverse-complemented.  Region 1 (TATTG): spanning reads of 6 and 17 units and four reads cut inside the
    17-unit tract after 6 units.  Region 2 has no reads.  Returns {read name: tract bases L} of the cut reads."""
    rng = np.random.default_rng(seed)
    chrom = synth.rand_seq(rng, 1500)
    s1 = len(chrom); chrom += "CAG" * 12; e1 = len(chrom); chrom += synth.rand_seq(rng, 1400)
    s2 = len(chrom); chrom += "TATTG" * 8; e2 = len(chrom); chrom += synth.rand_seq(rng, 1500)
    s3 = len(chrom); chrom += "GGCCCC" * 5; e3 = len(chrom); chrom += synth.rand_seq(rng, 900)
    (tmp_path / "ref.fa").write_text(">chr7\n" + "\n".join(chrom[i:i + 80] for i in range(0, len(chrom), 80)) + "\n")
    (tmp_path / "r.bed").write_text(f"chr7\t{s1}\t{e1}\tCAG\nchr7\t{s2}\t{e2}\tTATTG\nchr7\t{s3}\t{e3}\tGGCCCC\n")
    recs, planted = [], {}

    def add(name, seq, pos, end, flip):
        recs.append([name, synth.revcomp(seq) if flip else seq, [30] * len(seq), "chr7", pos, end])

    for g, (st, en, unit, alleles) in enumerate(((s1, e1, "CAG", (10, 10)), (s2, e2, "TATTG", (6, 17)))):
        for i in range(16):
            lo = st - 500 - 7 * i
            s = synth.apply_errors(rng, chrom[lo:st] + unit * alleles[i % 2] + chrom[en:en + 520], "ont_q20")
            add(f"g{g}s{i:02d}", s, lo, en + 520, i % 3 == 0)
    tract = "CAG" * LONG_UNITS
    for i in range(8):
        L = (20, 31, 95, 200, 333, 500, 640, 800)[i]
        lo = s1 - 450 - 11 * i
        add(f"g0l{i}", chrom[lo:s1] + tract[:L], lo, e1, i % 2 == 1)
        planted[f"g0l{i}"] = L
        L += 7
        add(f"g0r{i}", tract[len(tract) - L:] + chrom[e1:e1 + 450 + 11 * i], s1, e1 + 450 + 11 * i, i % 2 == 0)
        planted[f"g0r{i}"] = L
    for i in range(4):
        lo = s2 - 460 - 5 * i
        add(f"g1l{i}", chrom[lo:s2] + "TATTG" * 6 + "TA"[:i % 3], lo, e2, i % 2 == 1)
        planted[f"g1l{i}"] = 30 + len("TA"[:i % 3])
    recs.sort(key=lambda r: r[4])
    write_bam(str(tmp_path / "in.bam"), [("chr7", len(chrom))], recs)
    return planted


def _tree(root):
    import os
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def check_panel_outputs(regions, tree, summary, planted, stderr_text):
    """What the panel must show, whichever engines computed it."""
    header = "#Chrom\tStart\tEnd\tMotif\tNum_Spanning\tMax_Spanning_Size\tNum_Partial_Left\tNum_Partial_Right\t" \
             "Max_Min_Repeat_Size\tNum_Exceeding\n"
    assert summary.startswith(header)
    srows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    assert len(srows) == 3 and srows[2][4:] == ["0", "-", "0", "0", "-", "0"]
    files = sorted(k for k in tree if k.endswith(".partial_reads.tsv"))
    assert len(files) == 2                                       # the third region has no reads
    n_exceeding = []
    for g, (region, unit) in enumerate(zip(regions[:2], ("CAG", "TATTG"))):
        p = len(unit)
        sizes = [r.round3_repeat_size for r in region.read_dict.values() if r.round3_repeat_size is not None]
        assert len(sizes) == 16 and not set(region.read_dict) & set(planted)       # every spanning read, no cut read
        top = max(sizes)
        text = tree[[k for k in files if unit in k][0]].decode().split("\n")
        assert text[0] == f"##RepeatRegion={region.to_unique_id()}" and text[1] == f"##Motif={unit}"
        assert text[2] == "#Read_Name\tAnchor\tStrand\tTail_Bases\tExtended_Bases\tMotif_Bases\tMin_Repeat_Size\t" \
                          "Score\tExceeds_Spanning"
        rows = [l.split("\t") for l in text[3:] if l]
        mine = {n: L for n, L in planted.items() if n.startswith(f"g{g}")}
        assert sorted(r[0] for r in rows) == sorted(mine)
        assert [(-int(r[6]), r[0]) for r in rows] == sorted((-int(r[6]), r[0]) for r in rows)
        exceeding = 0
        for name, anchor, strand, tail, ext, mb, size, score, exc in rows:
            L = mine[name]
            assert anchor == ("left" if name[2] == "l" else "right")
            assert (tail, ext, mb, score) == (str(L), str(L), str(L), str(2 * L)), (name, L)
            assert int(size) == L // p
            assert int(exc) == int(L // p > top), (name, L, top)
            exceeding += int(exc)
        strands = {r[0]: r[2] for r in rows}
        assert set(strands.values()) == {"+", "-"}
        n_exceeding.append(exceeding)
        assert srows[g][3:] == [unit, "16", f"{top:.1f}", str(sum(n[2] == "l" for n in mine)),
                                str(sum(n[2] == "r" for n in mine)), str(max(L // p for L in mine.values())),
                                str(exceeding)]
    # the long allele shows: every cut read of region 0 with more units than the short allele's largest read (the 12
    # reads cut after 30 units or more among them); none in region 1
    assert n_exceeding[0] >= 12 and n_exceeding[1] == 0
    notices = [l for l in stderr_text.split("\n") if l.startswith("NOTICE") and "one-anchor" in l]
    assert len(notices) == 1 and regions[0].to_unique_id() in notices[0]
    assert f"{n_exceeding[0]} one-anchor read(s)" in notices[0]


def run_panel(tmp_path, capsys, **engines):
    from nanorepeat_amd import pipeline
    planted = partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, **engines)
    off_regions = pipeline.quantify_from_bam(*args, str(tmp_path / "off"), **common)
    capsys.readouterr()
    regions = pipeline.quantify_from_bam(*args, str(tmp_path / "on"), partial_reads=True, **common)
    err = capsys.readouterr().err
    # the switch adds files and changes none; off, neither new name is written
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".partial_reads.tsv")} == off
    assert not any(k.endswith(".partial_reads.tsv") for k in off)
    assert not (tmp_path / "off.NanoRepeat_partial.tsv").exists()
    for a, b in zip(off_regions, regions):                       # the recording changes no placed read and no size
        assert list(a.read_dict) == list(b.read_dict)
        for n in a.read_dict:
            ra, rb = a.read_dict[n], b.read_dict[n]
            for f in ("round1_repeat_size", "round2_repeat_size", "round3_repeat_size", "core_seq_start_pos",
                      "core_seq_end_pos", "strand"):
                assert getattr(ra, f) == getattr(rb, f), (n, f)
    return regions, on, (tmp_path / "on.NanoRepeat_partial.tsv").read_text(), planted, err


def test_bam_command_finds_the_allele_no_read_spans(oracle, tmp_path, monkeypatch, capsys):
    monkeypatch.setitem(sys.modules, "pysam", None)
    regions, tree, summary, planted, err = run_panel(tmp_path, capsys, aligner=oracle.align_pairs,
                                                     scorer=oracle.round3_1d, extension_engine=ref_extend_tracts)
    check_panel_outputs(regions, tree, summary, planted, err)
    # the spanning reads alone give a clean call of the short allele: the output table knows nothing of the long one
    row = (tmp_path / "on.NanoRepeat_output.tsv").read_text().split("\n")[0].split("\t")
    assert max(float(x) for x in row[5:5 + int(row[4])]) < 20


def test_no_details_writes_only_the_summary(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"),
                               str(tmp_path / "o"), data_type="ont_q20", anchor_len=400, seed=1, no_details=True,
                               aligner=oracle.align_pairs, scorer=oracle.round3_1d, partial_reads=True,
                               extension_engine=ref_extend_tracts)
    assert not (tmp_path / "o.details").exists()
    assert len((tmp_path / "o.NanoRepeat_partial.tsv").read_text().split("\n")) == 5


# ---------------------------------------------------------------------------- C ABI checks
def test_extend_tracts_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    lib = capi.load()
    if lib.nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for motif, code in (("", -1), ("A" * 65, -3), ("CAN", -1), ("cag", -1)):
        with pytest.raises(capi.NraError) as e:
            capi.extend_tracts([motif], ["CAGCAG"], [0])
        assert e.value.code == code, motif
    for kw in (dict(match=0), dict(match=128), dict(mismatch=-1), dict(mismatch=128), dict(gap=0), dict(gap=128)):
        with pytest.raises(capi.NraError) as e:
            capi.extend_tracts(["CAG"], ["CAGCAG"], [0], **kw)
        assert e.value.code == -1, kw
    with pytest.raises(capi.NraError) as e:
        capi.extend_tracts(["CAG"], ["CAG"], [1])
    assert e.value.code == -1
    with pytest.raises(capi.NraError) as e:
        capi.extend_tracts(["CAG"], ["A" * 200001], [0])
    assert e.value.code == -3
    data, off = capi.pack_reads(["CAG"])
    none4 = (None,) * 4
    assert lib.nra_extend_tracts(0, 0, data, capi._ptr(off, C.c_int64), 0, None, None, None, 2, 4, 6, *none4) == -1
    assert lib.nra_extend_tracts(0, 1, data, None, 0, None, None, None, 2, 4, 6, *none4) == -1
    with pytest.raises(capi.NraError) as e:
        capi.extend_tracts(["CAG", "A" * 64], ["CAGCAG", ""], [0, 1], mismatch=0, gap=127)
    assert e.value.code == -2 and "no HIP device" in str(e.value)
