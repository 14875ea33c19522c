"""CpG methylation without a device: the restatement against a case counted by hand, the tag parser, the tags through
the BAM container reader, a pysam stand-in and FASTQ comments, the orientation invariance of the contract, and both
commands from files to files with the restatement as the engine."""
import sys
import types

import numpy as np
import pytest

import methylation_cases as K
import methylation_ref as R
from nanorepeat_amd import bam as B, io as nr_io, methylation as M
from nanorepeat_amd.round3 import RepeatRegion

# ---------------------------------------------------------------------------- (a) a case counted by hand
# index      0         1         2
#            012345678901234567890123
HAND_READ = "ACGTTCGAcgNCCGTACGGTACGA"
# sites (stored C of a CG): 1 5 8 12 16 21.  Tract [7, 13), flank 9, bin 4: nb = 3, rows before0 before1 before2 tract
# after0 after1 after2.  Site 1 -> before1 (7 - 1 - 2 = 4), 5 -> before0 (0), 8 -> tract, 12 -> none (12 + 2 > 13 and
# 12 < 13: it straddles the edge), 16 -> after0 (3), 21 -> after2 (8).
# Forward, the C of O are stored 1 5 8 11 12 16 21 (ranks 0..6): the sites have ranks 0 1 2 4 5 6.
# Reversed, the C of O are the stored G 22 18 17 13 9 6 2 (ranks 0..6): the sites 21 16 12 8 5 1 have ranks 0 2 3 4 5 6.
# The list names the ranks 0, 2, 5, 6 (deltas 0 1 2 0) with the bytes 200 63 192 100; hi = 192, lo = 63.
HAND_LIST = (np.array([0, 1, 2, 0], np.int32), np.array([200, 63, 192, 100], np.uint8))
HAND_ARGS = dict(flank=9, bin=4, lo_byte=63, hi_byte=192)
Z = [0, 0, 0, 0, 0]
HAND_WANT = {
    0: [[1, 0, 0, 0, 0], [1, 1, 1, 0, 200], Z, [1, 1, 0, 1, 63], [1, 1, 1, 0, 192], Z, [1, 1, 0, 0, 100]],
    2: [[1, 1, 0, 1, 0], [1, 1, 1, 0, 200], Z, [1, 1, 0, 1, 63], [1, 1, 1, 0, 192], Z, [1, 1, 0, 0, 100]],
    1: [[1, 1, 1, 0, 192], [1, 1, 0, 0, 100], Z, [1, 0, 0, 0, 0], [1, 1, 0, 1, 63], Z, [1, 1, 1, 0, 200]],
    3: [[1, 1, 1, 0, 192], [1, 1, 0, 0, 100], Z, [1, 1, 0, 1, 0], [1, 1, 0, 1, 63], Z, [1, 1, 1, 0, 200]],
}


def hand_call(engine, **kw):
    bits = sorted(HAND_WANT)
    return engine([HAND_READ] * 4, [HAND_LIST] * 4, np.array(bits, np.uint8), np.full(4, 7, np.int32),
                  np.full(4, 13, np.int32), **HAND_ARGS, **kw), bits


@pytest.mark.parametrize("engine", [R.ref_read_methylation, R.np_read_methylation])
def test_hand_counted_case(engine):
    out, bits = hand_call(engine)
    for i, b in enumerate(bits):
        assert out["counts"][i].tolist() == HAND_WANT[b], b
    assert out["n_c"].tolist() == [7, 7, 7, 7] and out["status"].tolist() == [0, 0, 0, 0]


def test_numpy_form_equals_the_restatement():
    batch = K.edge_batch(seed=4, lengths=[0, 1, 2, 63, 64, 65, 255, 257, 1000])
    kinds = K.kinds_batch()
    for b in (batch, kinds):
        for flank, bin_len in K.SHAPES:
            want, got = K.call(R.ref_read_methylation, b, flank, bin_len), K.call(R.np_read_methylation, b, flank, bin_len)
            for key in ("counts", "n_c", "status"):
                assert np.array_equal(want[key], got[key]), (key, flank, bin_len)
    # the kinds do what their names say
    st = K.call(R.ref_read_methylation, kinds)["status"].reshape(-1)
    by_kind = {k: st[4 * i:4 * i + 4].tolist() for i, k in enumerate(K.LIST_KINDS)}
    assert all(by_kind[k] == [0] * 4 for k in ("empty", "all", "cpg", "random", "last"))
    assert all(by_kind[k] == [1] * 4 for k in ("beyond", "huge", "too_many"))
    assert st[-2:].tolist() == [0, 1]                                   # n_c - 1 is fine, n_c is not


# ---------------------------------------------------------------------------- (b) the tag parser
def test_parse_mm():
    d, p, implicit = M.parse_mm("C+m?,0,1,2,0;", bytes([200, 63, 192, 100]))
    assert d.tolist() == [0, 1, 2, 0] and p.tolist() == [200, 63, 192, 100] and implicit is False
    assert d.dtype == np.int32 and p.dtype == np.uint8
    # several entries: ML is their concatenation, the first matching one is taken
    mm, ml = "A+a,1,1;C+h?,5;C+m.,2,3;C+m,9;", bytes([1, 2, 77, 10, 20, 99])
    d, p, implicit = M.parse_mm(mm, ml)
    assert (d.tolist(), p.tolist(), implicit) == ([2, 3], [10, 20], True)
    d, p, implicit = M.parse_mm(mm, ml, mod_code="h")
    assert (d.tolist(), p.tolist(), implicit) == ([5], [77], False)
    d, p, implicit = M.parse_mm(mm, ml, base="A", mod_code="a")
    assert (d.tolist(), p.tolist(), implicit) == ([1, 1], [1, 2], True)
    # two codes in one entry: interleaved per position in the order of the codes
    for codes, want_m, want_h in (("mh", [1, 3, 5], [2, 4, 6]), ("hm", [2, 4, 6], [1, 3, 5])):
        mm = f"C+{codes}?,0,0,7;"
        assert M.parse_mm(mm, bytes([1, 2, 3, 4, 5, 6]))[1].tolist() == want_m
        assert M.parse_mm(mm, bytes([1, 2, 3, 4, 5, 6]), mod_code="h")[1].tolist() == want_h
    # a ChEBI code is one code, and is matched whole
    d, p, _ = M.parse_mm("C+76792,4;C+27551?,1,1;", bytes([9, 8, 7]), mod_code="27551")
    assert (d.tolist(), p.tolist()) == ([1, 1], [8, 7])
    assert M.parse_mm("C+76792,4;", bytes([9]), mod_code="7") == M.NO_MOD
    # the flag
    assert [M.parse_mm(f"C+m{f},1;", b"\x05")[2] for f in ("?", ".", "")] == [False, True, True]
    # an empty delta list, with and without ML
    for ml in (b"", None):
        d, p, implicit = M.parse_mm("C+m?;", ml)
        assert len(d) == len(p) == 0 and implicit is False
    assert M.parse_mm("C+m?", b"")[0].tolist() == []                    # no trailing separator
    # the statuses
    assert M.parse_mm(None, None) == M.NO_TAG
    assert M.parse_mm("", b"") == M.NO_MOD
    assert M.parse_mm("C+h,1;C-m,1;G+m,1;", bytes(3)) == M.NO_MOD      # another code, the other strand, another base
    for bad in ("C+m?,1,-2;", "C+m?,x;", "C+m?,1,;", "C*m,1;", "+m,1;", "C+m!,1;", "C+,1;", "C+m?,1.5;",
                "C+m,99999999999;", "C+m4,1;"):
        assert M.parse_mm(bad, bytes(bad.count(","))) == M.BAD_TAG, bad
    assert M.parse_mm("C+m?,1,2;", bytes(3)) == M.BAD_TAG               # ML too long
    assert M.parse_mm("C+mh?,1,2;", bytes(3)) == M.BAD_TAG              # ML too short for two codes
    assert M.parse_mm("C+m?,1;", None) == M.BAD_TAG
    assert M.parse_mm("A+a,1;C+m?,1;", bytes(1)) == M.BAD_TAG           # the total counts, not the entry's share


def test_decode_read_tags():
    assert M.decode_read_tags(None)[0] == M.NO_TAG
    assert M.decode_read_tags((None, None, True, False))[0] == M.NO_TAG
    assert M.decode_read_tags(("C+m?,1;", b"\x01", False, False))[0] == M.CLIPPED
    assert M.decode_read_tags(("C+h?,1;", b"\x01", False, True))[0] == M.NO_MOD
    for rev, flag, bits in ((False, "?", 0), (True, "?", 1), (False, ".", 2), (True, "", 3)):
        st, d, p, got = M.decode_read_tags((f"C+m{flag},4;", b"\x09", rev, True))
        assert (st, d.tolist(), p.tolist(), got) == (M.OK, [4], [9], bits)


# ---------------------------------------------------------------------------- (c) the container reader
EVERY_TYPE = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 250), ("Xs", "s", -3000), ("XS", "S", 60000),
              ("Xi", "i", -100000), ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "MM:Z:C+m,1;"),
              ("XH", "H", "1AE301"), ("Bc", ("B", "c"), [-1, 2]), ("BC", ("B", "C"), [1, 2, 3]),
              ("Bs", ("B", "s"), [-300]), ("BS", ("B", "S"), [300, 301]), ("Bi", ("B", "i"), [-70000]),
              ("BI", ("B", "I"), [70000, 1]), ("Bf", ("B", "f"), [0.5, 0.25]), ("Be", ("B", "C"), [])]


def _tag_records():
    filler = b"".join(K.tag_bytes(*t) for t in EVERY_TYPE)
    seq = "ACGTCGCGTTACGCGA"
    mm, ml = "C+m?,0,1;", [7, 200]
    both = K.tag_bytes("MM", "Z", mm) + K.tag_bytes("ML", ("B", "C"), ml)
    recs = [("plain", seq, "c", 10, 40, 0, b"", 0),
            ("front", seq, "c", 11, 40, 0x10, filler + both, 0),
            ("behind", seq, "c", 12, 40, 0, both + filler, 0),
            ("between", seq, "c", 13, 40, 0, K.tag_bytes("MM", "Z", mm) + filler + K.tag_bytes("ML", ("B", "C"), ml) + filler, 0),
            ("old", seq, "c", 14, 40, 0x10, K.tag_bytes("Mm", "Z", mm) + K.tag_bytes("Ml", ("B", "C"), ml), 0),
            ("clipped", seq, "c", 15, 40, 0, both, 5),
            ("mn_ok", seq, "c", 16, 40, 0, both + K.tag_bytes("MN", "S", len(seq)), 0),
            ("mn_off", seq, "c", 17, 40, 0, K.tag_bytes("MN", "i", len(seq) + 4) + both, 0),
            ("front", "ACGT", "c", 18, 40, 0, both, 0),                  # a second record of a name: the first wins
            ("no_ml", seq, "c", 19, 40, 0, K.tag_bytes("MM", "Z", "C+m?;"), 0)]
    want = {"plain": (None, None, False, True), "front": (mm, bytes(ml), True, True),
            "behind": (mm, bytes(ml), False, True), "between": (mm, bytes(ml), False, True),
            "old": (mm, bytes(ml), True, True), "clipped": (mm, bytes(ml), False, False),
            "mn_ok": (mm, bytes(ml), False, True), "mn_off": (mm, bytes(ml), False, False),
            "no_ml": ("C+m?;", None, False, True)}
    return recs, want


@pytest.mark.parametrize("block", [37, 4000])
def test_container_reader_carries_the_tags(tmp_path, monkeypatch, block):
    """Every tag type stepped over in front of, between and behind MM / ML; with 37-byte BGZF blocks every record's
    tags cross block edges."""
    monkeypatch.setitem(sys.modules, "pysam", None)
    recs, want = _tag_records()
    path = str(tmp_path / "t.bam")
    K.write_bam(path, [("c", 1000)], recs, block=block)
    region = RepeatRegion("c\t20\t30\tCAG")
    got = {}
    n = B.extract_fastq_from_bam(path, region, 5, str(tmp_path / "with.fastq"), mod_tags=got)
    assert n == len(want) and got == want
    assert B.extract_fastq_from_bam(path, region, 5, str(tmp_path / "without.fastq")) == n
    assert (tmp_path / "with.fastq").read_bytes() == (tmp_path / "without.fastq").read_bytes()
    f = B.BamFile(path)                                                  # unless asked, tags are not parsed
    assert all(r.tags is None for r in f.fetch("c", 0, 1000))
    f.close()
    assert [M.decode_read_tags(got[k])[0] for k in ("plain", "front", "clipped", "mn_off", "no_ml")] == \
        [M.NO_TAG, M.OK, M.CLIPPED, M.CLIPPED, M.OK]


def test_pysam_stand_in_gives_the_same_dict(tmp_path, monkeypatch):
    recs, want = _tag_records()

    class Read:
        def __init__(self, name, seq, flag, tags, clip):
            self.query_name, self.query_sequence, self.query_qualities = name, seq, None
            self.is_reverse = bool(flag & 0x10)
            self.cigartuples = ([(5, clip)] if clip else []) + [(0, len(seq))]
            self._tags = tags

        def has_tag(self, key):
            return key in self._tags

        def get_tag(self, key):
            return self._tags[key]

    def tags_of(raw):
        import array
        got = B.parse_mod_tags(raw, 0)
        out = {}
        if "MM" in got:
            out["Mm" if b"Mm" in raw else "MM"] = got["MM"]
        if "ML" in got:
            out["Ml" if b"Ml" in raw else "ML"] = array.array("B", got["ML"])      # pysam returns an array
        if "MN" in got:
            out["MN"] = got["MN"]
        return out

    class AlignmentFile:
        def __init__(self, path, mode, reference_filename=None):
            pass

        def fetch(self, chrom, start, end):
            return [Read(name, seq, flag, tags_of(raw), clip) for name, seq, _, _, _, flag, raw, clip in recs]

        def close(self):
            pass

    monkeypatch.setitem(sys.modules, "pysam", types.SimpleNamespace(AlignmentFile=AlignmentFile))
    got = {}
    B.extract_fastq_from_bam("in.bam", RepeatRegion("c\t20\t30\tCAG"), 5, str(tmp_path / "o.fastq"), mod_tags=got)
    assert got == want


# ---------------------------------------------------------------------------- (d) FASTQ header tags
def test_fastq_header_tags(tmp_path):
    text = ("@a\tMM:Z:C+m?,0,1;\tML:B:C,7,200\n" "ACGTCGCG\n+\n########\n"
            "@b some words MN:i:8 Ml:B:C,9 Mm:Z:C+m,3;\n" "ACGTCGCG\n+\n########\n"
            "@c\tMN:i:9\tMM:Z:C+m,3;\tML:B:C,1\n" "ACGTCGCG\n+\n########\n"
            "@d\n" "ACGT\n+\n####\n"
            "@e\tMM:Z:C+m?;\tML:B:C\n" "ACGT\n+\n####\n"
            "@a\tMM:Z:C+h,1;\tML:B:C,1\n" "AC\n+\n##\n")
    (tmp_path / "t.fastq").write_text(text)
    got = nr_io.read_fastq_mod_tags(str(tmp_path / "t.fastq"))
    assert got == {"a": ("C+m?,0,1;", bytes([7, 200]), False, True), "b": ("C+m,3;", bytes([9]), False, True),
                   "c": ("C+m,3;", bytes([1]), False, False), "e": ("C+m?;", b"", False, True)}
    assert list(nr_io.read_fastq(str(tmp_path / "t.fastq"))) == ["a", "b", "c", "d", "e"]


# ---------------------------------------------------------------------------- (e) orientation invariance
def test_a_reverse_complement_record_gives_the_same_counters_with_the_sides_exchanged():
    batch = K.edge_batch(seed=7, lengths=[0, 1, 2, 63, 64, 65, 129, 500, 1025])
    for flank, bin_len in K.SHAPES[:3]:
        a, b = K.call(R.ref_read_methylation, batch, flank, bin_len), K.call(R.ref_read_methylation, K.mirrored(batch), flank, bin_len)
        assert np.array_equal(a["counts"], K.swap_sides(b["counts"]))
        assert np.array_equal(a["n_c"], b["n_c"]) and np.array_equal(a["status"], b["status"])
        assert a["counts"].sum() > 0


# ---------------------------------------------------------------------------- (f) the commands
METH = dict(methylation=True, meth_flank=300, meth_bin=100)


def check_command_files(prefix, regions, truth, capsys_err):
    """The three files of a run of command_case: rows, statuses, and the planted difference."""
    region = regions[0]
    rows = [l.split("\t") for l in open(f"{region.out_prefix}.read_methylation.tsv").read().split("\n")
            if l and not l.startswith("#")]
    assert len(rows) == 22 and all(len(r) == 5 + 18 for r in rows)
    structure_order = [n for n, _ in M._ordered_reads(region)]
    assert [r[0] for r in rows] == structure_order
    by_name = {r[0]: r for r in rows}
    assert by_name["r20"][4] == M.NO_TAG and by_name["r21"][4] == M.CLIPPED
    assert all(by_name[n][5:] == ["-"] * 18 for n in ("r20", "r21"))
    assert all(r[4] == M.OK for r in rows if r[0] not in ("r20", "r21"))
    assert {r[3] for r in rows} == {"+", "-"}
    long_ids = {r[1] for r in rows if truth[r[0]] == 30 and r[1] != "."}
    short_ids = {r[1] for r in rows if truth[r[0]] == 10 and r[1] != "."}
    assert len(long_ids) == len(short_ids) == 1 and long_ids != short_ids
    long_id, short_id = long_ids.pop(), short_ids.pop()
    for r in rows:
        if r[4] != M.OK:
            continue
        tract, left, right = r[5:11], r[11:17], r[17:23]
        assert int(tract[0]) == int(tract[1]) == truth[r[0]] and int(left[0]) == int(left[1]) > 0 and int(right[0]) > 0
        if truth[r[0]] == 30:
            assert (tract[4], left[4], right[4]) == ("1.0000", "1.0000", "0.0000"), r
            explicit = int(r[0][1:]) % 3 != 1              # an unlisted site of an implicit list is byte 0
            assert tract[5] == f"{250.5 / 256:.4f}" and right[5] == f"{(5.5 if explicit else 0.5) / 256:.4f}"
        else:
            assert (tract[4], left[4], right[4]) == ("0.0000", "0.0000", "0.0000"), r
    alleles = [l.split("\t") for l in open(f"{region.out_prefix}.allele_methylation.tsv").read().split("\n")
               if l and not l.startswith("#")]
    assert len(alleles) == 2 * 7 and all(len(a) == 11 for a in alleles)
    assert [a[1:4] for a in alleles[:7]] == [["LEFT", "200", "300"], ["LEFT", "100", "200"], ["LEFT", "0", "100"],
                                             ["TRACT", "-", "-"], ["RIGHT", "0", "100"], ["RIGHT", "100", "200"],
                                             ["RIGHT", "200", "300"]]
    for a in alleles:
        want = "1.0000" if a[0] == long_id and a[1] != "RIGHT" else "0.0000"
        assert a[9] == want and int(a[4]) == 10 and int(a[5]) == int(a[6]) > 0, a
    tract_rows = {a[0]: a for a in alleles if a[1] == "TRACT"}
    assert int(tract_rows[long_id][5]) == 10 * 30 and int(tract_rows[short_id][5]) == 10 * 10
    summary = open(f"{prefix}.NanoRepeat_methylation.tsv").read().split("\n")
    assert summary[0] == "#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tReads_With_Calls\tReads_Without\tAllele_Methylation"
    assert len(summary) == 3 and summary[2] == ""
    f = summary[1].split("\t")
    assert f[3:7] == ["CGG", "2", "20", "2"]
    cells = dict(c.split(":", 1) for c in f[7].split("|"))
    assert cells[long_id] == "10:1.0000:1.0000:0.0000" and cells[short_id] == "10:0.0000:0.0000:0.0000"
    assert "NOTICE: methylation: 2 read(s) with a size have no usable calls (NO_TAG 1, CLIPPED 1)" in capsys_err


def run_commands(tmp_path, oracle, engine, tag):
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    bam = pipeline.quantify_from_bam(str(tmp_path / "in.bam"), ref, bed, str(tmp_path / f"bam_{tag}"),
                                     methylation_engine=engine, **METH, **common)
    fq = pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / f"fq_{tag}"),
                                      screener=RefScreen, methylation_engine=engine, **METH, **common)
    return bam, fq, common


def test_commands_from_files_to_files(oracle, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    from test_screen_cpu import _tree
    monkeypatch.setitem(sys.modules, "pysam", None)
    truth = K.command_case(tmp_path)
    capsys.readouterr()
    bam, fq, common = run_commands(tmp_path, oracle, R.ref_read_methylation, "on")
    err = capsys.readouterr().err
    assert err.count("NOTICE: methylation:") == 2
    check_command_files(str(tmp_path / "bam_on"), bam, truth, err)
    check_command_files(str(tmp_path / "fq_on"), fq, truth, err)
    # every other file is what the command writes without the switch
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), ref, bed, str(tmp_path / "bam_off"), methylation=False, **common)
    pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / "fq_off"), screener=RefScreen,
                                 **common)
    for kind in ("bam", "fq"):
        on, off = _tree(tmp_path / f"{kind}_on.details"), _tree(tmp_path / f"{kind}_off.details")
        assert {k: v for k, v in on.items() if "_methylation." not in k} == off
        assert sorted(k.rsplit(".", 2)[-2] for k in on if "_methylation." in k) == ["allele_methylation", "read_methylation"]
        assert sorted(p.name for p in tmp_path.glob(f"{kind}_off.*")) == [f"{kind}_off.NanoRepeat_output.tsv", f"{kind}_off.details"]
        assert sorted(p.name for p in tmp_path.glob(f"{kind}_on.*")) == [
            f"{kind}_on.NanoRepeat_methylation.tsv", f"{kind}_on.NanoRepeat_output.tsv", f"{kind}_on.details"]
        assert (tmp_path / f"{kind}_on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / f"{kind}_off.NanoRepeat_output.tsv").read_bytes()
    # no_details: the summary only
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), ref, bed, str(tmp_path / "nd"), no_details=True,
                               methylation_engine=R.ref_read_methylation, **METH, **common)
    assert sorted(p.name for p in tmp_path.glob("nd.*")) == ["nd.NanoRepeat_methylation.tsv", "nd.NanoRepeat_output.tsv"]
    assert (tmp_path / "nd.NanoRepeat_methylation.tsv").read_bytes() == (tmp_path / "bam_on.NanoRepeat_methylation.tsv").read_bytes()


# ---------------------------------------------------------------------------- (g) bad values
@pytest.mark.parametrize("bad", [dict(meth_flank=0), dict(meth_flank=100001), dict(meth_bin=0), dict(meth_bin=2001),
                                 dict(meth_flank=6500, meth_bin=100), dict(meth_lo=192), dict(meth_lo=-1),
                                 dict(meth_hi=256), dict(meth_hi=10, meth_lo=20), dict(meth_mod_code=""),
                                 dict(meth_mod_code="M"), dict(meth_mod_code="mh"), dict(meth_flank=2000.5)])
def test_bad_values_are_refused_before_any_work(tmp_path, bad):
    from nanorepeat_amd import pipeline
    missing = [str(tmp_path / n) for n in ("no.bam", "no.fa", "no.bed")]
    for command in (pipeline.quantify_from_bam, pipeline.quantify_from_reads):
        with pytest.raises(ValueError, match="meth_|call bytes"):
            command(*missing, str(tmp_path / "out"), methylation=True, **bad)
    assert not list(tmp_path.iterdir())
