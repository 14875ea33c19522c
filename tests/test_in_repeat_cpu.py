"""In-repeat reads and the FASTQ command's partial reads without a GPU: the four extensions of a read without an
anchor, what upstream keeps when asked, the host form of the motif screen's count rule, and the FASTQ command with
partial_reads / in_repeat_reads on a panel with an allele no read spans (restatements as screener and extension
engine, the oracle as aligner and scorer)."""
import sys

import numpy as np
import pytest

import in_repeat_panel
from extend_ref import ref_extend_tracts
from nanorepeat_amd import partial, round3 as R3, screen, synth, upstream as U
from screen_partial_ref import RefScreenPartial, class_windows, classes_of


def _region(unit="CAG"):
    rr = R3.RepeatRegion(f"chr1\t1000\t1030\t{unit}")
    rr.left_anchor_seq, rr.right_anchor_seq = "A" * 400, "C" * 400
    return rr


def test_four_extensions_best_score_wins_and_ties_go_to_the_earliest():
    rr = _region()
    fwd = "CAG" * 30 + "TTTTTTTTTTTT"                 # the repeat from the first base on, other sequence at the end
    back = "TTTTTTTTTTTT" + "CAG" * 30                # ... from the last base backwards
    reads = {"f+": fwd, "f-": U.rev_comp(back), "b+": back, "b-": U.rev_comp(fwd), "pure": "AGC" * 25, "none": "N" * 50}
    rr.no_anchor_reads = dict.fromkeys(reads, True)
    calls = []

    def engine(motifs, tracts, read_motif, **kw):
        calls.append((list(motifs), list(tracts), list(read_motif), kw))
        return ref_extend_tracts(motifs, tracts, read_motif, **kw)

    class Sized:
        round3_repeat_size = 26.0

    rr.read_dict = {"s": Sized()}
    partial.in_repeat_regions([rr], [reads], engine=engine)
    motifs, tracts, rm, kw = calls[0]
    assert kw == dict(match=2, mismatch=4, gap=6, device=0)
    assert [motifs[i] for i in rm[:4]] == ["CAG", "CTG", "GAC", "GTC"]
    assert tracts[:4] == [fwd, fwd, fwd[::-1], fwd[::-1]]
    ir = rr.in_repeat_reads
    assert ir["f+"].fields() == ["+", "start", "102", "90", "90", "30", "180", "1"]
    assert ir["f-"].fields()[:2] == ["-", "start"] and ir["f-"].fields()[3:] == ["90", "90", "30", "180", "1"]
    assert ir["b+"].fields()[:2] == ["+", "end"] and ir["b-"].fields()[:2] == ["-", "end"]
    # a pure read scores the same from both ends: the first attempt keeps it; 25 units are not above 26.0
    assert ir["pure"].fields() == ["+", "start", "75", "75", "75", "25", "150", "0"]
    assert ir["none"].fields()[3:] == ["0", "0", "0", "0", "0"]
    assert partial.in_repeat_counts(rr) == (1, 26.0, 6, 30, 4)
    text = partial.in_repeat_reads_text(rr).split("\n")
    assert [l.split("\t")[0] for l in text[3:9]] == ["b+", "b-", "f+", "f-", "pure", "none"]    # units descending, name
    rr.read_dict = {}
    partial.in_repeat_regions([rr], [reads], engine=engine, keep=lambda region, seq: "N" * 50 != seq)
    assert sorted(rr.in_repeat_reads) == ["b+", "b-", "f+", "f-", "pure"]
    assert partial.in_repeat_counts(rr) == (0, None, 5, 30, 5)


def test_unsupported_motif_and_over_long_read_get_dash_fields():
    calls = []
    for unit, read in (("CAGN", "CAGCAG"), ("ACGTC" * 13, "CAGCAG"), ("CAG", "CAG" * 66667)):
        rr = _region(unit)
        rr.no_anchor_reads = {"a": True}
        partial.in_repeat_regions([rr], [{"a": read}], engine=lambda *a, **k: calls.append(a))
        assert rr.in_repeat_reads["a"].fields() == ["-", "-", str(len(read)), "-", "-", "-", "-", "-"]
        assert partial.in_repeat_counts(rr) == (0, None, 1, None, 0)
    assert not calls


def test_upstream_keeps_no_anchor_reads_only_when_asked():
    def aligner(seqs, pq, pt, sc=None, device=0):
        score = np.full(len(pq), -1, np.int32)
        for j, t in enumerate(pt):
            if "ACGTACGT" in seqs[t]:                            # "hit": the read carries the marker on this strand
                score[j] = 500
        return dict(score=score, tstart=np.full(len(pq), 10, np.int32), tend=np.full(len(pq), 300, np.int32))
    reads = {"hit": "TT" + "ACGTACGT" + "G" * 400, "bare": "CAG" * 100, "bare2": "CTG" * 90}
    asked, plain, many = _region(), _region(), _region()
    asked.keep_no_anchor_reads = many.keep_no_anchor_reads = True
    U.find_anchor_locations_in_reads("ont", asked, region_reads=reads, aligner=aligner)
    U.find_anchor_locations_in_reads("ont", plain, region_reads=reads, aligner=aligner)
    U.find_anchor_locations_in_reads_many("ont", [many], [reads], aligner=aligner)
    assert list(asked.no_anchor_reads) == list(many.no_anchor_reads) == ["bare", "bare2"]
    assert not hasattr(plain, "no_anchor_reads")
    assert list(asked.read_dict) == list(plain.read_dict) == list(many.read_dict)


def test_host_count_rule_equals_the_restatement():
    rng = np.random.default_rng(3)
    for motif in ("A", "AC", "CTG", "CAGCAG", "AAAG", "AATGG", "GGCCCC", "AAAAAAC", "CANG"):
        members = classes_of([motif])[1] if screen.screenable_motif(motif) else []
        assert (screen.motif_class(motif) is None) == (not members)
        root = (motif.upper() * 2)[:6]
        reads = [synth.apply_errors(rng, root * 40, "ont"), synth.revcomp(root * 30).lower(), "N".join([root * 5] * 4),
                 synth.rand_seq(rng, 400), root[:3], ""]
        for k in (11, 15):
            want = class_windows(reads, k, members)[:, 0].tolist() if members else [0] * len(reads)
            assert [screen.class_windows(s, motif, k) for s in reads] == want, (motif, k)
    assert screen.in_repeat_rule("CAG" * 20, "GCT", 15, 4, 100) and not screen.in_repeat_rule("CAG" * 20, "GCT", 15, 47, 5)
    assert not screen.in_repeat_rule("CAG" * 4, "CAG", 15) and not screen.in_repeat_rule("CAG" * 20, "AAAAAAC")


def test_fastq_command_finds_the_allele_no_read_spans(oracle, tmp_path, capsys):
    regions, names, _ = in_repeat_panel.run_and_check(tmp_path, capsys, aligner=oracle.align_pairs,
                                                      scorer=oracle.round3_1d, screener=RefScreenPartial,
                                                      extension_engine=ref_extend_tracts)
    # the spanning reads alone give a clean call of the short allele
    row = (tmp_path / "on.NanoRepeat_output.tsv").read_text().split("\n")[0].split("\t")
    assert max(float(x) for x in row[5:5 + int(row[4])]) < 25
    assert sorted(regions[0].one_anchor_reads) == sorted(names["left"] + names["right"])


def test_one_switch_alone_and_a_motif_without_a_class(oracle, tmp_path, capsys):
    from nanorepeat_amd import pipeline
    in_repeat_panel.write_panel(tmp_path)
    bed = (tmp_path / "r.bed").read_text().split("\n")
    args = (str(tmp_path / "in.fastq"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=in_repeat_panel.ANCHOR_LEN, seed=1, aligner=oracle.align_pairs,
                  scorer=oracle.round3_1d, screener=RefScreenPartial, extension_engine=ref_extend_tracts)
    pipeline.quantify_from_reads(*args, str(tmp_path / "p"), partial_reads=True, **common)
    assert (tmp_path / "p.NanoRepeat_partial.tsv").exists() and not (tmp_path / "p.NanoRepeat_in_repeat.tsv").exists()
    assert not any(k.endswith(".in_repeat_reads.tsv") for k in in_repeat_panel.tree(tmp_path / "p.details"))
    # the third region's motif written as a 12-base word whose root has 12 bases: no class
    (tmp_path / "r.bed").write_text("\n".join(bed[:2] + [bed[2].rsplit("\t", 1)[0] + "\tGGCCCCGGCCCA"]) + "\n")
    capsys.readouterr()
    pipeline.quantify_from_reads(*args, str(tmp_path / "q"), in_repeat_reads=True, no_details=True,
                                 no_check_repeat_motif_in_ref=True, **common)
    err = capsys.readouterr().err
    rows = [l.split("\t") for l in (tmp_path / "q.NanoRepeat_in_repeat.tsv").read_text().split("\n")[2:] if l]
    assert rows[0][6] == "8" and rows[2][6:] == ["-", "-", "-", "0"]
    assert sum("motif without a class" in l for l in err.split("\n")) == 1
    assert not (tmp_path / "q.NanoRepeat_partial.tsv").exists() and not (tmp_path / "q.details").exists()


def test_bam_command_in_repeat_reads_adds_files_and_changes_none(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_partial_cpu import partial_panel
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  extension_engine=ref_extend_tracts, partial_reads=True)
    pipeline.quantify_from_bam(*args, str(tmp_path / "off"), **common)
    pipeline.quantify_from_bam(*args, str(tmp_path / "on"), in_repeat_reads=True, **common)
    for s in (".NanoRepeat_output.tsv", ".NanoRepeat_partial.tsv"):
        assert (tmp_path / ("on" + s)).read_bytes() == (tmp_path / ("off" + s)).read_bytes()
    on, off = in_repeat_panel.tree(tmp_path / "on.details"), in_repeat_panel.tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".in_repeat_reads.tsv")} == off
    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_in_repeat.tsv").read_text().split("\n")[2:] if l]
    assert len(rows) == 3 and all(r[6:] == ["0", "-", "0", "-"] for r in rows)
