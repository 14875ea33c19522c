"""Tandem motifs without a GPU: the numpy restatement against the brute force, hand cases of the contract, the per-read
call and the in-phase unit, both commands with discover_motifs=True (restatement as motif engine, oracle as scorer) on
synth.motif_panel, and the argument checks of nra_tract_motifs."""
import ctypes as C
import sys

import numpy as np
import pytest

from nanorepeat_amd import motifs, round3, structure, synth
from motif_ref import ref_tract_motifs, lyndon_classes


def _top(out, t=0):
    return [(motifs.class_string(int(p), int(c)), int(k))
            for p, c, k in zip(out["top_p"][t], out["top_code"][t], out["top_count"][t]) if k > 0]


def test_numpy_restatement_equals_brute_force():
    rng = np.random.default_rng(21)
    tracts = []
    for i in range(120):
        p = int(rng.integers(1, 7))
        u = synth.rand_unit(rng, p) if p > 1 else "ACGT"[i % 4]
        base = (u * 40)[int(rng.integers(0, p)):][:int(rng.integers(0, 120))]
        kind = i % 5
        s = base if kind == 0 else synth.apply_errors(rng, base, "ont") if kind == 1 else \
            synth.rand_seq(rng, int(rng.integers(0, 60))) if kind == 2 else base.lower() if kind == 3 else \
            "".join(ch if rng.random() > 0.05 else "N" for ch in base)
        tracts.append(s)
    for max_period, top_n in ((6, 8), (6, 1), (3, 4), (1, 2)):
        a = ref_tract_motifs(tracts, max_period, top_n)
        b = ref_tract_motifs(tracts, max_period, top_n, vectorised=False)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, max_period, top_n)


def test_there_are_964_classes():
    cls = lyndon_classes()
    assert [sum(p == q for p, _ in cls) for q in range(1, 7)] == [4, 6, 20, 60, 204, 670]
    assert len(cls) == 964


def test_hand_cases():
    out = ref_tract_motifs(["A" * 30])
    assert list(out["n_tandem"][0]) == [29, 0, 0, 0, 0, 0] and _top(out) == [("A", 29)]
    assert list(out["top_p"][0]) == [1, 0, 0, 0] and list(out["top_code"][0]) == [0, -1, -1, -1]
    out = ref_tract_motifs(["AT" * 20])
    assert out["n_tandem"][0][3] == 0 and out["n_tandem"][0][5] == 0 and _top(out) == [("AT", 37)]
    out = ref_tract_motifs(["CAG" * 10])
    assert _top(out) == [("AGC", 25)] and out["top_code"][0][0] == 0b001001
    # an N breaks every window over it
    assert _top(ref_tract_motifs(["CAG" * 3 + "N" + "CAG" * 3])) == [("AGC", 4 + 4)]
    assert _top(ref_tract_motifs(["CAGCAN"])) == []
    # empty, and shorter than 2p
    out = ref_tract_motifs(["", "A", "CAGCA"])
    assert not out["n_tandem"].any() and (out["top_code"] == -1).all()
    # ties: count, then p, then code
    out = ref_tract_motifs(["TTTGGGCCCAAA"], top_n=8)
    assert _top(out) == [("A", 2), ("C", 2), ("G", 2), ("T", 2)]
    out = ref_tract_motifs(["ACAC" + "GG" + "CATCAT"], top_n=3)
    assert _top(out) == [("G", 1), ("AC", 1), ("ATC", 1)]


def test_call_thresholds_and_in_phase_unit():
    assert motifs.dominant_call([("AGC", 4)], 40) == "AGC"
    assert motifs.dominant_call([("AGC", 3)], 10) is None                      # below min_motif_count
    assert motifs.dominant_call([("AGC", 9)], 100) is None                     # below 10 % of the tract
    assert motifs.dominant_call([("AGC", 10)], 100) == "AGC"
    assert motifs.dominant_call([("AGC", 3)], 10, min_motif_count=3) == "AGC"
    assert motifs.dominant_call([("AGC", 9)], 100, min_motif_share=0.05) == "AGC"
    assert motifs.dominant_call([], 0) is None
    assert motifs.in_phase_unit("GCAGCAGCA", "AGC") == "GCA"
    assert motifs.in_phase_unit("TTAAGGGAAGGG", "AAGGG") == "AAGGG"
    assert motifs.in_phase_unit("GGGAAGGGAA", "AAGGG") == "GGGAA"
    assert motifs.in_phase_unit("ACGT", "AGC") is None
    assert motifs.bed_class("CAGCAG") == "AGC" and motifs.bed_class("AAAAG") == "AAAAG"
    assert motifs.bed_class("A" * 8) == "A" and motifs.bed_class("ACGTACG") is None
    assert motifs.bed_class("CAN") is None and motifs.bed_class("tattg") == "ATTGT"
    assert motifs.motif_class("TTTCA") == "ATTTC"


# ---------------------------------------------------------------------------- the commands
def _panel_files(tmp_path):
    p = synth.motif_panel(reads_per_allele=4, anchor_len=400, model="hifi", seed=12)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    return p, ref, bed, reads


def _run_both(tmp_path, command, oracle, src, ref, bed, extra):
    from test_screen_cpu import _tree
    common = dict(dict(data_type="hifi", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d),
                  **extra)
    command(src, ref, bed, str(tmp_path / "off"), **common)
    regions = command(src, ref, bed, str(tmp_path / "on"), discover_motifs=True, motif_engine=ref_tract_motifs,
                      **common)
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_motifs.tsv")} == off
    assert not (tmp_path / "off.NanoRepeat_motifs.tsv").exists()
    return regions, on, (tmp_path / "on.NanoRepeat_motifs.tsv").read_text()


def _motif_file(tmp_path, tree, region):
    import os
    return tree[os.path.relpath(region.out_prefix + ".read_motifs.tsv", str(tmp_path / "on.details"))].decode()


def _check_outputs(tmp_path, p, regions, tree, summary, oracle):
    files = sorted(k for k in tree if k.endswith(".read_motifs.tsv"))
    assert len(files) == 4
    for g, region in enumerate(regions):
        text = _motif_file(tmp_path, tree, region)
        lines = text.split("\n")
        assert lines[0] == f"##RepeatRegion={region.to_unique_id()}" and lines[1] == f"##Motif={region.repeat_unit_seq}"
        assert lines[2] == f"##BED_Class={motifs.bed_class(region.repeat_unit_seq)}"
        assert lines[3] == ("#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tDominant_Motif\tDiffers\tSize_In_Motif\t"
                            "Top_Motifs")
        rows = [l.split("\t") for l in lines[4:] if l]
        assert sorted(r[0] for r in rows) == sorted(n for n in region.read_dict if n in region.read_core_seq_dict)
        phased = [l.split("\t") for l in open(region.out_prefix + ".phased_reads.txt").read().split("\n")[2:] if l]
        assert [(r[0], r[1]) for r in rows[:len(phased)]] == [(r[0], r[1]) for r in phased]
        assert all(r[1] == "." for r in rows[len(phased):])
        assert [r[0] for r in rows[len(phased):]] == sorted(r[0] for r in rows[len(phased):])
        calls = {}
        for r in rows:
            assert len(r) == 8
            calls.setdefault(p["truth"][r[0]][1], []).append(r[4])
            assert r[5] == ("-" if r[4] == "-" else "yes" if r[4] != motifs.bed_class(region.repeat_unit_seq) else "no")
            if r[5] == "no":
                assert r[6] == r[2]
            if r[4] != "-":
                assert r[7].split(",")[0].split(":")[0] == r[4]
        # most reads of an allele call its planted class (a homopolymer-rich motif such as AAAAG or ATTTT can lose a
        # read to its period-1 class when errors break its period-5 windows)
        for a, got in calls.items():
            want = p["planted"][g][a][0]
            assert 2 * sum(c == want for c in got) > len(got), (g, a, got)
        if g == 3:
            assert all(r[5] == "no" for r in rows) and not any(rm.differs for rm in region.read_motifs.values())
    # the re-sized reads equal the oracle's sizes for them
    for region in regions:
        redo = [(n, rm) for n, rm in region.read_motifs.items() if rm.differs]
        for name, rm in redo:
            tract = structure.tract_of(region, name).upper()
            unit = motifs.in_phase_unit(tract, rm.call)
            lo, hi = round3.round3_window(len(tract) / len(unit), False)
            out = oracle.round3_1d([(region.left_anchor_seq, unit, region.right_anchor_seq)],
                                   [region.read_core_seq_dict[name].strip()], np.array([lo], np.int32),
                                   np.array([hi], np.int32))
            assert int(out["status"][0]) == 0
            assert rm.size_in_motif == out["sum_k"][0] / out["n_ties"][0]
    srows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    assert summary.startswith("#Chrom\tStart\tEnd\tMotif\tNum_Reads\tMotif_Groups\tAllele_Motifs\n")
    assert len(srows) == 4
    groups = [dict((c.split(":")[0], c.split(":")[1:]) for c in row[5].split(",")) for row in srows]
    assert abs(float(groups[0]["AAGGG"][1]) - 200) <= 2 and int(groups[0]["AAGGG"][0]) == 4
    assert abs(float(groups[1]["CCTG"][1]) - 120) <= 2
    assert set(groups[3]) == {"ATTGT"}
    assert any("ATTTC" in cell.split(":")[3].split(",") for cell in srows[2][6].split("|"))


def test_fastq_command_writes_motif_files(oracle, tmp_path):
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    p, ref, bed, reads = _panel_files(tmp_path)
    _check_outputs(tmp_path, p, *_run_both(tmp_path, pipeline.quantify_from_reads, oracle, reads, ref, bed,
                                 dict(screener=RefScreen)), oracle)


def test_bam_command_writes_motif_files(oracle, tmp_path, monkeypatch):
    """The BAM case of test_bam: pure CAG and TATTG alleles, so almost every read calls the BED class."""
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    regions, tree, summary = _run_both(tmp_path, pipeline.quantify_from_bam, oracle, str(tmp_path / "in.bam"),
                                       str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"), dict(data_type="ont_q20"))
    assert sum(k.endswith(".read_motifs.tsv") for k in tree) == 2
    for region in regions[:2]:
        rows = [l.split("\t") for l in _motif_file(tmp_path, tree, region).split("\n")[4:] if l]
        assert len(rows) == len(region.read_core_seq_dict) >= 20
        assert 10 * sum(r[5] == "no" for r in rows) >= 9 * len(rows)       # a short TATTG read may call T
        assert all(r[6] == r[2] for r in rows if r[5] == "no")
    srows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    assert [r[5].split(":")[0] for r in srows] == ["AGC", "ATTGT", "-"] and srows[2][4:] == ["0", "-", "-"]


def test_no_details_writes_only_the_summary(oracle, tmp_path):
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    p, ref, bed, reads = _panel_files(tmp_path)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "o"), data_type="hifi", anchor_len=400, seed=1,
                                 no_details=True, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                                 screener=RefScreen, discover_motifs=True, motif_engine=ref_tract_motifs)
    assert not (tmp_path / "o.details").exists()
    assert len((tmp_path / "o.NanoRepeat_motifs.tsv").read_text().split("\n")) == 6


def test_region_without_reads_and_unsupported_motif():
    class Region:
        chrom, start_pos, end_pos, repeat_unit_seq = "chr2", 10, 40, "CAGN"

    assert motifs.motif_summary_row(Region) == "chr2\t10\t40\tCAGN\t0\t-\t-\n"

    class Read:
        round3_repeat_size, left_buffer_len, right_buffer_len = 12.0, 2, 2

    class Live:
        repeat_unit_seq = "CAGN"
        read_dict = {"a": Read()}
        read_core_seq_dict = {"a": "TT" + "CCTG" * 8 + "TT"}

    calls = []
    motifs.motif_regions([Live], engine=ref_tract_motifs, scorer=lambda *a, **k: calls.append(a))
    rm = Live.read_motifs["a"]
    assert not calls and rm.call == "CCTG" and rm.fields() == ["32", "CCTG", "-", "-", "CCTG:25,C:8"]


# ---------------------------------------------------------------------------- C ABI checks
def test_tract_motifs_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    lib = capi.load()
    if lib.nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for kw in (dict(max_period=0), dict(max_period=7), dict(top_n=0), dict(top_n=9)):
        with pytest.raises(capi.NraError) as e:
            capi.tract_motifs(["CAGCAG"], **kw)
        assert e.value.code == -1, kw
    with pytest.raises(capi.NraError) as e:
        capi.tract_motifs(["CAG", "A" * 200001])
    assert e.value.code == -3
    data, off = capi.pack_reads(["CAG"])
    assert lib.nra_tract_motifs(0, -1, data, capi._ptr(off, C.c_int64), 6, 4, None, None, None, None) == -1
    assert lib.nra_tract_motifs(0, 1, data, None, 6, 4, None, None, None, None) == -1
    with pytest.raises(capi.NraError) as e:
        capi.tract_motifs(["CAGCAG", "", "A" * 200000])
    assert e.value.code == -2 and "no HIP device" in str(e.value)
