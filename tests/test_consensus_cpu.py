"""Allele consensus without a GPU: the two restatements of the contract (full matrix, banded with the widening rule)
against each other, what the rule achieves on noisy reads (conditions, not numbers), the BAM and FASTQ commands with
allele_consensus=True on a small panel with the restatements as engines, and the C ABI's argument checks."""
import ctypes as C
import sys

import numpy as np
import pytest

from nanorepeat_amd import consensus, structure, synth
import consensus_ref as R
from consensus_cases import edge_groups, seeded_alleles
from structure_ref import ref_read_structure


def _dist(a, b):
    return int(R.full_matrix(R.encode(a), R.encode(b))[-1, -1])


# ---------------------------------------------------------------------------- the two restatements
def test_banded_restatement_equals_the_full_matrix():
    seen_left = seen_one = seen_empty = seen_open = False
    for q, (groups, max_dist) in enumerate(edge_groups()):
        full = R.ref_tract_consensus(groups, max_dist=max_dist, banded=False)
        band = R.ref_tract_consensus(groups, max_dist=max_dist, banded=True)
        assert R.same_result(full, band), q
        seen_left |= bool((full["left_out"] > 0).any())
        seen_open |= bool(((full["converged"] == 0) & (full["n_rounds"] > 0)).any())
        seen_one |= any(len([t for t in g if t]) == 1 for g in groups)
        seen_empty |= bool((full["n_rounds"] == 0).any())
    assert seen_left and seen_one and seen_empty and seen_open
    groups = [g for g in seeded_alleles(60, seed=31, max_len=500)]
    assert R.same_result(R.ref_tract_consensus(groups, banded=False), R.ref_tract_consensus(groups, banded=True))
    assert R.same_result(R.ref_tract_consensus(groups, max_dist=25, max_rounds=2, banded=False),
                         R.ref_tract_consensus(groups, max_dist=25, max_rounds=2, banded=True))


def test_hand_cases():
    # the distances around max_dist: 11 and 12 substitutions vote, 13 and 30 are left out
    groups, max_dist = edge_groups()[1]
    out = R.ref_tract_consensus(groups, max_dist=max_dist, banded=False)
    assert (out["voted"][0], out["left_out"][0], out["converged"][0]) == (5, 2, 1)
    assert out["consensus"][0] == groups[0][3]
    # one read: its ACGT bases after one round; two reads: every vote ties and the backbone's own base wins
    out = R.ref_tract_consensus([["CAGNCAG"], ["CAGCAG", "CATCAGG"], ["NN"], []], banded=False)
    assert out["consensus"] == ["CAGCAG", "CAGCAG", "", ""]
    assert list(out["n_rounds"]) == [1, 1, 1, 0] and list(out["converged"]) == [1, 1, 1, 0]
    assert list(out["support"][0]) == [1] * 6 and list(out["support"][1]) == [2, 2, 1, 2, 2, 2]
    # all reads left out: the round-0 backbone stays, not converged, no support
    out = R.ref_tract_consensus([["AAAAAAAA", "CCCCCCCC", "GGGGGGGG"]], max_dist=0, banded=True)
    assert out["consensus"] == ["CCCCCCCC"] and (out["voted"][0], out["left_out"][0], out["converged"][0]) == (1, 2, 1)
    out = R.ref_tract_consensus([["AAAAAAAAN", "CCCCCCCCN", "GGGGGGGGN"]], max_dist=0, banded=True)
    assert out["consensus"] == ["CCCCCCCC"] and out["converged"][0] == 0 and out["n_rounds"][0] == 1
    assert out["voted"][0] == 0 and out["left_out"][0] == 3 and not out["support"][0].any()
    # an insertion most reads share enters through a slot, one base per round
    out = R.ref_tract_consensus([["CAGCAGCAG", "CAGTTCAGCAG", "CAGTTCAGCAG", "CAGTTCAGCAG", "CAGCAGCAG"][::-1]],
                                banded=False)
    assert out["consensus"] == ["CAGTTCAGCAG"] and out["converged"][0] == 1


# ---------------------------------------------------------------------------- what the rule achieves
LINES = (("TATTG", 40, 6), ("TATTG", 40, 12), ("TATTG", 40, 30), ("CAG", 100, 12), ("GAA", 200, 20), ("AAGGG", 60, 8),
         ("A", 40, 12))


def quality_table(seed=18, alleles_per_line=3):
    """[(model, unit, k, reads, consensus distance, best read, median read, [rounds], all converged)], distances to
    the true tract summed over the line's alleles."""
    rng = np.random.default_rng(seed)
    rows = []
    for model in ("ont", "hifi"):
        for unit, k, m in LINES:
            truth = unit * k
            cons = best = med = 0
            rounds, conv = [], True
            for _ in range(alleles_per_line):
                reads = [synth.apply_errors(rng, truth, model) for _ in range(m)]
                out = R.ref_tract_consensus([reads], banded=True)
                d = sorted(_dist(r, truth) for r in reads)
                cons += _dist(out["consensus"][0], truth)
                best += d[0]
                med += d[len(d) // 2]
                rounds.append(int(out["n_rounds"][0]))
                conv &= bool(out["converged"][0])
            rows.append((model, unit, k, m, cons, best, med, rounds, conv))
    return rows


def test_consensus_is_closer_to_the_truth_than_the_best_read():
    rows = quality_table()
    for row in rows:
        print(row)
    assert all(row[8] for row in rows)                                   # every allele converges within max_rounds
    for model in ("ont", "hifi"):
        mine = [row for row in rows if row[0] == model and len(row[1]) > 1]
        assert len(mine) == 6
        assert sum(row[4] for row in mine) < sum(row[5] for row in mine), model


def test_planted_interruptions_come_back(oracle, tmp_path):
    """The planted alleles of synth.structure_panel (HiFi, 8 reads each, its own seed),
    through the FASTQ command with the restatements as engines: every consensus is the planted tract, so its
    interruptions sit at the planted units."""
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    p = synth.structure_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), data_type="hifi", anchor_len=1000,
                                           seed=3, allele_consensus=True, aligner=oracle.align_pairs,
                                           scorer=oracle.round3_1d, screener=RefScreen,
                                           consensus_engine=R.ref_tract_consensus, structure_engine=ref_read_structure)
    for region, tracts, inter in zip(regions, PLANTED, p["planted"]):
        assert [ac.sequence for ac in region.allele_consensus] == tracts
        for ac, want in zip(region.allele_consensus, inter):
            assert ac.converged == 1 and ac.left_out == 0 and ac.voted == 8
            assert [(b, k) for k, b in ac.interruptions] == want
            assert ac.pure_units == len(ac.sequence) // len(region.repeat_unit_seq) - len(want)


PLANTED = [["CAG" * 17 + "CAA" + "CAG", "CAG" * 36 + "CAA" + "CAG"],
           ["CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * m for m in (10, 28)],
           ["TATTG" * 12, "TATTG" * 30]]


# ---------------------------------------------------------------------------- the commands
def _run(tmp_path, command, oracle, extra):
    from test_screen_cpu import _tree
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  **extra)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    src = str(tmp_path / ("in.bam" if command.__name__ == "quantify_from_bam" else "in.fastq"))
    command(src, ref, bed, str(tmp_path / "absent"), **common)
    command(src, ref, bed, str(tmp_path / "off"), allele_consensus=False, **common)
    regions = command(src, ref, bed, str(tmp_path / "on"), allele_consensus=True,
                      consensus_engine=R.ref_tract_consensus, structure_engine=ref_read_structure, **common)
    out = (tmp_path / "absent.NanoRepeat_output.tsv").read_bytes()
    assert (tmp_path / "off.NanoRepeat_output.tsv").read_bytes() == out
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == out
    absent, off, on = (_tree(tmp_path / f"{n}.details") for n in ("absent", "off", "on"))
    assert absent == off and {k: v for k, v in on.items() if not k.endswith(".allele_consensus.fasta")} == off
    for name in ("absent", "off"):
        assert sorted(p.name for p in tmp_path.glob(f"{name}.*")) == [f"{name}.NanoRepeat_output.tsv", f"{name}.details"]
    assert sorted(p.name for p in tmp_path.glob("on.*")) == ["on.NanoRepeat_consensus.tsv", "on.NanoRepeat_output.tsv",
                                                             "on.details"]
    return regions, on, (tmp_path / "on.NanoRepeat_consensus.tsv").read_text(), out.decode()


def _check(regions, tree, summary, output):
    files = sorted(k for k in tree if k.endswith(".allele_consensus.fasta"))
    assert len(files) == 2                                       # the third region has no alleles
    assert summary.startswith("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Consensus\n")
    srows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    orows = [l.split("\t") for l in output.split("\n") if l]
    assert len(srows) == 3 and srows[2][4:] == ["0", "-"]
    for region, srow, orow in zip(regions[:2], srows, orows):
        p = len(region.repeat_unit_seq)
        sizes = [float(a.split(";")[0]) for a in orow[7].split("|")[1:]]          # Allele_Repeat_Size, phasing order
        text = tree[[k for k in files if region.repeat_unit_seq in k][0]].decode()
        records = [r.split("\n", 1) for r in text.split(">")[1:]]
        assert len(records) == len(sizes) == int(srow[4]) == 2 and srow[:4] == orow[:4]
        for (head, seq), cell, size, ac in zip(records, srow[5].split("|"), sizes, region.allele_consensus):
            f = dict(x.split("=") for x in head.split()[1:])
            seq = seq.replace("\n", "")
            assert head.split()[0] == f"allele{ac.allele_id}" and all(len(l) <= 80 for l in text.split("\n"))
            assert seq == ac.sequence and int(f["len"]) == len(seq) and set(seq) <= set("ACGT")
            assert int(f["reads"]) + int(f["left_out"]) == ac.n_reads >= 5 and f["converged"] == "1"
            assert abs(float(f["units"]) - size) <= 1.0, (f, size)
            label, voted, left, ln, units, support, purity, inter = cell.split(":", 7)
            assert (int(label), int(voted), int(left), int(ln)) == (ac.allele_id, ac.voted, ac.left_out, len(seq))
            assert units == f["units"] and 0.0 < float(support) <= 1.0 and 0.9 < float(purity) <= 1.0


def test_bam_command_writes_consensus_files(oracle, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    _check(*_run(tmp_path, pipeline.quantify_from_bam, oracle, {}))
    assert "allele consensus" not in capsys.readouterr().err            # every allele converged, no read left out


def test_fastq_command_writes_consensus_files(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    from test_screen_cpu import _bam_reads, _write_fastq
    from screen_ref import RefScreen
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    _write_fastq(tmp_path / "in.fastq", _bam_reads(tmp_path))
    _check(*_run(tmp_path, pipeline.quantify_from_reads, oracle, dict(screener=RefScreen)))


def test_no_details_writes_only_the_summary(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"),
                               str(tmp_path / "o"), data_type="ont_q20", anchor_len=400, seed=1, no_details=True,
                               aligner=oracle.align_pairs, scorer=oracle.round3_1d, allele_consensus=True,
                               consensus_engine=R.ref_tract_consensus, structure_engine=ref_read_structure)
    assert not (tmp_path / "o.details").exists()
    assert len((tmp_path / "o.NanoRepeat_consensus.tsv").read_text().split("\n")) == 5


def test_unsupported_motif_keeps_its_consensus_and_notice_counts(capsys):
    class Q:
        def __init__(self, allele_id):
            self.allele_id = allele_id

    class Read:
        round3_repeat_size, left_buffer_len, right_buffer_len = 4.0, 2, 2

    class Region:
        repeat_unit_seq, chrom, start_pos, end_pos = "CAGN", "chr1", 10, 30
        read_dict = {n: Read() for n in "abc"}
        read_core_seq_dict = {"a": "TTCAGCAGTT", "b": "TTCAGCAGTT", "c": "TTGGGGGGGGGGGGTT"}

    res = consensus.phasing.results_of(Region)
    res.quantified_allele_list = [object()]
    res.quantified_read_dict = {n: Q(1) for n in "abc"}
    calls = []
    consensus.consensus_regions([Region], engine=R.ref_tract_consensus, max_dist=3,
                                structure_engine=lambda *a, **k: calls.append(a))
    ac, = Region.allele_consensus
    assert not calls and ac.sequence == "CAGCAG" and ac.purity is None and (ac.voted, ac.left_out) == (2, 1)
    assert consensus.consensus_summary_row(Region) == "chr1\t10\t30\tCAGN\t1\t1:2:1:6:1.5:1.00:-:-\n"
    assert consensus.report_unsettled_alleles([Region]) == (0, 1)
    assert "1 left 1 read(s) out" in capsys.readouterr().err


# ---------------------------------------------------------------------------- C ABI checks
def test_tract_consensus_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    lib = capi.load()
    if lib.nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for kw, code in ((dict(max_dist=-1), -1), (dict(max_dist=1001), -3), (dict(max_rounds=0), -1),
                     (dict(max_rounds=65), -3)):
        with pytest.raises(capi.NraError) as e:
            capi.tract_consensus([["CAGCAG"]], **kw)
        assert e.value.code == code, kw
    with pytest.raises(capi.NraError) as e:
        capi.tract_consensus([["A" * 200001]])
    assert e.value.code == -3
    goff = np.array([0, 2], np.int64)
    data, off = capi.pack_reads(["CAG"])
    res, coff = np.zeros(4, np.int32), np.zeros(2, np.int64)
    args = (1, data, capi._ptr(off, C.c_int64), 100, 8, 0, None, None, capi._ptr(coff, C.c_int64),
            capi._ptr(res, C.c_int32), None)
    assert lib.nra_tract_consensus(0, 1, capi._ptr(goff, C.c_int64), *args) == -1      # groups beyond the tracts
    assert lib.nra_tract_consensus(0, 1, None, *args) == -1
    with pytest.raises(capi.NraError) as e:
        capi.tract_consensus([["CAGCAG", "CAGCAA"], []])
    assert e.value.code == -2 and "no HIP device" in str(e.value)
