"""The round-3 alignment file (alignments.py) with the oracle as path aligner and scorer: no device."""
import sys

import pytest

from nanorepeat_amd import alignments, phasing, pipeline, round3, synth
from paths_cases import paths_panel, paf_rows, spans_fit_cigar
from screen_ref import RefScreen
from test_screen_cpu import _tree


def test_smallest_best_k():
    assert alignments.smallest_best_k(10, [50, 90, 90, 70], 90) == 11
    assert alignments.smallest_best_k(0, [-1, -1], 0) is None
    assert alignments.smallest_best_k(7, [], 3) is None


def test_k_on_a_constructed_tie_is_the_smallest_not_the_mean(oracle):
    """Two candidates tie: the size is their mean, 11.5, and the template is the one of k = 11."""
    import numpy as np
    rng = np.random.default_rng(5)
    region = round3.RepeatRegion("chr1\t100\t130\tCAG\n")
    region.left_anchor_seq, region.right_anchor_seq = synth.rand_seq(rng, 120), synth.rand_seq(rng, 120)
    core = region.left_anchor_seq[-50:] + "CAG" * 11 + "CA" + region.right_anchor_seq[:50]
    for name, status in (("tie", 0), ("fallback", 1)):
        read = round3.Read(name, 11.0)
        read.round3_status, read.round3_best_score = status, 90
        read.round3_repeat_size = 11.5
        alignments.keep_candidates(read, 10, np.array([50, 90, 90, 70], np.int32))
        region.read_dict[name] = read
        region.read_core_seq_dict[name] = core + "\n"
    alignments.alignment_regions([region], engine=oracle.align_pairs_cigar)
    (name, k, q, tlen, res), = region.round3_alignments
    assert (name, k, q, tlen) == ("tie", 11, core, 240 + 33)
    row = alignments.alignment_text(region).rstrip("\n").split("\t")
    assert row[0] == "tie" and row[5] == "chr1-100-130-CAG|k=11" and row[-1] == "rs:f:11.5"
    want = oracle.align_cigar(core, alignments.template_of(region, 11))
    assert f"AS:i:{want['score']}" in row and f"cg:Z:{want['cigar']}" in row


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("paths")
    p = paths_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp))
    common = dict(data_type="hifi", anchor_len=500, seed=3, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "on"), read_alignments=True,
                                           path_aligner=oracle.align_pairs_cigar, **common)
    return tmp, (ref, bed, reads), common, regions


def test_switch_off_writes_no_file_and_the_other_files_are_identical(runs):
    tmp, _, _, _ = runs
    on, off = _tree(tmp / "on.details"), _tree(tmp / "off.details")
    assert not any(k.endswith(".round3.paf") for k in off)
    assert sum(k.endswith(".round3.paf") for k in on) == 3
    assert {k: v for k, v in on.items() if not k.endswith(".round3.paf")} == off
    assert (tmp / "on.NanoRepeat_output.tsv").read_bytes() == (tmp / "off.NanoRepeat_output.tsv").read_bytes()


def test_rows_follow_phased_reads_order_and_hold_the_oracle_alignment(runs, oracle):
    _, _, _, regions = runs
    for region in regions:
        rows = paf_rows(f"{region.out_prefix}.round3.paf")
        phased = [l.split("\t")[0] for l in open(f"{region.out_prefix}.phased_reads.txt") if not l.startswith("#")]
        ok = {n for n, r in region.read_dict.items() if r.round3_status == 0}
        others = sorted(ok - set(phased))
        assert [p.qname for p, _ in rows] == [n for n in phased if n in ok] + others and len(rows) == 6
        for p, rs in rows:
            read = region.read_dict[p.qname]
            k = int(p.tname.rsplit("|k=", 1)[1])
            lo, cand = read.round3_candidates
            assert cand[k - lo] == read.round3_best_score and read.round3_best_score not in cand[:k - lo]
            assert p.align_score == read.round3_best_score and rs == f"{read.round3_repeat_size:.1f}"
            o = oracle.align_cigar(region.read_core_seq_dict[p.qname].strip(), alignments.template_of(region, k))
            assert (p.cigar, p.tstart, p.tend, p.qstart, p.qend) == (o["cigar"], o["tstart"], o["tend"], o["qstart"], o["qend"])
            assert spans_fit_cigar(p)


def test_pairs_beyond_the_limits_are_left_out_and_counted(runs, oracle, monkeypatch, capsys):
    tmp, (ref, bed, reads), common, before = runs
    cores = sorted(len(c.strip()) for c in before[0].read_core_seq_dict.values())
    limit = (cores[2] + cores[3]) // 2                         # between the cores of the two GAA alleles
    assert cores[2] < limit < cores[3]
    monkeypatch.setattr(alignments, "MAX_QUERY", limit)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "cut"), read_alignments=True,
                                           path_aligner=oracle.align_pairs_cigar, **common)
    err = capsys.readouterr().err
    left = [len(r.round3_alignments_left_out) for r in regions]
    assert left == [sum(len(r.read_core_seq_dict[n].strip()) > limit for n, rd in r.read_dict.items() if rd.round3_status == 0)
                    for r in regions] and left[0] == 3
    for region, n in zip(regions, left):
        note = f"NOTICE: {region.to_unique_id()}: {n} read(s) beyond the path call's limits"
        assert (err.count(note) == 1) if n else (f"NOTICE: {region.to_unique_id()}" not in err)
        assert len(paf_rows(f"{region.out_prefix}.round3.paf")) == 6 - n
    assert _tree(tmp / "cut.details").keys() == _tree(tmp / "on.details").keys()


def test_no_details_writes_nothing(runs, oracle):
    tmp, (ref, bed, reads), common, _ = runs

    def never(*a, **k):
        raise AssertionError("the path aligner was called")
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "nd"), read_alignments=True, no_details=True,
                                 path_aligner=never, **common)
    assert not (tmp / "nd.details").exists()
    assert (tmp / "nd.NanoRepeat_output.tsv").read_bytes() == (tmp / "off.NanoRepeat_output.tsv").read_bytes()
