"""Motif runs without a GPU: the two restatements of the contract (plain Python over the full matrix, numpy) against each
other, the hand-worked cases, derive_runs, what the switch cost achieves on noisy reads (quality_table: DESIGN.md
section 20.3), the file formats and the FASTQ command with motif_runs=True with restatements as engines, and the C ABI's
argument checks."""
import re

import numpy as np
import pytest

from nanorepeat_amd import segments, synth
import consensus_ref
import segment_ref as R
from segment_cases import seeded_case
from structure_ref import ref_read_structure

TWO = ["ATTTT", "ATTTC"]


# ---------------------------------------------------------------------------- the two restatements
def test_numpy_restatement_equals_the_plain_one():
    sets, tracts, ts = seeded_case(300, seed=2, max_len=90)
    assert len({sum(map(len, s)) > 8 for s in sets}) == 2 and any(len(s) == 1 for s in sets)
    for W in (1, 3):
        a = R.ref_tract_segments(sets, tracts, ts, W, vectorised=False)
        b = R.ref_tract_segments(sets, tracts, ts, W, vectorised=True)
        assert R.same_result(a, b), W
    off = a["path_off"]
    assert sum(len(set(a["motif_of"][off[i]:off[i + 1]].tolist())) > 1 for i in range(300)) > 30


def test_one_motif_is_the_repeat_structure():
    rng = np.random.default_rng(4)
    motifs = [synth.rand_unit(rng, p) for p in (1, 2, 3, 5, 8, 13, 32)]
    tracts = [synth.apply_errors(rng, u * int(rng.integers(1, 60 // len(u) + 2)), "ont") for u in motifs for _ in range(6)]
    rm = np.repeat(np.arange(len(motifs)), 6)
    st = ref_read_structure(motifs, tracts, rm)
    got = R.ref_tract_segments([[u] for u in motifs], tracts, rm, 3)
    assert all(np.array_equal(got[k], st[k]) for k in ("edits", "start_phase", "path", "path_off"))
    assert not got["motif_of"].any() and not got["start_motif"].any()


# ---------------------------------------------------------------------------- hand cases
def _runs(tract, motifs, W, engine=R.plain_segment):
    e, sp, sm, path, which = engine(tract, motifs, W)
    return e, sp, sm, segments.derive_runs(path, which)


def test_hand_case_three_runs():
    """(ATTTT)5 (ATTTC)8 (ATTTT)5, W = 3: two switches and nothing else, 6 edits.  The strict tie rule puts both
    boundaries at the last distinguishing base: rows 25 and 65."""
    tract = "ATTTT" * 5 + "ATTTC" * 8 + "ATTTT" * 5
    e, sp, sm, runs = _runs(tract, TWO, 3)
    assert (e, sp, sm) == (6, 0, 0)
    assert segments.runs_text(runs, TWO) == "(ATTTT)5.0(ATTTC)8.0(ATTTT)5.0"
    assert [r.as_tuple() for r in runs] == [(0, 0, 25, 25, 0), (1, 25, 40, 40, 0), (0, 65, 25, 25, 0)]
    assert segments.units_per_motif(runs, TWO) == [10.0, 8.0]
    out = R.ref_tract_segments([TWO], [tract], [0], 3)
    assert out["edits"][0] == 6 and bytes(out["motif_of"]) == b"\0" * 25 + b"\1" * 40 + b"\0" * 25


def test_hand_case_four_foreign_units_stay_interruptions():
    """4 ATTTC units save 4 edits, fewer than 2 W = 6: one run with 4 mismatches."""
    e, _, _, runs = _runs("ATTTT" * 5 + "ATTTC" * 4 + "ATTTT" * 5, TWO, 3)
    assert e == 4 and segments.runs_text(runs, TWO) == "(ATTTT)14.0" and runs[0].edits == 4
    # 6 units save exactly 2 W: a tie keeps A; 7 units pay
    assert len(_runs("ATTTT" * 5 + "ATTTC" * 6 + "ATTTT" * 5, TWO, 3)[3]) == 1
    assert len(_runs("ATTTT" * 5 + "ATTTC" * 7 + "ATTTT" * 5, TWO, 3)[3]) == 3


def test_derive_runs_on_hand_paths():
    M, X, I = segments.MATCH, segments.MISMATCH, segments.INSERTION
    assert segments.derive_runs(b"", b"") == []
    # 3 matches in motif 0; then a mismatch, an insertion and a match followed by two deleted bases in motif 1; then motif 0
    runs = segments.derive_runs(bytes([M, M, M, X, I, M | 2 << 2, M]), bytes([0, 0, 0, 1, 1, 1, 0]))
    assert [r.as_tuple() for r in runs] == [(0, 0, 3, 3, 0), (1, 3, 3, 4, 4), (0, 6, 1, 1, 0)]
    assert segments.runs_text(runs, ["CAG", "CCGA"]) == "(CAG)1.0(CCGA)1.0(CAG)0.3"
    assert segments.units_per_motif(runs, ["CAG", "CCGA"]) == [4 / 3, 1.0]
    assert segments.runs_text([], ["CAG"]) == "-"
    assert segments.nearest_rotation("AAGGG", "AAAAG") == "AAGGG" and segments.nearest_rotation("ATTTC", "TTTTA") == "TTTCA"


def test_restatement_refuses_what_the_abi_refuses():
    for sets, W in (([TWO], 0), ([TWO], 1001), ([[]], 3), ([["ATTTT", ""]], 3), ([["ATTNT"]], 3), ([["attt"]], 3),
                    ([["A"] * 9], 3), ([["ACGT" * 8, "A"]], 3)):
        with pytest.raises(ValueError):
            R.ref_tract_segments(sets, ["ATTTT"], [0], W)
    with pytest.raises(ValueError):
        R.ref_tract_segments([TWO], ["A" * 200001], [0], 3)


# ---------------------------------------------------------------------------- what the switch cost achieves
HTT = "CAG" * 20 + "CAA" + "CAG" + "CCG" + "CCA" + "CCG" * 8 + "CCT" * 2
# (name, planted tract, motif set, planted order, inserted run (index in the order) and its units, control).  The HTT
# line's CCG run holds CCG CCA (CCG)8 and, at W >= 2, the (CCT)2 tail as well: 12 units
CASES = (("DAB1", "ATTTT" * 60 + "ATTTC" * 40 + "ATTTT" * 20, ["ATTTT", "ATTTC"], (0, 1, 0), 1, 40.0, "ATTTT" * 120),
         ("RFC1", "AAAAG" * 18 + "AAGGG" * 12 + "AAAAG" * 18, ["AAAAG", "AAGGG"], (0, 1, 0), 1, 12.0, "AAAAG" * 48),
         ("HTT", HTT, ["CAG", "CCG", "CCT"], (0, 1, 2), 1, 12.0, "CAG" * 30))
MODELS = ("hifi", "ont_q20", "ont")
COSTS = (2, 3, 4, 6)


def quality_table(seeds=40, costs=COSTS, models=MODELS, seed=23):
    """[(model, case, {W: (reads whose runs name the planted motifs in the planted order, mean absolute error of the
    inserted run's units over those reads, reads of the homogeneous control with a second run, reads whose runs begin
    with the first two planted motifs, largest absolute error of the inserted run's units)})], each over `seeds` reads
    of the planted tract and `seeds` of the control.  The fourth figure is there for the HTT line: its (CCT)2 tail saves 2 edits as a run of its own, which no W >= 2 pays
    for, so that line's first figure is 0 by the contract and the CAG, CCG order is what W decides."""
    rng = np.random.default_rng(seed)
    rows = []
    for model in models:
        for name, planted, mset, order, inserted, units, control in CASES:
            reads = [synth.apply_errors(rng, planted, model) for _ in range(seeds)]
            plain = [synth.apply_errors(rng, control, model) for _ in range(seeds)]
            cell = {}
            for W in costs:
                out = R.ref_tract_segments([mset], reads + plain, [0] * (2 * seeds), W)
                off = out["path_off"]
                runs = [segments.derive_runs(out["path"][off[i]:off[i + 1]], out["motif_of"][off[i]:off[i + 1]])
                        for i in range(2 * seeds)]
                found = [r for r in runs[:seeds] if tuple(x.motif for x in r) == order]
                if name == "HTT":                  # the error of the CCG run is taken over the reads that name CAG, CCG
                    found_err = [r for r in runs[:seeds] if tuple(x.motif for x in r)[:2] == order[:2]]
                else:
                    found_err = found
                head = sum(tuple(x.motif for x in r)[:2] == order[:2] for r in runs[:seeds])
                err = [abs(r[inserted].consumed / len(mset[r[inserted].motif]) - units) for r in found_err]
                cell[W] = (len(found), float(np.mean(err)) if err else 0.0, sum(len(r) > 1 for r in runs[seeds:]), head,
                           float(np.max(err)) if err else 0.0)
            rows.append((model, name, cell))
    return rows


def test_hifi_lines_at_the_default_switch_cost():
    """The condition of DESIGN.md section 20.3 on the hifi lines of its table (quality_table() is the whole table): at
    the default W no read of a homogeneous tract shows a second run.  The bounds for the planted lines come from the
    contract, not from a trial: a planted interior run of k units saves k edits against 2 W, so 40 and 12 units are
    found unless more than k - 2 W errors fall into them (allowed for in 2 reads of 40); a boundary sits at the last
    distinguishing base of a unit, so one error beside it moves it by one unit at most: with both ends, 2 units."""
    W = segments.DEFAULT_SWITCH_COST
    rows = quality_table(costs=(W,), models=("hifi",))
    for row in rows:
        print(row)
    assert len(rows) == 3
    for _, name, cell in rows:
        found, err, second, head, worst = cell[W]
        assert second == 0, name
        assert (head if name == "HTT" else found) >= 38 and err <= 2.0, name


# ---------------------------------------------------------------------------- the commands and the files
ENGINES = dict(consensus_engine=consensus_ref.ref_tract_consensus, structure_engine=ref_read_structure,
               segment_engine=R.ref_tract_segments)


def _motif_engine():
    import motif_ref
    return motif_ref.ref_tract_motifs


def test_fastq_command_writes_the_run_files(oracle, tmp_path, capsys):
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    from test_screen_cpu import _tree
    p = synth.motif_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "absent"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), motif_runs=False, **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), motif_runs=True,
                                           motif_engine=_motif_engine(), **ENGINES, **common)
    assert "NOTICE: motif runs: the consensus of " in capsys.readouterr().err
    # off is the command without the keyword, byte for byte, and on changes no other file
    out = (tmp_path / "absent.NanoRepeat_output.tsv").read_bytes()
    assert (tmp_path / "off.NanoRepeat_output.tsv").read_bytes() == out == (tmp_path / "on.NanoRepeat_output.tsv").read_bytes()
    absent, off, on = (_tree(tmp_path / f"{n}.details") for n in ("absent", "off", "on"))
    assert absent == off and {k: v for k, v in on.items() if not k.endswith(".read_runs.tsv")} == off
    for name in ("absent", "off"):
        assert sorted(q.name for q in tmp_path.glob(f"{name}.*")) == [f"{name}.NanoRepeat_output.tsv", f"{name}.details"]
    assert sorted(q.name for q in tmp_path.glob("on.*")) == ["on.NanoRepeat_output.tsv", "on.NanoRepeat_runs.tsv",
                                                             "on.details"]
    # the sets: BED motif first, then the discovered classes in the rotation nearest to it
    assert regions[0].motif_set[:2] == ["AAAAG", "AAGGG"] and regions[1].motif_set[:2] == ["CAG", "CCTG"]
    assert regions[2].motif_set[:2] == ["ATTTT", "ATTTC"] and regions[3].motif_set == ["TATTG"]
    assert all(len(u) > 1 for r in regions for u in r.motif_set)
    # the summary
    text = (tmp_path / "on.NanoRepeat_runs.tsv").read_text().split("\n")
    assert text[0] == "#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tMotif_Set\tAllele_Runs" and len(text) == 6
    run_re = r"(\([ACGT]+\)\d+\.\d)+"
    for line, region in zip(text[1:], regions):
        f = line.split("\t")
        assert f[3] == region.repeat_unit_seq and f[5] == ",".join(region.motif_set) and int(f[4]) == 2
        for cell, (label, tr) in zip(f[6].split("|"), region.allele_runs):
            c = cell.split(":")
            assert int(c[0]) == label and int(c[1]) >= 6 and re.fullmatch(run_re, c[3])
            assert [x.split("=")[0] for x in c[2].split(",")] == region.motif_set
            assert c[3] == segments.runs_text(tr.runs, region.motif_set)
    dab = regions[2]
    assert [dab.motif_set[r.motif] for r in dab.allele_runs[1][1].runs] == ["ATTTT", "ATTTC", "ATTTT"]
    assert all(len(tr.runs) == 1 for _, tr in regions[3].allele_runs) and len(dab.allele_runs[0][1].runs) == 1
    # the per-read files
    for region in regions:
        lines = open(f"{region.out_prefix}.read_runs.tsv").read().split("\n")
        assert lines[0] == f"##RepeatRegion={region.to_unique_id()}" and lines[1] == "##Motifs=" + ",".join(region.motif_set)
        assert lines[2] == f"##Switch_Cost={segments.DEFAULT_SWITCH_COST}"
        assert lines[3] == "#Read_Name\tAllele_ID\tTract_Len\tEdits\tRuns\tUnits_Per_Motif"
        body = [l.split("\t") for l in lines[4:] if l]
        assert [b[0] for b in body] == [n for n, _ in segments._ordered_reads(region)] and len(body) == len(region.read_runs)
        for b in body:
            tr = region.read_runs[b[0]]
            assert int(b[2]) == tr.tract_len and int(b[3]) == tr.edits and re.fullmatch(run_re, b[4])
            assert sum(r.bases for r in tr.runs) == tr.tract_len
    # the caller's motifs, and a switch cost of its own
    key = regions[2].to_unique_id()
    again = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "own"), motif_runs=True, switch_cost=6,
                                         segment_motifs={key: ["ATTTC", "atttg"]}, motif_engine=_motif_engine(),
                                         **ENGINES, **common)
    assert again[2].motif_set == ["ATTTT", "ATTTC", "ATTTG"] and again[0].motif_set == regions[0].motif_set
    assert "##Switch_Cost=6\n" in open(f"{again[2].out_prefix}.read_runs.tsv").read()
    with pytest.raises(ValueError):
        segments.region_motif_set(regions[2], ["ATNT"])
    with pytest.raises(ValueError):
        segments.region_motif_set(regions[2], ["ACGTACGTAC", "ACGTACGTAA", "ACGTACGTCC"])


def test_a_region_whose_motif_cannot_be_segmented_gets_dashes():
    class Region:
        repeat_unit_seq = "ACGTN"
    assert segments.region_motif_set(Region) is None
    Region.repeat_unit_seq = "ACGT" * 8 + "A"
    assert segments.region_motif_set(Region) is None
    assert segments.TractRuns(17).fields() == ["17", "-", "-", "-"]


# ---------------------------------------------------------------------------- C ABI
def test_symbol_is_declared_and_exported(capi):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int nra_tract_segments(" in open(os.path.join(root, "include", "nanorepeat_amd.h")).read()
    assert "nra_tract_segments" in capi.EXPORTS and hasattr(capi.load(), "nra_tract_segments")
    assert capi.load().nra_abi_version() == 4
    assert (segments.MAX_MOTIFS, segments.MAX_STATES, segments.MAX_TRACT_LEN, segments.MAX_SWITCH_COST) == \
        (R.MAX_MOTIFS, R.MAX_STATES, R.MAX_TRACT_LEN, R.MAX_SWITCH_COST)


def test_argument_errors_come_back_without_a_device(capi):
    """Arguments are checked before the device is touched: the same codes with and without a GPU.  With good arguments
    and no device the call returns NRA_E_DEVICE."""
    for sets, tracts, W, code in (([TWO], ["ATTTT"], 0, -1), ([TWO], ["ATTTT"], -3, -1), ([[]], ["ATTTT"], 3, -1),
                                  ([["ATTTT", ""]], ["ATTTT"], 3, -1), ([["ATTNT"]], ["ATTTT"], 3, -1),
                                  ([["attt"]], ["ATTTT"], 3, -1), ([["A"] * 9], ["ATTTT"], 3, -3),
                                  ([["ACGT" * 8, "A"]], ["ATTTT"], 3, -3), ([["A" * 33]], ["ATTTT"], 3, -3),
                                  ([TWO], ["A" * 200001], 3, -3), ([TWO], ["ATTTT"], 1001, -3)):
        with pytest.raises(capi.NraError) as e:
            capi.tract_segments(sets, tracts, [0] * len(tracts), W)
        assert e.value.code == code, (sets, W)
    with pytest.raises(capi.NraError) as e:
        capi.tract_segments([TWO], ["ATTTT"], [1], 3)
    assert e.value.code == -1
    if capi.load().nra_device_count() <= 0:
        with pytest.raises(capi.NraError) as e:
            capi.tract_segments([TWO], ["ATTTTATTTC", ""], [0, 0], 3)
        assert e.value.code == -2 and "no HIP device" in str(e.value)
