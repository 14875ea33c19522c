"""Flank haplotypes without a GPU: the two restatements of the contract (full matrix, banded with the widening rule)
against each other, hand cases, the invariants of the rule (permuted rows), the FASTQ command with flank_phase=True on
synth.flank_panel() with the restatements as engines, the files, the switch off, and the C ABI's argument checks."""
import re

import numpy as np
import pytest

from nanorepeat_amd import synth
import flank_ref as R
from flank_cases import corner_cases, seeded_groups


# ---------------------------------------------------------------------------- the two restatements
def test_banded_restatement_equals_the_full_matrix():
    seen = dict(no_rows=0, all_left=0, no_site=0, cut=0, undecided=0, silent_hap=0, phased=0, left_out_side=0,
                absent_side=0, end_mod=set())
    for q, (groups, bbs, kw) in enumerate(corner_cases()):
        full = R.ref_flank_phase(groups, bbs, banded=False, **kw)
        band = R.ref_flank_phase(groups, bbs, banded=True, **kw)
        assert R.same_result(full, band), q
        assert (full["n0"] >= full["n1"]).all()
        m = np.array([len(g) for g in groups])
        assert np.array_equal(full["n0"] + full["n1"] + full["undecided"] + full["left_out"], m)
        seen["no_rows"] += int((m == 0).sum())
        seen["all_left"] += int(((m > 0) & (full["left_out"] == m)).sum())
        seen["no_site"] += int(((full["left_out"] < m) & (full["n_sites"] == 0)).sum())
        seen["cut"] += int("max_sites" in kw and (full["n_sites"] == kw["max_sites"]).all() and kw["max_sites"] < 9)
        seen["undecided"] += int((full["undecided"] > 0).sum())
        seen["silent_hap"] += sum(int(((s[:, 3:7].sum(axis=1) == 0) | (s[:, 7:11].sum(axis=1) == 0)).any())
                                  for s in full["sites"] if len(s))
        seen["phased"] += int(full["phased"].sum())
        for d, e, lab in zip(full["dist"], full["end"], full["label"]):
            seen["left_out_side"] += int((d == -1).sum())
            seen["absent_side"] += int((d == -2).sum())
            seen["end_mod"] |= {int(x) % 16 for x in e[d >= 0]}
            assert ((e == 0) | (d >= 0)).all() and np.array_equal(lab == -1, (d < 0).all(axis=1))
    assert all(seen.values()) and {15, 0, 1} <= seen["end_mod"], seen
    groups, bbs = seeded_groups(40, seed=31, max_len=300)
    for kw in ({}, dict(max_dist=25, min_sites=1, min_count=2, skip=3)):
        assert R.same_result(R.ref_flank_phase(groups, bbs, banded=False, **kw),
                             R.ref_flank_phase(groups, bbs, banded=True, **kw))


def test_hand_cases():
    bl, br = "ACGTTGCAAGGCTTAACCGGATATCGCG", "TTGACCAGTGCATGCAAGTC"
    alt_l, alt_r = bl[:9] + "T" + bl[10:], br[:12] + "A" + br[13:]            # L9: G/T, R12: T/A
    rows = [(bl, br)] * 4 + [(alt_l, alt_r)] * 3 + [(bl[:6], "")]
    out = R.ref_flank_phase([rows], [(bl, br)], skip=5, min_sites=2, banded=False)
    assert (out["phased"][0], out["n0"][0], out["n1"][0], out["undecided"][0], out["n_sites"][0]) == (1, 4, 3, 1, 2)
    assert list(out["label"][0]) == [0] * 4 + [1] * 3 + [2]
    assert [int(s[0]) for s in out["sites"][0]] == [9, len(bl) + 12]         # group columns: the right side from tL on
    assert out["sites"][0][0].tolist() == [9, 2, 3, 0, 0, 4, 0, 0, 0, 0, 3, 1]
    assert out["dist"][0].tolist() == [[0, 0]] * 4 + [[1, 1]] * 3 + [[0, -2]]
    assert out["end"][0].tolist() == [[len(bl), len(br)]] * 7 + [[6, 0]]
    assert out["site_sym"][0][:, 7].tolist() == [R.NOT_COVERED, R.NOT_COVERED]
    # the same sites inside skip are not called; one site is too few for min_sites 2
    out = R.ref_flank_phase([rows], [(bl, br)], skip=10, min_sites=2)
    assert (out["phased"][0], out["n_sites"][0]) == (0, 1) and int(out["sites"][0][0][0]) == len(bl) + 12
    out = R.ref_flank_phase([rows], [(bl, br)], skip=13)
    assert out["n_sites"][0] == 0 and list(out["label"][0]) == [0] * 8
    # a free end: the segment stops inside the side and the columns beyond are not covered
    out = R.ref_flank_phase([[(bl[:10] + "N", "")]], [(bl, br)], skip=0)
    assert out["dist"][0].tolist() == [[1, -2]] and out["end"][0].tolist() == [[10, 0]]    # a tie for j*: the smaller
    # left out by max_dist on its only side: label -1
    out = R.ref_flank_phase([[("TTTTTTTTTT", "")] + rows], [(bl, br)], max_dist=3, skip=5)
    assert out["label"][0][0] == -1 and out["dist"][0][0].tolist() == [-1, -2] and out["left_out"][0] == 1
    for bad in (dict(min_count=0), dict(min_share_pct=101), dict(max_sites=4097), dict(max_iter=0), dict(max_dist=501),
                dict(skip=-1)):
        with pytest.raises(ValueError):
            R.ref_flank_phase([rows], [(bl, br)], **bad)
    with pytest.raises(ValueError):
        R.ref_flank_phase([rows], [(bl, "ACNT")])


def test_permuting_the_rows_permutes_the_labels():
    rng = np.random.default_rng(8)
    groups, bbs = seeded_groups(30, seed=33, max_len=300)
    for groups, bbs, kw in [(groups, bbs, {})] + corner_cases()[-4:]:
        one = R.ref_flank_phase(groups, bbs, **kw)
        perms = [rng.permutation(len(g)) for g in groups]
        two = R.ref_flank_phase([[g[j] for j in p] for g, p in zip(groups, perms)], bbs, **kw)
        for k in R.RES_FIELDS:
            assert np.array_equal(one[k], two[k]), k
        for g, p in enumerate(perms):
            for k in ("label", "dist", "end"):
                assert np.array_equal(two[k][g], one[k][g][p]), k
            assert np.array_equal(two["sites"][g], one["sites"][g])
            assert np.array_equal(two["site_sym"][g], one["site_sym"][g][:, p])


# ---------------------------------------------------------------------------- the commands
SUMMARY_COLUMNS = ("#Chrom Start End Motif Phased Num_Sites Num_Supported Reads_a Reads_b Undecided Left_Out "
                   "Allele_By_Haplotype Spanning_a Median_Size_a Partial_a Max_Min_Repeat_Size_a Unspanned_a Spanning_b "
                   "Median_Size_b Partial_b Max_Min_Repeat_Size_b Unspanned_b").split()
READ_COLUMNS = ("#Read_Name Kind Size_Allele Repeat_Size Min_Repeat_Size Haplotype Site_Symbols Left_Dist Left_End "
                "Right_Dist Right_End").split()


def check_planted_panel(p, regions, flank_skip=20):
    """synth.flank_panel comes back: every read on its planted haplotype, the equal-size pair phased, the allele no read
    spans on a haplotype of its own, the control not phased, and no site nearer to the repeat than flank_skip."""
    assert len(regions) == 5
    for g, region in enumerate(regions):
        fp = region.flank_phase
        assert sorted(fp.read_names) == sorted(n for n, (rg, _) in p["truth"].items() if rg == g), g
        assert [p["kind"][n] for n in fp.read_names] == fp.kinds
        for name in fp.site_names():
            side, o = re.fullmatch(r"([LR])(\d+):[ACGT]/[ACGT]", name).groups()
            assert int(o) >= flank_skip
            assert g == 3 or int(o) in p["planted"][g][side == "R"], (g, name)
        if g == 3:
            assert fp.phased == 0
            continue
        assert fp.phased == 1 and fp.undecided == 0 and fp.left_out == 0 and fp.n_supported >= 2, g
        hap = np.array([p["haplotype"][n] for n in fp.read_names])
        assert np.array_equal(fp.labels, hap) or np.array_equal(fp.labels, 1 - hap), g
    # region 1: one size allele on two haplotypes
    fp = regions[1].flank_phase
    assert fp.allele_by_haplotype == [(1, 8, 8)]
    assert [hc.spanning for hc in fp.haplotypes] == [8, 8] and all(hc.median_size == 16.0 for hc in fp.haplotypes)
    # region 0: the size phasing and the flanks agree
    assert sorted(regions[0].flank_phase.allele_by_haplotype) in ([(1, 0, 8), (2, 8, 0)], [(1, 8, 0), (2, 0, 8)])
    # region 2: the long allele's haplotype has no spanning read and shows more than the short allele
    fp = regions[2].flank_phase
    long_, short = sorted(fp.haplotypes, key=lambda hc: hc.spanning)
    assert (long_.spanning, long_.partial, long_.unspanned, long_.median_size) == (0, 16, 1, None)
    assert (short.spanning, short.partial, short.unspanned, short.max_min_repeat_size) == (12, 0, 0, None)
    assert long_.max_min_repeat_size > 100 > short.median_size == 18.0
    assert [hc.unspanned for r in regions for hc in r.flank_phase.haplotypes].count(1) == 1


@pytest.fixture(scope="module")
def panel_run(oracle, tmp_path_factory):
    """The FASTQ command on synth.flank_panel() three times: without the keyword, with flank_phase=False and with
    flank_phase=True (partial_reads=True throughout)."""
    import contextlib
    import io
    from nanorepeat_amd import pipeline
    from screen_partial_ref import RefScreenPartial
    from extend_ref import ref_extend_tracts
    tmp = tmp_path_factory.mktemp("flank")
    p = synth.flank_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp))
    common = dict(data_type="hifi", anchor_len=1000, seed=3, partial_reads=True, aligner=oracle.align_pairs,
                  scorer=oracle.round3_1d, screener=RefScreenPartial, extension_engine=ref_extend_tracts)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "absent"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "off"), flank_phase=False, **common)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "on"), flank_phase=True,
                                               flank_engine=R.ref_flank_phase, **common)
    return p, regions, tmp, err.getvalue()


def test_planted_panel_comes_back(panel_run):
    p, regions, _, err = panel_run
    check_planted_panel(p, regions)
    notices = [l for l in err.split("\n") if "flank haplotype" in l]
    assert len(notices) == 1 and regions[2].to_unique_id() in notices[0] and "has no spanning read and 16 one-anchor" in notices[0]


def check_files(regions, out_prefix):
    from nanorepeat_amd import split
    summary = open(f"{out_prefix}.NanoRepeat_flank_phase.tsv").read().split("\n")
    assert summary[0].split("\t") == SUMMARY_COLUMNS and len(summary) == len(regions) + 2 and summary[-1] == ""
    for line, region in zip(summary[1:], regions):
        f = line.split("\t")
        fp = region.flank_phase
        assert len(f) == len(SUMMARY_COLUMNS) and f[3] == region.repeat_unit_seq
        assert [int(x) for x in f[4:11]] == [fp.phased, fp.n_sites, fp.n_supported, fp.n0, fp.n1, fp.undecided, fp.left_out]
        assert all(re.fullmatch(r"\d+:\d+/\d+", c) for c in f[11].split(","))
        assert f[12:] == fp.haplotypes[0].fields() + fp.haplotypes[1].fields()
        text = open(f"{region.out_prefix}.flank_phase.tsv").read().split("\n")
        assert text[0] == f"##RepeatRegion={region.to_unique_id()}" and text[1] == "##Flank_Len=3000"
        assert text[2] == "##Sites=" + (",".join(fp.site_names()) or "-") and text[3].split("\t") == READ_COLUMNS
        body = [l.split("\t") for l in text[4:] if l]
        assert [l[0] for l in body] == fp.read_names and [l[1] for l in body] == fp.kinds
        for i, l in enumerate(body):
            assert len(l) == len(READ_COLUMNS) and l[5] in ("a", "b", "-", ".") and l[5] == fp.haplotype_of(i)
            assert len(l[6]) == max(1, fp.n_sites) and set(l[6]) <= set(split.SYMBOLS)
            assert (l[1] == "spanning") == (l[3] != "-") and (l[1] == "spanning") == (l[4] == "-")
            assert [int(x) for x in l[7:]] == [fp.dist[i, 0], fp.end[i, 0], fp.dist[i, 1], fp.end[i, 1]]
            assert (l[1] != "left" or l[9] == "-2") and (l[1] != "right" or l[7] == "-2")


def test_file_formats(panel_run):
    _, regions, tmp, _ = panel_run
    check_files(regions, str(tmp / "on"))
    # the symbols of region 2: the long allele's left-anchored reads cover no right site and the other way round
    fp = regions[2].flank_phase
    n_left = sum(c < fp.t_left for c in fp.sites[:, 0])
    for i, kind in enumerate(fp.kinds):
        sym = fp.symbols_of(i)
        assert kind != "left" or set(sym[n_left:]) == {"."}
        assert kind != "right" or set(sym[:n_left]) == {"."}


def test_off_is_byte_for_byte_the_command_without_the_keyword(panel_run):
    from test_screen_cpu import _tree
    _, _, tmp, _ = panel_run
    absent, off, on = (_tree(tmp / f"{n}.details") for n in ("absent", "off", "on"))
    assert absent and absent == off
    assert {k: v for k, v in on.items() if not k.endswith(".flank_phase.tsv")} == off
    assert len([k for k in on if k.endswith(".flank_phase.tsv")]) == 5
    tops = {n: sorted(q.name[len(n) + 1:] for q in tmp.glob(f"{n}.*")) for n in ("absent", "off", "on")}
    assert tops["absent"] == tops["off"] == ["NanoRepeat_output.tsv", "NanoRepeat_partial.tsv", "details"]
    assert tops["on"] == ["NanoRepeat_flank_phase.tsv", "NanoRepeat_output.tsv", "NanoRepeat_partial.tsv", "details"]
    for name in tops["off"][:2]:
        assert (tmp / f"absent.{name}").read_bytes() == (tmp / f"off.{name}").read_bytes() == (tmp / f"on.{name}").read_bytes()


def test_a_region_without_a_call_and_the_joint_command(panel_run):
    import inspect
    from nanorepeat_amd import flank, pipeline
    _, regions, _, _ = panel_run

    class Bare:
        chrom, start_pos, end_pos, repeat_unit_seq = "chr9", 5, 50, "CAG"
    row = flank.flank_summary_row(Bare()).rstrip("\n").split("\t")
    assert len(row) == len(SUMMARY_COLUMNS) and row[:4] == ["chr9", "5", "50", "CAG"] and set(row[4:]) == {"-"}
    assert "flank_phase" not in inspect.signature(pipeline.quantify_joint).parameters
    for fn in (pipeline.quantify_from_bam, pipeline.quantify_from_reads):
        par = inspect.signature(fn).parameters
        assert [par[k].default for k in ("flank_phase", "flank_len", "flank_skip", "flank_min_sites")] == [False, 3000, 20, 2]


def test_backbones_and_segments():
    from nanorepeat_amd import flank
    chrom = "acgtNACGTTGCA" + "CAGCAG" + "TTGACnGT"
    assert flank.flank_sides(chrom, 13, 19, 5) == ("ACGTT", "TTGAC")
    assert flank.flank_sides(chrom, 13, 19, 3000) == ("ACGTTGCA", "TTGAC")        # cut at the first base that is not ACGT
    assert flank.cut_of(3000) == 2813 and flank.cut_of(10) == 10


# ---------------------------------------------------------------------------- C ABI
def test_symbol_is_declared_and_exported(capi):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int nra_flank_phase(" in open(os.path.join(root, "include", "nanorepeat_amd.h")).read()
    assert "nra_flank_phase" in capi.EXPORTS and hasattr(capi.load(), "nra_flank_phase")
    assert capi.load().nra_abi_version() == 4
    assert capi.FLANK_DEFAULTS == R.DEFAULTS and capi.FLANK_RES == R.RES_FIELDS


BAD_THRESHOLDS = ((dict(max_dist=-1), -1), (dict(max_dist=501), -3), (dict(skip=-1), -1), (dict(min_count=0), -1),
                  (dict(min_sites=0), -1), (dict(min_share_pct=0), -1), (dict(min_share_pct=101), -3),
                  (dict(min_purity_pct=0), -1), (dict(min_purity_pct=101), -3), (dict(max_sites=0), -1),
                  (dict(max_sites=4097), -3), (dict(max_iter=0), -1), (dict(max_iter=65), -3))
BAD_INPUTS = (([[("A" * 200001, "")]], [("ACGT", "ACGT")], -3), ([[("", "A" * 200001)]], [("ACGT", "ACGT")], -3),
              ([[("ACGT", "")]], [("A" * 200001, "")], -3), ([[("ACGT", "")]], [("", "A" * 200001)], -3),
              ([[("ACGT", "")]], [("ACNT", "ACGT")], -1), ([[("ACGT", "")]], [("ACGT", "AC-T")], -1))


def check_bad_arguments(capi):
    for kw, code in BAD_THRESHOLDS:
        with pytest.raises(capi.NraError) as e:
            capi.flank_phase([[("CAGCAG", "TTGACC")]], [("CAGCAG", "TTGACC")], **kw)
        assert e.value.code == code, kw
    for groups, bbs, code in BAD_INPUTS:
        with pytest.raises(capi.NraError) as e:
            capi.flank_phase(groups, bbs)
        assert e.value.code == code
    with pytest.raises(TypeError):
        capi.flank_phase([[("ACGT", "")]], [("ACGT", "")], min_site=1)
    with pytest.raises(ValueError):
        capi.flank_phase([[("ACGT", "")]], [])


def test_flank_phase_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    check_bad_arguments(capi)
    with pytest.raises(capi.NraError) as e:
        capi.flank_phase([[("CAGCAG", "TTG"), ("CAGCAA", None)], []], [("CAGCAG", "TTGACC"), ("", "")])
    assert e.value.code == -2 and "no HIP device" in str(e.value)
