"""Tandem periods without a GPU: the numpy restatement against the double loop and against the kernel's word algorithm
restated lane by lane, the rules on hand-made spectra, the unit of a consensus, the comparison with BED motifs of any
length, the file text, and the FASTQ command with discover_periods=True (restatements as engines, oracle as scorer) on
synth.period_panel.  The argument checks of nra_tract_periods are in test_periods_capi.py."""
import os

import numpy as np
import pytest

from nanorepeat_amd import motifs, periods, synth
import period_cases as cases
from period_ref import ref_tract_periods, words_tract_periods


def test_numpy_restatement_equals_the_double_loop():
    tracts = [t for t in cases.edge_tracts() if len(t) <= 129] + cases.p_and_p_plus_one() + \
        cases.non_acgt_tracts() + cases.lower_case_tracts() + cases.short_mixed(count=40)
    for max_period in cases.MAX_PERIODS:
        a = ref_tract_periods(tracts, max_period)
        b = ref_tract_periods(tracts, max_period, vectorised=False)
        for k in a:
            assert a[k].dtype == np.int32 and np.array_equal(a[k], b[k]), (k, max_period)


def test_word_algorithm_of_the_kernel_equals_the_restatement():
    """Packing, the two pairs, the shift by the whole word at lags 32 and 64, the tail masks and the 62-word step (from
    1985 bases on), at every edge length."""
    tracts = cases.edge_tracts() + cases.p_and_p_plus_one() + cases.non_acgt_tracts() + cases.lower_case_tracts() + \
        [synth.rand_seq(np.random.default_rng(38), n) for n in (1984, 1985, 4000)]
    want = ref_tract_periods(tracts)
    for t, s in enumerate(tracts):
        match, valid = words_tract_periods(s)
        assert match == want["match"][t].tolist() and valid == want["valid"][t].tolist(), (t, len(s))


def test_hand_spectra():
    out = ref_tract_periods(["CAG" * 10, "", "A", "acgtN", "CAGCAN"], 6)
    assert out["valid"][0].tolist() == [29, 28, 27, 26, 25, 24] and out["match"][0].tolist() == [0, 0, 27, 0, 0, 24]
    assert not out["valid"][1:3].any() and not out["match"][1:3].any()
    assert out["valid"][3].tolist() == [3, 2, 1, 0, 0, 0] and not out["match"][3].any()
    assert out["valid"][4].tolist() == [4, 3, 2, 1, 0, 0] and out["match"][4].tolist() == [0, 0, 2, 0, 0, 0]
    with pytest.raises(ValueError):
        ref_tract_periods(["A"], 65)


def _spectrum(shares, valid=100):
    v = np.full(len(shares), valid, np.int64)
    return np.round(np.array(shares) * valid).astype(np.int64), v


def test_call_period_rules():
    flat = [0.25] * 64
    # multiples: 5 before 10 and 15; 12 before 24
    s = list(flat)
    for p in (5, 10, 15, 20):
        s[p - 1] = 1.0
    assert periods.call_period(*_spectrum(s)) == (5, 1.0)
    s = list(flat)
    s[11], s[23], s[4] = 0.97, 1.0, 0.6                          # a divisor-like lag of the 12-mer stays out
    assert periods.call_period(*_spectrum(s)) == (12, 0.97)
    # within tol of the largest: the smaller p; beyond tol: not
    s = list(flat)
    s[29], s[59] = 0.90, 0.95
    assert periods.call_period(*_spectrum(s), tol=0.05)[0] == 30
    assert periods.call_period(*_spectrum(s), tol=0.04)[0] == 60
    # ties
    s = list(flat)
    s[6] = s[13] = s[20] = 0.8
    assert periods.call_period(*_spectrum(s))[0] == 7
    # flat spectra: no call, the largest share comes back
    assert periods.call_period(*_spectrum(flat)) == (None, 0.25)
    s = list(flat)
    s[8] = 0.49
    assert periods.call_period(*_spectrum(s)) == (None, 0.49)
    assert periods.call_period(*_spectrum(s), min_share=0.49)[0] == 9
    # min_valid, and valid >= p
    m, v = _spectrum([1.0, 0.25, 0.25, 1.0])
    v[0], m[0] = 11, 11
    assert periods.call_period(m, v, min_valid=12)[0] == 4 and periods.call_period(m, v, min_valid=11)[0] == 1
    m, v = np.array([0, 0, 20, 0] + [0] * 36 + [30]), np.array([50, 50, 50, 50] + [50] * 36 + [40])
    assert periods.call_period(m, v) == (None, 0.4)              # lag 41 has 40 < 41 positions: out
    v[40] = 41
    assert periods.call_period(m, v)[0] == 41
    assert periods.call_period(np.zeros(64, int), np.zeros(64, int)) == (None, None)
    # support: the window p - 1, p, p + 1; the top lags by share, then lag
    s = list(flat)
    s[28], s[29], s[30], s[59] = 0.3, 0.4, 0.7, 0.7
    assert periods.support_of(*_spectrum(s), 30) == 0.7 and periods.support_of(*_spectrum(s), 28) == 0.3
    assert periods.support_of(*_spectrum(s), 1) == 0.25 and periods.support_of(*_spectrum(s), 64) == 0.25
    assert periods.top_lags(*_spectrum(s)) == [(31, 0.7), (60, 0.7), (30, 0.4)]
    assert periods.top_lags(np.zeros(4, int), np.zeros(4, int)) == []


def test_rules_on_the_restatement_of_pure_tracts():
    rng = np.random.default_rng(3)
    for p in (1, 2, 3, 5, 12, 25, 30, 60, 64):
        u = synth.primitive_unit(rng, p)
        for copies in (3, 6, 20):
            out = ref_tract_periods([u * copies + u[:p // 2]])
            got = periods.call_period(out["match"][0], out["valid"][0])
            if p * (copies - 1) + p // 2 >= periods.MIN_VALID:   # valid[p] of a tract of p * copies + p // 2 bases
                assert got == (p, 1.0), (p, copies)
            else:
                assert got[0] is None, (p, copies)
    out = ref_tract_periods([synth.rand_seq(rng, n) for n in (100, 200, 300) for _ in range(20)])
    assert all(periods.call_period(m, v)[0] is None for m, v in zip(out["match"], out["valid"]))


def test_unit_of_a_consensus():
    assert periods.unit_of("GCAGCAGCA", 3) == "GCA"
    assert periods.unit_of("TTCAGCAGCAG", 3) == "AGC"            # first copy at 2: rotated back by 2
    assert periods.unit_of("TCAGCAGCAG", 3) == "GCA"
    assert periods.unit_of("ttcagcagcag", 3) == "AGC"
    cstb = "CCCCGCCCCGCG"
    assert periods.unit_of("GCG" + cstb * 3, 12) == "GCG" + cstb[:9]
    assert periods.unit_of(cstb + cstb[:6] + "A" + cstb[6:] + cstb * 2, 12) == cstb[11:] + cstb[:11]   # first copy at 19: the inserted base moves the phase by one
    assert periods.unit_of("ATATATAT", 4) is None                # ATAT is not primitive
    assert periods.unit_of("AAAAAAAA", 2) is None and periods.unit_of("AAAA", 1) == "A"
    assert periods.unit_of("CAGCATCAGCAT", 3) is None            # no exact copy
    assert periods.unit_of("CANCANCAN", 3) is None               # not ACGT
    assert periods.unit_of("CAGCA", 3) is None and periods.unit_of("", 5) is None


def test_bed_roots_longer_than_six():
    cstb = "CCCCGCCCCGCG"
    assert motifs.bed_class(cstb) is None                        # what discover_motifs does with such a root
    assert periods.root_class(cstb) == motifs.motif_class(cstb) == "CCCCGCCCCGCG"
    assert periods.root_class(cstb * 2) == periods.root_class(cstb[5:] + cstb[:5]) == periods.root_class(cstb.lower())
    assert periods.root_class("CAGCAG") == "AGC" and periods.root_class("CAN") is None and periods.root_class("") is None
    rng = np.random.default_rng(4)
    u, v = synth.primitive_unit(rng, 30), synth.primitive_unit(rng, 30)
    assert periods.root_class(u[7:] + u[:7]) == periods.root_class(u) != periods.root_class(v)


# ---------------------------------------------------------------------------- file text
def _small_region():
    class Read:
        def __init__(self, size):
            self.round3_repeat_size, self.left_buffer_len, self.right_buffer_len = size, 2, 2

    class Q:
        def __init__(self, allele_id):
            self.allele_id = allele_id

    class Results:
        quantified_allele_list = [object(), object()]
        quantified_read_dict = {"a": Q(1), "b": Q(1), "c": Q(2), "d": Q(-1)}

    class Consensus:
        def __init__(self, sequence):
            self.sequence = sequence

    class Region:
        chrom, start_pos, end_pos, repeat_unit_seq = "chr2", 10, 40, "CAG"
        no_details, out_prefix = False, None
        left_anchor_seq, right_anchor_seq = "ACGTACGT", "TTGACCAT"
        results = Results()
        read_dict = {"a": Read(8.0), "b": Read(8.5), "c": Read(None), "d": Read(3.0), "e": Read(2.0)}
        read_core_seq_dict = {"a": "TT" + "CCTG" * 8 + "TT", "b": "TT" + "CCTG" * 4 + "A" + "CCTG" * 4 + "TT",
                              "c": "TTACGGTCATGCAATGCTAGGCTATT", "d": "TT" + "CAG" * 6 + "TT"}
        allele_consensus = [Consensus("CCTG" * 8), Consensus("ACGGTCATGCAATGCTAGGCTA")]

        @staticmethod
        def to_unique_id():
            return "chr2-10-40-CAG"

    return Region


def test_file_text_of_a_small_region():
    region = _small_region()
    sized = []

    def scorer(units, reads, kmin, kmax, read_region, sc, device, per_candidate):
        sized.append((units, list(reads), kmin.tolist(), kmax.tolist(), read_region.tolist()))
        n = len(reads)
        return dict(status=np.array([0, 1][:n]), sum_k=np.array([17, 0][:n]), n_ties=np.array([2, 1][:n]))

    periods.period_regions([region], engine=ref_tract_periods, scorer=scorer)
    assert sized == [([("ACGTACGT", "CCTG", "TTGACCAT")], [region.read_core_seq_dict["a"], region.read_core_seq_dict["b"]],
                      [0, 0], [23, 23], [0, 0])]
    assert periods.read_periods_text(region) == (
        "##RepeatRegion=chr2-10-40-CAG\n##Motif=CAG\n##Allele=1 period=4 unit=CCTG\n##Allele=2 period=- unit=-\n"
        "#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tPeriod\tShare\tSupport\tSize_In_Unit\tTop_Lags\n"
        "a\t1\t8.0\t32\t4\t1.00\t1.00\t8.5\t4:1.00,8:1.00,12:1.00\n"
        "b\t1\t8.5\t33\t4\t0.86\t0.86\t-\t4:0.86,8:0.72,13:0.70\n"          # 25 of 29 at lag 4; not READ_OK
        "c\t2\t-\t22\t-\t0.59\t-\t-\t5:0.59,10:0.50,8:0.29\n"            # 10 of 17 at lag 5: below min_share
        "d\t.\t3.0\t18\t3\t1.00\t-\t-\t3:1.00,6:1.00,1:0.00\n")
    assert periods.period_summary_row(region) == (
        "chr2\t10\t40\tCAG\t4\t1:4:CCTG:1.00:2/2:0.93:8.5|2:-:-:0.59:0/0:-:-\n")
    assert periods.report_foreign_units([region], stream=open(os.devnull, "w")) == (1, 2)

    class Empty:
        chrom, start_pos, end_pos, repeat_unit_seq = "chr2", -5, 40, "CAGN"

    assert periods.period_summary_row(Empty) == "chr2\t0\t40\tCAGN\t0\t-\n"


# ---------------------------------------------------------------------------- the command
def _truth_allele(p, ap):
    votes = [p["truth"][n][1] for n in ap.read_names]
    return max(set(votes), key=votes.count)


def check_panel(p, regions, summary):
    """What section 22 promises on synth.period_panel, on the regions and on the summary text (also the GPU suite's)."""
    rows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    assert summary.startswith("#Chrom\tStart\tEnd\tMotif\tNum_Reads\tAllele_Periods\n") and len(rows) == len(regions) == 7
    for g, (region, row) in enumerate(zip(regions, rows)):
        cells = [c.split(":") for c in row[5].split("|")]
        aps = region.allele_periods
        assert len(cells) == len(aps) >= 1 and all(len(c) == 7 for c in cells), row
        bed = periods.root_class(region.repeat_unit_seq)
        for ap, cell in zip(aps, cells):
            assert cell[0] == str(ap.allele_id) and cell[1] == ("-" if ap.period is None else str(ap.period))
            assert cell[2] == (ap.unit or "-")
            unit, copies = p["planted"][g][_truth_allele(p, ap)]
            rps = [region.read_periods[n] for n in ap.read_names if n in region.read_periods]
            sizes = [rp.size_in_unit for rp in rps if rp.size_in_unit is not None]
            if unit is None:                                     # the region without a period
                assert ap.period is None and ap.unit is None and cell[1:3] == ["-", "-"] and cell[6] == "-", row
                continue
            assert ap.period == len(unit) and motifs.motif_class(ap.unit) == motifs.motif_class(unit), (g, cell)
            assert sizes and abs(float(np.median(sizes)) - copies) <= 1, (g, cell)
            assert cell[6] == f"{float(np.median(sizes)):.1f}"
            foreign = motifs.motif_class(unit) != bed
            assert ap.differs == foreign and foreign == (g == 3 and copies == 15)
            if not foreign:                                      # the round-3 size, the controls among them
                assert all(region.read_periods[n].size_in_unit == region.read_dict[n].round3_repeat_size
                           for n in ap.read_names if n in region.read_periods)
        if g < 6:
            assert {_truth_allele(p, ap) for ap in aps} == {0, 1}, row
    assert [len(u) for u, _ in p["planted"][4] + p["planted"][5]] == [5, 5, 3, 3]


@pytest.fixture(scope="module")
def panel_runs(oracle, tmp_path_factory):
    """The FASTQ command on the panel with and without discover_periods, once for the tests below."""
    import consensus_ref
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    from structure_ref import ref_read_structure
    tmp = tmp_path_factory.mktemp("periods")
    p = synth.period_panel(reads_per_allele=4, anchor_len=400, model="hifi", seed=12)
    ref, bed, reads = synth.write_panel(p, str(tmp))
    common = dict(data_type="hifi", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen, no_check_repeat_motif_in_ref=True)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp / "on"), discover_periods=True,
                                           period_engine=ref_tract_periods,
                                           consensus_engine=consensus_ref.ref_tract_consensus,
                                           structure_engine=ref_read_structure, **common)
    return tmp, p, regions


def test_switch_off_is_byte_for_byte_and_writes_no_new_file(panel_runs):
    from test_screen_cpu import _tree
    tmp, p, regions = panel_runs
    assert (tmp / "on.NanoRepeat_output.tsv").read_bytes() == (tmp / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp / "on.details"), _tree(tmp / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_periods.tsv")} == off
    assert sum(k.endswith(".read_periods.tsv") for k in on) == 7
    assert sorted(f for f in os.listdir(tmp) if f.startswith("off.")) == ["off.NanoRepeat_output.tsv", "off.details"]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("on.")) == [
        "on.NanoRepeat_output.tsv", "on.NanoRepeat_periods.tsv", "on.details"]


def test_fastq_command_finds_planted_periods(panel_runs):
    tmp, p, regions = panel_runs
    check_panel(p, regions, (tmp / "on.NanoRepeat_periods.tsv").read_text())
    for region in regions:
        lines = open(region.out_prefix + ".read_periods.tsv").read().split("\n")
        assert lines[0] == f"##RepeatRegion={region.to_unique_id()}" and lines[1] == f"##Motif={region.repeat_unit_seq}"
        head = 2 + len(region.allele_periods)
        assert [l.split(" ")[0] for l in lines[2:head]] == [f"##Allele={ap.allele_id}" for ap in region.allele_periods]
        assert lines[head] == "#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tPeriod\tShare\tSupport\tSize_In_Unit\tTop_Lags"
        rows = [l.split("\t") for l in lines[head + 1:] if l]
        assert all(len(r) == 9 for r in rows)
        assert sorted(r[0] for r in rows) == sorted(n for n in region.read_dict if n in region.read_core_seq_dict)
        phased = [l.split("\t") for l in open(region.out_prefix + ".phased_reads.txt").read().split("\n")[2:] if l]
        assert [(r[0], r[1]) for r in rows[:len(phased)]] == [(r[0], r[1]) for r in phased]
        assert all(r[1] == "." for r in rows[len(phased):])
    # the reads of the foreign allele have no size to speak of in the BED motif and 15 units in their own
    foreign = [ap for ap in regions[3].allele_periods if ap.differs]
    assert len(foreign) == 1
    for n in foreign[0].read_names:
        assert abs(regions[3].read_periods[n].size_in_unit - 15) <= 1 and regions[3].read_dict[n].round3_repeat_size < 5


def test_no_details_writes_only_the_summary(oracle, tmp_path):
    import consensus_ref
    from nanorepeat_amd import pipeline
    from screen_ref import RefScreen
    from structure_ref import ref_read_structure
    p = synth.period_panel(reads_per_allele=2, anchor_len=300, model="hifi", seed=12)
    p["bed"], keep = p["bed"][4:6], {n for n, (g, _) in p["truth"].items() if g in (4, 5)}
    p["reads"] = [(n, s) for n, s in p["reads"] if n in keep]
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "o"), data_type="hifi", anchor_len=300, seed=1,
                                 no_details=True, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                                 screener=RefScreen, discover_periods=True, period_engine=ref_tract_periods,
                                 consensus_engine=consensus_ref.ref_tract_consensus,
                                 structure_engine=ref_read_structure)
    assert not (tmp_path / "o.details").exists()
    assert len((tmp_path / "o.NanoRepeat_periods.tsv").read_text().split("\n")) == 4
