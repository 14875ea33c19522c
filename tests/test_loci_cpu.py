"""Loci from discovered runs (nanorepeat_amd/loci.py) without a GPU: the two restatements of the
sketch-pair contract against each other, every grouping rule on hand-built runs with the restatement as the engine, the
files, and the measured default min_shared."""
import inspect
import os

import numpy as np
import pytest

import scan_ref
import sketch_cases as cases
import sketch_ref as R
from nanorepeat_amd import discover as D, io as nr_io, loci as L, pipeline, synth

RNG = np.random.default_rng(30)
FLANK = {name: synth.rand_seq(RNG, 200) for name in
         ("L1", "R1", "L2", "R2", "L3", "R3", "L4", "R4", "L5", "R5", "L9", "R9", "X", "Y")}
rc = synth.revcomp


def scan_engine(seqs, k, max_gap, min_span, device=0):
    runs, stats = scan_ref.scan(list(seqs), k, max_gap, min_span)
    cols = np.array(runs, np.int32).reshape(len(runs), 6).T
    out = dict(zip(("read", "start", "end", "cls", "windows", "fwd_windows"), cols))
    out["stats"] = stats
    return out


def run(name, cls, left, right, kind="spanned", strand="+", copies=40, index=None):
    """A row as discover.scan_reads(flank_len > 0) gives it; left / right name a FLANK or are a sequence."""
    p = len(cls)
    left, right = FLANK.get(left, left), FLANK.get(right, right)
    return dict(name=name, read_len=len(left) + copies * p + len(right), ref="-", ref_start="-", start=len(left),
                end=len(left) + copies * p, span=copies * p, class_id=D.class_id(cls), cls=D.class_word(D.class_id(cls)),
                unit=cls, strand=strand, copies=copies, windows=copies * p - 10, density=1.0, kind=kind,
                left_flank=left, right_flank=right, read_index=index)


def grouped(rows, **kw):
    return L.group_runs(rows, engine=R.engine, **kw)


def members(g):
    return [[r for r in locus["runs"]] for locus in g["loci"]]


# ----------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("i", range(7))
def test_numpy_restatement_equals_plain_python(i):
    c = cases.small_cases()[i]
    a, b = R.pairs_loops(**c), R.pairs_numpy(**c)
    assert a == b
    if i < 3:
        assert a[1][:4] == [0, 0, 1, 2] and a[1][6] == a[1][9] == a[1][10] == 0 and len(a[0]) > 5


def test_restatement_by_hand():
    k = 11
    w = "ACGTTGCATGA"
    got, sizes, stats = R.pairs_loops([w, rc(w), w.lower() + "N" + w, "AAAAAAAAAAAAAAA", "ACACACACACACACA", w], [0, 0, 0, 0, 0, 1],
                                      k, 1)
    assert sizes == [1, 1, 1, 0, 0, 1] and got == [(0, 1, 1), (0, 2, 1), (1, 2, 1)]
    assert stats == dict(n_windows=1 + 1 + 2 + 5 + 5 + 1, n_kmers=4, n_compared=10)
    assert R.sketch_loops(w, k)[0] == {min(R.word_value(w), R.word_value(rc(w)))}


# ----------------------------------------------------------------------------------- the rules
def test_both_sides_link_and_one_side_does_not():
    rows = [run("a", "AAGGG", "L1", "R1"), run("b", "AAGGG", "L1", "R1"), run("c", "AAGGG", "L1", "R2"),
            run("d", "AAAAG", "L1", "R1")]                                    # another class: another group
    g = grouped(rows)
    assert members(g) == [[0, 1], [2], [3]] and [l["type"] for l in g["loci"]] == ["core"] * 3
    assert [r["role"] for r in g["runs"]] == ["core"] * 4 and [r["links"] for r in g["runs"]] == [1, 1, 0, 0]
    assert g["counts"] == dict(core=3, open=0, ambiguous=0, unplaced=0)


def test_attachment_and_an_ambiguous_open_run():
    rows = [run("a", "AAGGG", "L1", "R1"), run("b", "AAGGG", "L1", "R1"), run("c", "AAGGG", "L1", "R2"),
            run("o1", "AAGGG", "X", "R1", kind="left_open"),                   # its D side: locus 1 only
            run("o2", "AAGGG", "L1", "Y", kind="right_open"),                  # its U side: loci 1 and 2
            run("o3", "AAGGG", "R2", "Y", kind="right_open")]                  # its U side is locus 2's D side: no match
    g = grouped(rows)
    assert [(r["locus"], r["role"], r["links"]) for r in g["runs"]] == [
        (1, "core", 1), (1, "core", 1), (2, "core", 0), (1, "attached", 2), (None, "ambiguous", 0), (3, "open", 0)]
    assert g["counts"] == dict(core=2, open=1, ambiguous=1, unplaced=0)
    table = L.locus_rows(rows, g)
    first = next(c for c in table if c["Locus"] == 1)
    assert (first["Runs"], first["Spanned"], first["Left_Open"], first["Max_Open_Copies"]) == (3, 2, 1, 40)


def test_open_loci_of_each_kind():
    rows = [run("u1", "AAGGG", "L9", "X", kind="right_open"), run("d1", "AAGGG", "X", "R9", kind="left_open", copies=70),
            run("u2", "AAGGG", "L9", "Y", kind="right_open"), run("d2", "AAGGG", "Y", "R9", kind="left_open"),
            run("m", "AAGGG", rc(FLANK["R9"]), "X", kind="right_open", strand="-"),   # a - run's left flank is its D side
            run("n", "AAGGG", "R9", "X", kind="right_open")]                  # R9 as a U side: comparable with no D side
    g = grouped(rows)
    assert members(g) == [[0, 2], [1, 3, 4], [5]]
    assert [l["type"] for l in g["loci"]] == ["open_U", "open_D", "open_U"]
    table = L.locus_rows(rows, g)
    assert [c["Max_Copies"] for c in table] == ["-"] * 3 and [c["Locus"] for c in table] == [1, 2, 3]
    assert table[1]["Max_Open_Copies"] == 70 and table[1]["Left_Open"] == 2 and table[1]["Right_Open"] == 1


def test_minus_strand_sides_swap():
    fwd = run("f", "AAGGG", "L1", "R1")
    rev = run("r", "AAGGG", rc(FLANK["R1"]), rc(FLANK["L1"]), strand="-")     # the same locus read from the other strand
    assert L.run_sides(rev, 13) == {"D": rev["left_flank"], "U": rev["right_flank"]}
    assert members(grouped([fwd, rev])) == [[0, 1]]
    wrong = dict(rev, strand="+")                                              # without the swap U meets D: no link
    assert members(grouped([fwd, wrong])) == [[0], [1]]


def test_self_complementary_class_links_under_either_pairing():
    assert L.self_complementary("AT") and L.self_complementary("ACGT") and not L.self_complementary("AAGGG")
    fwd = run("f", "AT", "L5", "R5")
    rev = run("r", "AT", rc(FLANK["R5"]), rc(FLANK["L5"]))                    # reverse-complemented read, strand still +
    half = run("h", "AT", rc(FLANK["R5"]), "Y")                               # one side only, under either pairing
    o = run("o", "AT", "X", rc(FLANK["L5"]), kind="left_open")                # any side is comparable with any
    g = grouped([fwd, rev, half, o])
    assert members(g) == [[0, 1, 3], [2]] and g["runs"][3]["role"] == "attached"


def test_unplaced_runs():
    rows = [run("in", "AAGGG", "L1", "R1", kind="in_repeat"), run("short", "AAGGG", "L1", "ACGTACGTACGT"),
            run("open", "AAGGG", "ACGT", "ACGTACGTACGT", kind="left_open"), run("a", "AAGGG", "L1", "R1")]
    g = grouped(rows)
    assert [r["role"] for r in g["runs"]] == ["unplaced"] * 3 + ["core"] and [r["locus"] for r in g["runs"]] == [None] * 3 + [1]
    assert L.run_sides(rows[0], 13) == {} and list(L.run_sides(rows[1], 13)) == ["U"]
    assert grouped([])["counts"] == dict(core=0, open=0, ambiguous=0, unplaced=0)


def test_representative_and_locus_order():
    noisy = lambda name, seed: synth.apply_errors(np.random.default_rng(seed), FLANK[name], "ont")
    rows = [run("late", "AAAAG", "L4", "R4", copies=90),
            run("n1", "AAGGG", noisy("L1", 1), noisy("R1", 2), copies=50), run("clean", "AAGGG", "L1", "R1", copies=60),
            run("n2", "AAGGG", noisy("L1", 3), noisy("R1", 4), copies=55), run("late2", "AAAAG", "L4", "R4", copies=91)]
    g = grouped(rows)
    assert members(g) == [[0, 4], [1, 2, 3]]
    assert [l["rep"] for l in g["loci"]] == [0, 2]                             # a tie goes to the earliest; else the most shared
    table = L.locus_rows(rows, g, {D.class_id("AAGGG"): 2})
    assert [c["Locus"] for c in table] == [1, 2] and table[1]["Rep_Read"] == "clean"
    assert (table[1]["Min_Copies"], table[1]["Median_Copies"], table[1]["Max_Copies"]) == (50, "55", 60)
    assert table[0]["Catalogued_Regions"] == 0 and table[1]["Catalogued_Regions"] == 2


def test_bad_values():
    for bad in (dict(sketch_k=12), dict(sketch_k=17), dict(flank_len=5), dict(flank_len=3000), dict(min_shared=0),
                dict(min_locus_reads=0)):
        with pytest.raises(ValueError):
            pipeline.discover_repeats("nowhere.fastq", "nowhere", group_loci=True, **bad)
    with pytest.raises(ValueError):
        pipeline.quantify_from_reads("r.fq", "ref.fa", "x.bed", "out", group_loci=True)
    sig = inspect.signature(pipeline.discover_repeats).parameters
    assert sig["group_loci"].default is False and sig["flank_len"].default == 500 and sig["sketch_k"].default == 13
    assert sig["min_locus_reads"].default == 3 and L.check_options(500, 13, None, 3) == L.MIN_SHARED
    assert inspect.signature(pipeline.quantify_from_reads).parameters["group_loci"].default is False


# ----------------------------------------------------------------------------------- the files
def _panel(tmp_path):
    """Two AAGGG loci (A: 4 spanning reads of 60 and 2 of 120 copies, one of them reverse-complemented, and a
    left-open read; B: 3 spanning reads), one AAAAG locus of 2 reads and a read inside an AAGGG run."""
    rng = np.random.default_rng(31)
    flank = lambda: "T" + synth.rand_seq(rng, 1198) + "C"
    la, ra, lb, rb, lc, rcc = (flank() for _ in range(6))
    pure = lambda unit, n: unit * n
    reads = [("b1", lb + pure("AAGGG", 200) + rb), ("a60_1", la + pure("AAGGG", 60) + ra),
             ("c1", lc[500:] + pure("AAAAG", 80) + rcc), ("a120_1", la[300:] + pure("AAGGG", 120) + ra),
             ("a60_2", rc(la + pure("AAGGG", 60) + ra)), ("b2", lb + pure("AAGGG", 200) + rb[:800]),
             ("inside", pure("AAGGG", 300)), ("a_open", pure("AAGGG", 150) + ra), ("a60_3", la + pure("AAGGG", 60) + ra),
             ("b3", lb[100:] + pure("AAGGG", 201) + rb), ("a120_2", la + pure("AAGGG", 120) + ra),
             ("c2", lc + pure("AAAAG", 80) + rcc), ("a60_4", la[:] + pure("AAGGG", 60) + ra[:1100])]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join(f"@{n}\n{s}\n+\n{'5' * len(s)}\n" for n, s in reads))
    return str(fq), dict(reads)


def test_files_formats_and_the_feedback_inputs(tmp_path, capsys):
    fq, reads = _panel(tmp_path)
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    pipeline.discover_repeats(fq, off, engine=scan_engine)
    capsys.readouterr()
    pipeline.discover_repeats(fq, on, engine=scan_engine, group_loci=True, sketch_engine=R.engine)
    err = capsys.readouterr().err
    assert "NOTICE: the discovered runs form 3 core locus/loci (2 with at least 3 spanned runs) and 0 open" in err
    assert "0 ambiguous and 1 unplaced run(s)" in err

    # the two files of the command without the switch are byte for byte what they were
    names = {f[3:] for f in os.listdir(tmp_path) if f.startswith("on.")}
    assert names == {"discovered_runs.tsv", "NanoRepeat_discovered.tsv", "discovered_loci.tsv",
                     "discovered_locus_runs.tsv", "discovered_loci.fa", "discovered_loci.bed"}
    assert {f[4:] for f in os.listdir(tmp_path) if f.startswith("off.")} == {"discovered_runs.tsv",
                                                                             "NanoRepeat_discovered.tsv"}
    for name in ("discovered_runs.tsv", "NanoRepeat_discovered.tsv"):
        assert open(f"{on}.{name}", "rb").read() == open(f"{off}.{name}", "rb").read()

    lines = [l.split("\t") for l in open(on + ".discovered_loci.tsv").read().splitlines()]
    assert tuple(lines[0]) == L.LOCUS_COLUMNS
    loci = [dict(zip(lines[0], l)) for l in lines[1:]]
    assert [(c["Locus"], c["Class"], c["Type"], c["Max_Copies"]) for c in loci] == [
        ("1", "AAGGG", "core", "201"), ("2", "AAGGG", "core", "120"), ("3", "AAAAG", "core", "80")]
    a = loci[1]
    assert (a["Runs"], a["Reads"], a["Spanned"], a["Left_Open"], a["Right_Open"]) == ("7", "7", "6", "1", "0")
    assert (a["Min_Copies"], a["Median_Copies"], a["Max_Copies"], a["Max_Open_Copies"]) == ("60", "60", "120", "150")
    assert a["Rep_Read"] == "a60_1" and a["Ref"] == a["Ref_Start"] == a["Catalogued_Regions"] == "-"
    assert loci[0]["Rep_Read"] == "b1" and loci[0]["Unit"] in ("AAGGG", "AGGGA", "GGGAA", "GGAAG", "GAAGG")

    runs = [l.split("\t") for l in open(on + ".discovered_locus_runs.tsv").read().splitlines()]
    assert tuple(runs[0]) == L.LOCUS_RUN_COLUMNS
    by_read = {r[0]: r for r in runs[1:]}
    assert [r[0] for r in runs[1:]] == [n for n in reads]                     # file order
    assert by_read["inside"][4:] == ["-", "unplaced", "0"] and by_read["a_open"][4:] == ["2", "attached", "6"]
    assert by_read["a60_2"][4:] == ["2", "core", "5"] and by_read["c2"][4:] == ["3", "core", "1"]

    # the pseudo-reference and its BED file load through io and are what the rule says
    ref = nr_io.fasta_file2dict(on + ".discovered_loci.fa")
    regions = nr_io.read_repeat_region_file(on + ".discovered_loci.bed", True)
    assert list(ref) == ["locus_1", "locus_2"] == [r.chrom for r in regions]
    b1 = reads["b1"]
    assert ref["locus_1"] == b1[200:1200 + 1000 + 1000] and (regions[0].start_pos, regions[0].end_pos) == (1000, 2000)
    assert ref["locus_2"] == reads["a60_1"][200:1200 + 300 + 1000] and regions[1].repeat_unit_seq == a["Unit"]
    for region in regions:
        nr_io.extract_ref_sequence(ref, region, 1000)
        assert nr_io.check_repeat_motif_in_ref(region) and region.left_anchor_len == region.right_anchor_len == 1000

    # a representative that starts less than 1000 bases into its read: the left anchor actually cut
    short = str(tmp_path / "short")
    pipeline.discover_repeats(fq, short, engine=scan_engine, group_loci=True, sketch_engine=R.engine, min_locus_reads=2,
                              no_details=True)
    bed = [l.split("\t") for l in open(short + ".discovered_loci.bed").read().splitlines()]
    assert bed[2][:3] == ["locus_3", "700", "1100"] and not os.path.exists(short + ".discovered_locus_runs.tsv")
    assert nr_io.fasta_file2dict(short + ".discovered_loci.fa")["locus_3"] == reads["c1"][:700 + 400 + 1000]


def test_group_limit_notice(tmp_path, capsys):
    fq, _ = _panel(tmp_path)
    rows = D.scan_reads(fq, engine=scan_engine, flank_len=500)
    table, g = L.loci_files(fq, str(tmp_path / "lim"), rows, engine=R.engine, max_group=10)
    err = capsys.readouterr().err
    assert "NOTICE: class(es) AAGGG have more than 10 sides and are left ungrouped" in err
    assert [c["Class"] for c in table] == ["AAAAG"] and g["ungrouped"] == ["AAGGG"]
    runs = [l.split("\t") for l in open(tmp_path / "lim.discovered_locus_runs.tsv").read().splitlines()[1:]]
    assert all(r[4:] == ["-", "unplaced", "0"] for r in runs if r[3] == "AAGGG") and len(runs) == 13


def test_rows_without_flanks_are_what_they_were(tmp_path):
    fq, _ = _panel(tmp_path)
    plain = D.scan_reads(fq, engine=scan_engine)
    with_flanks = D.scan_reads(fq, engine=scan_engine, flank_len=500, chunk_bases=3000)     # several chunks
    extra = ("left_flank", "right_flank", "read_index")
    assert not any(key in row for row in plain for key in extra)
    assert [{k: v for k, v in row.items() if k not in extra} for row in with_flanks] == plain
    assert [row["read_index"] for row in with_flanks] == list(range(13))
    assert all(len(row["left_flank"]) <= 500 and len(row["right_flank"]) <= 500 for row in with_flanks)
    assert D.fetch_reads(fq, {0, 12}, 3000) == {0: ("b1", _panel(tmp_path)[1]["b1"]), 12: ("a60_4", _panel(tmp_path)[1]["a60_4"])}


# ----------------------------------------------------------------------------------- the default
def _pair_counts(pairs, k):
    seqs = [s for p in pairs for s in p]
    got, _, _ = R.pairs(seqs, [i // 2 for i in range(len(seqs))], k, 1)
    out = np.zeros(len(pairs), int)
    for a, _, n in got:
        out[a // 2] = n
    return out


def _flank_pairs(rng, model, n, flank, kind):
    out = []
    for _ in range(n):
        if kind == "true":
            x = y = synth.rand_seq(rng, flank)
        elif kind == "decoy":
            x, y = synth.rand_seq(rng, flank), synth.rand_seq(rng, flank)
        else:                                       # two unrelated flanks around one 300-base interspersed element
            element = synth.rand_seq(rng, 300)
            x, y = (synth.rand_seq(rng, (flank - 300) // 2) + element + synth.rand_seq(rng, (flank - 300) // 2)
                    for _ in range(2))
        a, b = synth.apply_errors(rng, x, model), synth.apply_errors(rng, y, model)
        out.append((a, synth.revcomp(b) if rng.random() < 0.5 else b))
    return out


def test_default_table(capsys):
    """400 pairs per line, seeded.  At the defaults (k = 13, flank_len = 500) the largest count of
    an unrelated pair is below min_shared and the smallest count of a true pair is at or above it, for both models.  The
    pairs that share a 300-base element do match: rule 1's both-sides requirement is for them, and their counts are
    recorded, not asserted."""
    sig = inspect.signature(pipeline.discover_repeats).parameters
    k, flank, n = sig["sketch_k"].default, sig["flank_len"].default, 400
    assert sig["min_shared"].default is None and (k, flank) == (13, 500)
    lines = []
    for model in ("ont", "hifi"):
        rng = np.random.default_rng(1000 + len(model))
        true = _pair_counts(_flank_pairs(rng, model, n, flank, "true"), k)
        short = _pair_counts(_flank_pairs(rng, model, n, 300, "true"), k)
        decoy = _pair_counts(_flank_pairs(rng, model, n, flank, "decoy"), k)
        element = _pair_counts(_flank_pairs(rng, model, n, flank, "element"), k)
        lines.append(f"{model}: true 500 min {true.min()} median {int(np.median(true))}; true 300 min {short.min()} "
                     f"({int((short < L.MIN_SHARED).sum())} of {n} below min_shared); decoy max {decoy.max()}; "
                     f"element-sharing min {element.min()} median {int(np.median(element))} max {element.max()}")
        with capsys.disabled():
            print("\n" + lines[-1])
        assert decoy.max() < L.MIN_SHARED <= true.min()
