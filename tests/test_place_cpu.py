"""Placement of discovered loci (nanorepeat_amd/place.py) without a GPU: the two restatements of the
nra_place_* contract against each other, every rule of place.py on a planted reference with the restatement as the engine
and the oracle as the aligner, the files, and the measured defaults."""
import inspect
import os

import numpy as np
import pytest

import place_cases as cases
import place_ref as R
import sketch_ref
from nanorepeat_amd import io as nr_io, pipeline, place as P, synth
from test_loci_cpu import scan_engine


# ----------------------------------------------------------------------------------- the contract
@pytest.mark.parametrize("n", range(len(cases.small_cases())))
def test_restatements_agree(n):
    c = cases.small_cases()[n]
    loops, arrays = R.candidates_loops(**c), R.candidates_numpy(**c)
    assert loops == arrays
    assert set(loops[1]) == set(R.COUNTERS)


def test_restatement_on_hand_counted_hits():
    """One query of k + 2 bases (three windows) on both strands of a contig, worked out by hand."""
    q = "ACGGTCATTGCAAGT"                                   # 15 bases, k = 13: windows at 0, 1, 2
    contig = "T" * 40 + q + "G" * 37 + synth.revcomp(q) + "TT"
    got, st = R.candidates_loops([q], [(7, 100, contig)], 13, 16, 16, 64, 1)
    # + strand: d = 140, bin 8; - strand: d = i + j + k - len(q) = 100 + 92 = 192 for every window, bin 12
    assert got == [(0, 7, 0, 7, 3), (0, 7, 0, 8, 3), (0, 7, 1, 11, 3), (0, 7, 1, 12, 3)]
    assert st["n_keys"] == st["n_postings"] == 3 and st["n_hits_kept"] == 6 and st["n_keys_over"] == 0
    assert st["n_target_windows"] == len(contig) - 12 and st["target_bases"] == len(contig)
    assert R.candidates_loops([q], [(7, 100, contig)], 13, 16, 16, 1, 1)[0] == []      # occ = 2 > max_target_occ = 1
    assert R.candidates_loops([q, q], [(7, 100, contig)], 13, 1, 16, 64, 1)[1]["n_masked_max_occ"] == 3


# ----------------------------------------------------------------------------------- streaming
def test_reference_chunks_give_every_window_once(tmp_path):
    p = cases.planted_panel()
    _, fa = cases.write_panel(p, tmp_path)
    for chunk in (13, 500, 1000, 70 * 7, 1 << 24):
        seen = {}
        for t, name, pos0, bases in P.iter_reference(fa, chunk, 13):
            assert name == list(p["ref"])[t] and bases == p["ref"][name][pos0:pos0 + len(bases)] and len(bases) <= chunk
            for i in range(pos0, pos0 + len(bases) - 12):
                seen[(name, i)] = seen.get((name, i), 0) + 1
        assert set(seen.values()) == {1} and len(seen) == sum(len(s) - 12 for s in p["ref"].values())
    (tmp_path / "odd.fa").write_text(">empty\n>short x\nACGT\n\n>last\nACGTACGTACGTACGTA\n")
    assert list(P.iter_reference(str(tmp_path / "odd.fa"), 16, 13)) == [
        (0, "empty", 0, ""), (1, "short", 0, "ACGT"), (2, "last", 0, "ACGTACGTACGTACGT"), (2, "last", 4, "ACGTACGTACGTA")]
    with pytest.raises(ValueError):
        list(P.iter_reference(fa, 12, 13))
    windows = P.fetch_windows(fa, {("chrB", 65, 145), ("chrB", 0, 3), ("chrC", 47800, 47850), ("chrA", 139, 141)})
    assert windows == {w: p["ref"][w[0]][w[1]:w[2]] for w in windows}

    sides = [p["ref"]["chrB"][3000:4000], synth.revcomp(p["ref"]["chrA"][100:900])]
    whole = P.scan_reference(fa, sides, 13, 16, 64, 64, 24, engine=R.Engine())
    parts = P.scan_reference(fa, sides, 13, 16, 64, 64, 24, engine=R.Engine(), chunk_bases=777)
    assert all(whole[0][key].tolist() == parts[0][key].tolist() for key in R.KEYS) and len(whole[0]["query"]) == 4
    assert whole[1] == ["chrA", "chrB", "chrC"] and whole[2] == parts[2] == {n: len(s) for n, s in p["ref"].items()}
    assert whole[3]["n_target_windows"] == parts[3]["n_target_windows"] and parts[3]["n_chunks"] > 150


# ----------------------------------------------------------------------------------- the rules
def test_side_rule():
    cands = dict(query=[0, 0, 0, 0, 1, 1, 1, 3], contig=[0, 0, 0, 2, 0, 0, 1, 5], strand=[0, 0, 1, 0, 0, 0, 0, 1],
                 bin=[4, 5, 5, 9, 7, 9, 7, -3], votes=[30, 41, 27, 20, 30, 30, 45, 24])
    clusters = P.side_clusters(cands, 4)
    assert clusters[0] == [[0, 0, 4, 5, 41], [0, 1, 5, 5, 27], [2, 0, 9, 9, 20]]      # adjacent bins of one (t, s) only
    assert clusters[1] == [[1, 0, 7, 7, 45], [0, 0, 7, 7, 30], [0, 0, 9, 9, 30]] and clusters[2] == []
    assert P.unique_side(clusters[0], 24) == (41, 27, [0, 0, 4, 5, 41])               # 41 > 1.5 * 27 = 40.5
    assert P.unique_side([[0, 0, 4, 5, 40], [0, 1, 5, 5, 27]], 24) == (40, 27, None)
    assert P.unique_side(clusters[1], 24) == (45, 30, None)                           # 45 = 1.5 * 30: not above it
    assert P.unique_side(clusters[2], 24) == (0, 0, None)
    assert P.unique_side(clusters[3], 24)[2] == [5, 1, -3, -3, 24] and P.unique_side(clusters[3], 25)[2] is None


def test_locus_status_rule():
    side = lambda chrom, strand, edge, votes=100: dict(votes=votes, second=0, chrom=chrom, strand=strand, edge=edge)
    weak = lambda votes: dict(votes=votes, second=votes)
    st = lambda l, r, span=50000: P.locus_status(l, r, 64, 24, span)
    assert st(side("c", "+", 500), side("c", "+", 530)) == ("placed", "c", "+", 500, 530)
    assert st(side("c", "-", 530), side("c", "-", 500)) == ("placed", "c", "-", 500, 530)   # - strand: L is the end
    assert st(side("c", "+", 500), side("c", "+", 436))[0] == "placed"                      # span -bin
    assert st(side("c", "+", 500), side("c", "+", 435))[0] == "discordant"
    assert st(side("c", "+", 500), side("c", "+", 50500))[0] == "placed"
    assert st(side("c", "+", 500), side("c", "+", 50501))[0] == "discordant"
    assert st(side("c", "+", 500), side("c", "+", 600), span=99)[0] == "discordant"
    assert st(side("c", "+", 500), side("d", "+", 530))[0] == st(side("c", "+", 500), side("c", "-", 530))[0] == "discordant"
    assert st(side("c", "+", 500), weak(100)) == ("left_only", "c", "+", 500, None) == st(side("c", "+", 500), None)
    assert st(side("c", "-", 500), None) == ("left_only", "c", "-", None, 500)
    assert st(None, side("c", "+", 500)) == ("right_only", "c", "+", None, 500)
    assert st(weak(0), side("c", "-", 500)) == ("right_only", "c", "-", 500, None)
    assert st(weak(24), weak(0))[0] == st(None, weak(24))[0] == "ambiguous"
    assert st(weak(23), weak(0))[0] == st(weak(23), None)[0] == "unplaced"
    assert P.bed_unit("CCCTT", 350, "-") == "AAGGG" and P.bed_unit("CCCTT", 352, "-") == "GGAAG"   # rc(CCCTT x 70 + CC)
    assert P.bed_unit("AAGGG", 352, "+") == "AAGGG"


def _run(tmp_path, name, p, oracle, **kw):
    fq, fa = cases.write_panel(p, tmp_path)
    pipeline.discover_repeats(fq, str(tmp_path / name), engine=scan_engine, group_loci=True,
                              sketch_engine=sketch_ref.engine, place_engine=R.Engine(), place_aligner=oracle.align_pairs,
                              **kw)
    return fq, fa


def _tables(tmp_path, name):
    """{locus name: the placed row} (the locus named by its representative read) and the BED rows."""
    read = lambda f: [l.split("\t") for l in open(tmp_path / f"{name}.{f}").read().splitlines()]
    loci = read("discovered_loci.tsv")
    rep = {row[0]: row[loci[0].index("Rep_Read")].split("_")[0] for row in loci[1:]}
    placed = read("discovered_loci_placed.tsv")
    assert tuple(placed[0]) == P.PLACED_COLUMNS
    return {rep[row[0]]: dict(zip(placed[0], row)) for row in placed[1:]}, read("discovered_loci.ref.bed")


def test_every_status_on_a_planted_reference(oracle, tmp_path, capsys):
    p = cases.planted_panel()
    bed = tmp_path / "catalogue.bed"
    lo, hi = 6200 - 2 * 64, 6215 + 2 * 64                  # p3's tract with the pad
    bed.write_text(f"chrA\t6000\t{lo}\tAAGGG\nA\t6000\t{lo + 1}\tAAGGG\nchrA\t{hi - 1}\t6400\tAAGGG\n"
                   f"chrA\t{hi}\t6400\tAAGGG\nchrB\t8210\t8220\tAAGGG\nchrB\t21000\t{21880 - 128}\tAAGGG\n")
    fq, fa = _run(tmp_path, "off", p, oracle, repeat_region_bed=str(bed))
    capsys.readouterr()
    _run(tmp_path, "on", p, oracle, repeat_region_bed=str(bed), place_ref=str(tmp_path / "ref.fa"))
    err = capsys.readouterr().err
    assert "NOTICE: of 10 locus/loci with a side to place on" in err
    assert "5 placed, 1 left_only, 1 right_only, 1 discordant, 1 ambiguous, 1 unplaced" in err

    # every file that existed before is byte for byte what it was
    names = lambda prefix: {f[len(prefix) + 1:] for f in os.listdir(tmp_path) if f.startswith(prefix + ".")}
    assert names("on") - names("off") == {"discovered_loci_placed.tsv", "discovered_loci.ref.bed"}
    for f in names("off"):
        assert open(tmp_path / f"on.{f}", "rb").read() == open(tmp_path / f"off.{f}", "rb").read(), f

    rows, ref_bed = _tables(tmp_path, "on")
    assert set(rows) == {"p3", "p11", "p0", "amb", "disc", "unp", "overs", "overe", "openr", "openl"}
    for x in ("p3", "p11", "p0", "overs", "overe"):        # error-free representatives: the planted coordinates
        chrom, strand, start, end = p["truth"][x]
        r = rows[x]
        assert (r["Status"], r["Chrom"], r["Strand"], r["Ref_Start"], r["Ref_End"]) == (
            "placed", chrom, strand, str(start), str(end)), x
        assert (r["Ref_Span"], r["Ref_Copies"]) == (str(end - start), str((end - start) // 5))
    assert [rows[x]["Ref_Copies"] for x in ("p3", "p11", "p0")] == ["3", "11", "0"]
    assert (rows["p11"]["Unit"], rows["p11"]["Median_Copies"], rows["p11"]["Max_Copies"]) == ("CCCTT", "70", "70")
    # a side overhanging the contig's start votes with the 400 bases inside it, one overhanging its end with 300
    assert int(rows["overs"]["Left_Votes"]) == 400 - 14 and int(rows["overe"]["Right_Votes"]) == 300 - 14
    assert int(rows["p3"]["Left_Votes"]) == 1000 - 14 and rows["p3"]["Left_Second"] == "0"
    a = rows["amb"]
    assert a["Status"] == "ambiguous" and a["Left_Votes"] == a["Left_Second"] == "986" and a["Chrom"] == a["Ref_Start"] == "-"
    assert rows["disc"]["Status"] == "discordant" and rows["disc"]["Left_Votes"] == rows["disc"]["Right_Votes"] == "986"
    u = rows["unp"]
    assert (u["Status"], u["Left_Votes"], u["Right_Votes"], u["Ref_Copies"], u["Catalogued"]) == ("unplaced", "0", "0", "-", "-")
    r, l = rows["openr"], rows["openl"]
    assert (r["Status"], r["Type"], r["Chrom"], r["Ref_Start"], r["Ref_End"], r["Left_Votes"]) == (
        "right_only", "open_D", "chrB", "-", "21880", "-")
    assert (l["Status"], l["Type"], l["Chrom"], l["Ref_Start"], l["Ref_End"], l["Right_Votes"]) == (
        "left_only", "open_U", "chrC", "20630", "-", "-")
    # Catalogued by overlap with the tract +- 2 bin: a row that ends at the pad's first base or starts at its last one
    # overlaps, one base further it does not; either naming of the contig
    assert [rows[x]["Catalogued"] for x in ("p3", "p11", "p0", "openr", "openl")] == ["2", "1", "0", "0", "0"]

    assert ref_bed == [["chrB", "8200", "8255", "AAGGG"], ["chrA", "6200", "6215", "AAGGG"], ["chrC", "400", "415", "AAGGG"],
                       ["chrA", "46230", "46245", "AAGGG"], ["chrC", "8815", "8815", "AAGGG"]]
    regions = nr_io.read_repeat_region_file(str(tmp_path / "on.discovered_loci.ref.bed"), True)
    ref = nr_io.fasta_file2dict(fa)
    for region in regions:                                 # the feedback inputs load, and the motif check passes
        nr_io.extract_ref_sequence(ref, region, 1000)
        assert nr_io.check_repeat_motif_in_ref(region)

    # other options reach the rule: a span limit below p11's 55 bases, and sides too short to reach min_votes
    _run(tmp_path, "span", p, oracle, place_ref=fa, max_ref_span=54, no_details=True)
    assert {x: r["Status"] for x, r in _tables(tmp_path, "span")[0].items() if r["Status"] == "discordant"} == {
        "disc": "discordant", "p11": "discordant"}
    _run(tmp_path, "short", p, oracle, place_ref=fa, place_flank_len=60, place_min_votes=50, place_bin=16, place_k=11)
    short = _tables(tmp_path, "short")[0]
    assert short["p3"]["Status"] == "placed" and short["p3"]["Left_Votes"] == "50" and short["p3"]["Ref_Start"] == "6200"
    _run(tmp_path, "shorter", p, oracle, place_ref=fa, place_flank_len=60, place_min_votes=51, place_bin=16, place_k=11)
    assert _tables(tmp_path, "shorter")[0]["p3"]["Status"] == "unplaced"


@pytest.mark.parametrize("model", ["ont", "hifi"])
def test_noisy_representatives_overlap_the_planted_tracts(oracle, tmp_path, model, capsys):
    """The largest deviation of a boundary from the planted one is printed (ont 8, hifi 5)."""
    p = cases.planted_panel(model)
    _, fa = _run(tmp_path, "noisy", p, oracle, place_ref=str(tmp_path / "ref.fa"))
    rows, _ = _tables(tmp_path, "noisy")
    worst = 0
    for x in ("p3", "p11", "p0", "overs", "overe"):
        chrom, strand, start, end = p["truth"][x]
        r = rows[x]
        assert (r["Status"], r["Chrom"], r["Strand"]) == ("placed", chrom, strand), (x, r)
        assert int(r["Ref_Start"]) <= end + 128 and int(r["Ref_End"]) >= start - 128, (x, r)
        worst = max(worst, abs(int(r["Ref_Start"]) - start), abs(int(r["Ref_End"]) - end))
    assert rows["amb"]["Status"] == "ambiguous" and rows["unp"]["Status"] == "unplaced"
    with capsys.disabled():
        print(f"\n{model}: largest deviation of a placed boundary {worst} base(s)")


def test_bad_values(tmp_path):
    for bad in (dict(place_k=12), dict(place_k=17), dict(place_k=13.0), dict(place_bin=0), dict(place_bin=4097),
                dict(place_min_votes=0), dict(place_max_occ=0), dict(place_max_occ=256), dict(place_max_target_occ=0),
                dict(place_max_target_occ=1025), dict(place_flank_len=12), dict(place_flank_len=2049),
                dict(max_ref_span=-1), dict(max_ref_span="far")):
        with pytest.raises(ValueError):
            pipeline.discover_repeats("nowhere.fastq", "nowhere", group_loci=True, place_ref="nowhere.fa", **bad)
        with pytest.raises(ValueError):
            pipeline.quantify_from_reads("r.fq", "ref.fa", "x.bed", "out", discover_repeats=True, group_loci=True,
                                         place_loci=True, **bad)
    with pytest.raises(ValueError, match="group_loci"):
        pipeline.discover_repeats("nowhere.fastq", "nowhere", place_ref="nowhere.fa")
    with pytest.raises(ValueError, match="group_loci"):
        pipeline.quantify_from_reads("r.fq", "ref.fa", "x.bed", "out", discover_repeats=True, place_loci=True)
    for f in (pipeline.discover_repeats, pipeline.quantify_from_reads):
        sig = inspect.signature(f).parameters
        assert (sig["place_k"].default, sig["place_bin"].default, sig["place_min_votes"].default) == (P.K, P.BIN, None)
        assert (sig["place_max_occ"].default, sig["place_max_target_occ"].default) == (P.MAX_OCC, P.MAX_TARGET_OCC)
        assert (sig["place_flank_len"].default, sig["max_ref_span"].default) == (P.FLANK_LEN, P.MAX_REF_SPAN) == (1000, 50000)
    assert inspect.signature(pipeline.discover_repeats).parameters["place_ref"].default is None
    assert inspect.signature(pipeline.quantify_from_reads).parameters["place_loci"].default is False
    assert P.check_options() == P.MIN_VOTES and P.OCC_CEILING == R.CEILING == cases.CEILING


# ----------------------------------------------------------------------------------- the defaults
def _best_votes(model, k, bins, n=100, contig_len=250_000, n_contigs=4):
    """{bin: (the best votes of n true sides of 1000, 500 and 300 bases, of n decoy sides)} against a random reference
    of n_contigs contigs: the true sides are cut from it and go through the error channel, every second one reverse-
    complemented; the decoys are unrelated 1000-base sequences."""
    rng = np.random.default_rng(3100 + len(model))
    contigs = [synth.rand_seq(rng, contig_len) for _ in range(n_contigs)]
    queries, kind = [], []
    for length in (1000, 500, 300):
        for i in range(n):
            t, at = int(rng.integers(n_contigs)), int(rng.integers(0, contig_len - length))
            side = synth.apply_errors(rng, contigs[t][at:at + length], model)[:P.MAX_SIDE]
            queries.append(synth.revcomp(side) if i % 2 else side)
            kind.append(length)
    queries += [synth.rand_seq(rng, 1000) for _ in range(n)]
    kind = np.array(kind + [0] * n)
    e = R.Engine()
    h = e.place_create(queries, k, P.MAX_OCC)
    for t, contig in enumerate(contigs):
        e.place_scan(h, t, 0, contig)
    out = {}
    for bin in bins:
        got = e.place_candidates(h, bin, P.MAX_TARGET_OCC, 1)
        best = np.zeros(len(queries), int)
        np.maximum.at(best, got["query"], got["votes"])
        out[bin] = {length: best[kind == length] for length in (1000, 500, 300, 0)}
    return out


def test_default_table(capsys):
    """100 sides per line against 1 Mb of random reference, seeded.  At the defaults (k = 15,
    bin = 64) the smallest best vote of a true 1000-base side is at or above min_votes and the largest vote of a decoy
    is below it, for both models.  The other k and bin, and the sides of 500 and 300 bases, are recorded, not
    asserted."""
    assert (P.K, P.BIN, P.MIN_VOTES) == (15, 64, 24)
    for model in ("ont", "hifi"):
        for k in (11, 13, 15):
            table = _best_votes(model, k, (16, 32, 64, 128))
            for bin, v in table.items():
                with capsys.disabled():
                    print(f"\n{model} k {k} bin {bin}: " + "; ".join(
                        f"true {n} min {v[n].min()} median {int(np.median(v[n]))}" for n in (1000, 500, 300)) +
                        f"; decoy max {v[0].max()}", end="")
                if (k, bin) == (P.K, P.BIN):
                    assert v[0].max() < P.MIN_VOTES <= v[1000].min()
