"""The placement commands on the device: discovery with group_loci=True and place_ref on a planted
panel with its reference, then the FASTQ command on that reference and the BED file the placement wrote."""
import pytest

import place_cases as cases
import place_ref as R
from nanorepeat_amd import place as P, pipeline

pytestmark = pytest.mark.gpu


def table(path):
    lines = [l.split("\t") for l in open(path).read().splitlines()]
    return [dict(zip(lines[0], l)) for l in lines[1:]]


def test_planted_loci_are_placed_and_sized_on_the_reference(capi, tmp_path, capsys):
    p = cases.loci_panel("hifi")
    fq, fa = cases.write_panel(p, tmp_path)
    pipeline.discover_repeats(fq, str(tmp_path / "off"), group_loci=True)
    pipeline.discover_repeats(fq, str(tmp_path / "on"), group_loci=True, place_ref=fa)
    assert "3 placed, 0 left_only, 0 right_only, 0 discordant, 0 ambiguous, 0 unplaced" in capsys.readouterr().err
    pipeline.discover_repeats(fq, str(tmp_path / "cpu"), group_loci=True, place_ref=fa, place_engine=R.Engine())

    # three placed rows on the planted contigs and strands, their intervals over the planted tracts
    placed = table(tmp_path / "on.discovered_loci_placed.tsv")
    rep = {c["Locus"]: c["Rep_Read"] for c in table(tmp_path / "on.discovered_loci.tsv")}
    assert tuple(placed[0]) == P.PLACED_COLUMNS and [c["Status"] for c in placed] == ["placed"] * 3
    by_locus = {p["locus"][rep[c["Locus"]]]: c for c in placed}
    assert set(by_locus) == {"A", "B", "C"}
    for x, c in by_locus.items():
        chrom, start, end = p["truth"][x]
        assert (c["Chrom"], c["Strand"]) == (chrom, p["strand"][rep[c["Locus"]]]), (x, c)
        assert int(c["Ref_Start"]) <= end and int(c["Ref_End"]) >= start, (x, c)
        assert c["Left_Second"] == c["Right_Second"] == "0"
    assert by_locus["A"]["Strand"] == "+" and by_locus["C"]["Strand"] == "-"

    # the device's files equal those made with the restatement as the engine; the files that existed are what they were
    for name in ("discovered_loci_placed.tsv", "discovered_loci.ref.bed"):
        assert (tmp_path / f"on.{name}").read_bytes() == (tmp_path / f"cpu.{name}").read_bytes()
    old = {f.name[4:] for f in tmp_path.glob("off.*")}
    assert {f.name[3:] for f in tmp_path.glob("on.*")} - old == {"discovered_loci_placed.tsv", "discovered_loci.ref.bed"}
    for name in old:
        assert (tmp_path / f"on.{name}").read_bytes() == (tmp_path / f"off.{name}").read_bytes(), name

    # the FASTQ command on the real reference and the written BED file: the motif check passes on all three and locus A's
    # two alleles are sized; its own place_loci switch writes the same placement
    regions = pipeline.quantify_from_reads(fq, fa, str(tmp_path / "on.discovered_loci.ref.bed"), str(tmp_path / "sized"),
                                           data_type="hifi", anchor_len=1000, seed=1, mixture="gpu",
                                           discover_repeats=True, group_loci=True, place_loci=True)
    assert sorted(r.chrom for r in regions) == ["chrA", "chrB", "chrC"]
    assert not any(getattr(r, "ref_has_issue", True) for r in regions)
    a = next(r for r in regions if r.chrom == "chrA")
    sizes = sorted(x.repeat_size1 for x in a.results.quantified_allele_list)
    assert len(sizes) == 2 and abs(sizes[0] - p["alleles"][0]) <= 1 and abs(sizes[1] - p["alleles"][1]) <= 1
    again = table(tmp_path / "sized.discovered_loci_placed.tsv")
    assert [{k: v for k, v in c.items() if k != "Catalogued"} for c in again] == \
        [{k: v for k, v in c.items() if k != "Catalogued"} for c in placed]
    assert [c["Catalogued"] for c in again] == ["1"] * 3 and [c["Catalogued"] for c in placed] == ["-"] * 3
