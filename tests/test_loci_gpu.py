"""The locus commands on the device: discovery with group_loci=True on a planted panel, then the
FASTQ command on the pseudo-reference and BED file it wrote."""
import pytest

import sketch_cases as cases
from nanorepeat_amd import loci as L, pipeline

pytestmark = pytest.mark.gpu


def round_trip(directory, model, data_type):
    """Writes the panel, runs discovery without and with group_loci and the FASTQ command on the written files.
    Returns (panel, the locus table as dicts, the per-run table as lists, the regions of the FASTQ command)."""
    p = cases.loci_panel(model)
    fq = directory / "reads.fastq"
    fq.write_text("".join(f"@{n}\n{s}\n+\n{'5' * len(s)}\n" for n, s in p["reads"]))
    pipeline.discover_repeats(str(fq), str(directory / "off"))
    pipeline.discover_repeats(str(fq), str(directory / "on"), group_loci=True)
    lines = [l.split("\t") for l in (directory / "on.discovered_loci.tsv").read_text().splitlines()]
    table = [dict(zip(lines[0], l)) for l in lines[1:]]
    runs = [l.split("\t") for l in (directory / "on.discovered_locus_runs.tsv").read_text().splitlines()[1:]]
    regions = pipeline.quantify_from_reads(str(fq), str(directory / "on.discovered_loci.fa"),
                                           str(directory / "on.discovered_loci.bed"), str(directory / "sized"),
                                           data_type=data_type, anchor_len=1000, seed=1, mixture="gpu")
    return p, table, runs, regions


def test_planted_loci_and_the_feedback_path(capi, tmp_path, capsys):
    p, table, runs, regions = round_trip(tmp_path, "hifi", "hifi")
    err = capsys.readouterr().err
    assert "NOTICE: the discovered runs form 3 core locus/loci (3 with at least 3 spanned runs) and 0 open" in err
    assert "0 ambiguous and 0 unplaced run(s)" in err

    # exactly the planted core loci with the planted read sets; the open reads go to B
    assert tuple(table[0]) == L.LOCUS_COLUMNS and [c["Type"] for c in table] == ["core"] * 3
    members = {}
    for name, _, _, cls, locus, role, _ in runs:
        members.setdefault(locus, {}).setdefault(role, set()).add(name)
    planted = {x: {n for n, y in p["locus"].items() if y == x} for x in "ABC"}
    by_core = {frozenset(m["core"]): (locus, m) for locus, m in members.items()}
    assert set(by_core) == {frozenset(s) for s in planted.values()}
    locus_b, b = by_core[frozenset(planted["B"])]
    assert b["attached"] == p["open"] and sum("attached" in m for _, m in by_core.values()) == 1
    assert not any(r[0].startswith("decoy") for r in runs)
    row = {c["Locus"]: c for c in table}
    assert row[locus_b]["Class"] == "AAGGG" and int(row[locus_b]["Left_Open"]) + int(row[locus_b]["Right_Open"]) == 4
    locus_a = by_core[frozenset(planted["A"])][0]
    assert (row[locus_a]["Spanned"], row[locus_a]["Class"]) == ("16", "AAGGG")
    assert abs(int(row[locus_a]["Min_Copies"]) - 60) <= 3 and abs(int(row[locus_a]["Max_Copies"]) - 100) <= 3

    # every file that existed before is byte for byte what it was
    for name in ("discovered_runs.tsv", "NanoRepeat_discovered.tsv"):
        assert (tmp_path / f"on.{name}").read_bytes() == (tmp_path / f"off.{name}").read_bytes()
    new = {f.name[3:] for f in tmp_path.glob("on.*")} - {f.name[4:] for f in tmp_path.glob("off.*")}
    assert new == {"discovered_loci.tsv", "discovered_locus_runs.tsv", "discovered_loci.fa", "discovered_loci.bed"}

    # the FASTQ command on the written files: the motif check passes and locus A's two alleles are sized
    assert [r.chrom for r in regions] == [f"locus_{i}" for i in (1, 2, 3)]
    assert not any(getattr(r, "ref_has_issue", True) for r in regions)
    a = next(r for r in regions if r.chrom == f"locus_{locus_a}")
    sizes = sorted(x.repeat_size1 for x in a.results.quantified_allele_list)
    assert len(sizes) == 2 and abs(sizes[0] - p["alleles"][0]) <= 1 and abs(sizes[1] - p["alleles"][1]) <= 1
