"""A 3-region FASTQ panel with an allele no read spans, for the FASTQ command's partial_reads / in_repeat_reads
(tests/test_in_repeat_cpu.py with stand-in engines, tests/test_screen_partial_gpu.py on the device), and the checks
both make on its output files."""
import os

import numpy as np

from nanorepeat_amd import synth

LONG_UNITS = 400          # the long allele: 1200 tract bases; the reads are 600 to 900 bases long
ANCHOR_LEN = 300


def write_panel(tmp_path, seed=8):
    """ref.fa, r.bed, in.fastq under tmp_path.  Region 0 (CAG): reads span a 20-unit allele; a 400-unit allele is seen
    only by reads that end inside the tract (6 anchored left, 6 right) and by 8 reads that lie wholly in it.  Region
    1 (TATTG, 6 / 17 units) and region 2 (GGCCCC, 5 / 9 units) have spanning reads only.  12 random decoys.  Half of
    every kind is reverse-complemented.  Returns {kind: [names]}."""
    rng = np.random.default_rng(seed)
    chrom = synth.rand_seq(rng, 1500)
    spans = []
    for unit, kref in (("CAG", 12), ("TATTG", 8), ("GGCCCC", 5)):
        st = len(chrom); chrom += unit * kref; spans.append((st, len(chrom), unit)); chrom += synth.rand_seq(rng, 1500)
    (tmp_path / "ref.fa").write_text(">chr7\n" + "\n".join(chrom[i:i + 80] for i in range(0, len(chrom), 80)) + "\n")
    (tmp_path / "r.bed").write_text("".join(f"chr7\t{st}\t{en}\t{u}\n" for st, en, u in spans))
    reads, names = [], dict(spanning=[], left=[], right=[], inside=[], decoy=[])

    def add(kind, name, seq, flip):
        assert 600 <= len(seq) <= 900 or kind == "spanning", (name, len(seq))
        names[kind].append(name)
        reads.append((name, synth.revcomp(seq) if flip else seq))

    for g, ((st, en, unit), alleles) in enumerate(zip(spans, ((20, 20), (6, 17), (5, 9)))):
        for i in range(12):
            lo, ro = 310 + 5 * i, 320 + 4 * i
            s = synth.apply_errors(rng, chrom[st - lo:st] + unit * alleles[i % 2] + chrom[en:en + ro], "ont_q20")
            add("spanning", f"g{g}s{i:02d}", s, i % 3 == 0)
    st, en, _ = spans[0]
    tract = "CAG" * LONG_UNITS
    for i in range(6):
        L = 290 + 50 * i
        add("left", f"g0l{i}", chrom[st - 320:st] + tract[:L], i % 2 == 1)
        add("right", f"g0r{i}", tract[len(tract) - L - 7:] + chrom[en:en + 330], i % 2 == 0)
    for i in range(8):
        n = 630 + 35 * i
        add("inside", f"g0i{i}", synth.apply_errors(rng, tract[i:i + n], "hifi" if i % 2 else "ont_q20"), i % 2 == 1)
    for i in range(12):
        add("decoy", f"decoy{i:02d}", synth.rand_seq(rng, int(rng.integers(600, 901))), False)
    order = rng.permutation(len(reads))
    (tmp_path / "in.fastq").write_text("".join(f"@{reads[i][0]}\n{reads[i][1]}\n+\n{'5' * len(reads[i][1])}\n"
                                               for i in order))
    return names


def tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


NEW_DETAIL_FILES = (".partial_reads.tsv", ".in_repeat_reads.tsv", ".partial_candidates.fastq")
NEW_SUMMARIES = (".NanoRepeat_partial.tsv", ".NanoRepeat_in_repeat.tsv")


def run_and_check(tmp_path, capsys, **engines):
    """The FASTQ command with the switches off, on, and on without the screen; returns (regions, names, stderr)."""
    from nanorepeat_amd import pipeline
    names = write_panel(tmp_path)
    args = (str(tmp_path / "in.fastq"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=ANCHOR_LEN, seed=1, **engines)
    pipeline.quantify_from_reads(*args, str(tmp_path / "off"), **common)
    capsys.readouterr()
    regions = pipeline.quantify_from_reads(*args, str(tmp_path / "on"), partial_reads=True, in_repeat_reads=True, **common)
    err = capsys.readouterr().err
    pipeline.quantify_from_reads(*args, str(tmp_path / "all"), partial_reads=True, in_repeat_reads=True, screen=False,
                                 **common)

    # every file that exists without the switches is byte for byte what it was
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off, exhaustive = tree(tmp_path / "on.details"), tree(tmp_path / "off.details"), tree(tmp_path / "all.details")
    assert {k: v for k, v in on.items() if not k.endswith(NEW_DETAIL_FILES)} == off
    assert not any(k.endswith(NEW_DETAIL_FILES) for k in off)
    assert not any((tmp_path / ("off" + s)).exists() for s in NEW_SUMMARIES)
    # the exhaustive form writes the same partial and in-repeat files
    for s in NEW_SUMMARIES:
        assert (tmp_path / ("on" + s)).read_bytes() == (tmp_path / ("all" + s)).read_bytes(), s
    for k, v in on.items():
        if k.endswith(NEW_DETAIL_FILES[:2]):
            assert exhaustive[k] == v, k
    assert sum(k.endswith(".in_repeat_reads.tsv") for k in on) == 3

    # the long allele shows in region 0 and nowhere else
    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_partial.tsv").read_text().split("\n")[1:] if l]
    assert [r[3] for r in rows] == ["CAG", "TATTG", "GGCCCC"]
    assert rows[0][4] == "12" and int(rows[0][6]) == 6 and int(rows[0][7]) == 6
    assert int(rows[0][9]) > 0 and int(rows[0][8]) > 20
    assert all(r[6:] == ["0", "0", "-", "0"] for r in rows[1:])
    text = (tmp_path / "on.NanoRepeat_in_repeat.tsv").read_text().split("\n")
    assert text[0].startswith("##Shared_Motif_Regions")
    assert text[1] == "#Chrom\tStart\tEnd\tMotif\tNum_Spanning\tMax_Spanning_Size\tNum_In_Repeat\tMax_Repeat_Units\t" \
                      "Num_Exceeding\tShared_Motif_Regions"
    rows = [l.split("\t") for l in text[2:] if l]
    assert rows[0][6] == "8" and int(rows[0][8]) == 8 and int(rows[0][7]) > 150 and rows[0][9] == "1"
    assert all(r[6:] == ["0", "-", "0", "1"] for r in rows[1:])
    detail = [v for k, v in on.items() if k.endswith(".in_repeat_reads.tsv") and b"##Motif=CAG\n" in v][0].decode()
    lines = detail.split("\n")
    assert lines[2] == "#Read_Name\tStrand\tEnd\tRead_Len\tExtended_Bases\tMotif_Bases\tRepeat_Units\tScore\tExceeds_Spanning"
    got = [l.split("\t") for l in lines[3:] if l]
    assert sorted(r[0] for r in got) == sorted(names["inside"])
    assert {r[1] for r in got} == {"+", "-"} and all(r[2] in ("start", "end") for r in got)
    assert all(int(r[6]) == int(r[5]) // 3 and int(r[6]) > 150 for r in got)
    # the candidates never reach the region's reads or its sizes
    cand = [v for k, v in on.items() if k.endswith(".partial_candidates.fastq")]
    assert len(cand) == 3 and sorted(len(v) > 0 for v in cand) == [False, False, True]
    assert not set(regions[0].read_dict) & set(names["left"] + names["right"] + names["inside"])
    notices = [l for l in err.split("\n") if l.startswith("NOTICE")]
    assert sum("one-anchor read(s) show" in l for l in notices) == 1
    assert sum("in-repeat read(s) show" in l for l in notices) == 1
    return regions, names, err
