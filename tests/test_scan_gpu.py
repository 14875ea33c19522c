"""nra_scan_repeats on the device against tests/scan_ref.py: every comparison is exact, runs and
the counters n_windows, n_periodic and n_segments."""
import ctypes as C

import numpy as np
import pytest

import scan_cases as cases
import scan_ref as R
from in_repeat_panel import tree
from nanorepeat_amd import discover as D, synth

pytestmark = pytest.mark.gpu
KEYS = ("read", "start", "end", "cls", "windows", "fwd_windows")
COUNTERS = ("n_windows", "n_periodic", "n_segments")


def as_tuples(got):
    return list(zip(*(got[key].tolist() for key in KEYS)))


def same(capi, c, reads=None):
    """The device's result for a case equals the restatement's; returns (runs, stats)."""
    reads = c["reads"] if reads is None else reads
    got = capi.scan_repeats(reads, c["k"], c["max_gap"], c["min_span"])
    want, stats = R.scan(reads, c["k"], c["max_gap"], c["min_span"])
    assert as_tuples(got) == want
    assert {key: got["stats"][key] for key in COUNTERS} == stats
    return want, got["stats"]


@pytest.mark.parametrize("k", [8, 11, 15])
def test_kernel_edges(capi, k):
    c = cases.edge_case(k)
    runs, st = same(capi, c)
    of = lambda r: [x for x in runs if x[0] == r]
    assert of(0) == [] and of(1) == [(1, 0, k, 0, 1, 1)] and of(2) == [(2, 0, k + 1, 0, 2, 2)] and of(5) == []
    assert [x[3] for r in (10, 11, 12) for x in of(r)] == [D.class_id(w) for w in ("A", "AC", "ACG")]
    assert len(of(8)) == 2                                                  # one N inside a pure run
    n = len(c["reads"][16])
    a, b = max(of(16), key=lambda x: x[2] - x[1]), max(of(17), key=lambda x: x[2] - x[1])
    assert a[3] == b[3] == D.class_id("AAGGG") and b[1:3] == (n - a[2], n - a[1]) and (a[5], b[5]) == (a[4], 0)
    for r in (18, 19, 20, 21):                                               # AT, ACGT: forward on both strands
        x = max(of(r), key=lambda x: x[2] - x[1])
        assert x[4] == x[5] and D.class_word(x[3]) in ("AT", "ACGT")
    assert st["n_chunks"] == 1 and st["kernel_ms"] > 0


def test_boundaries(capi):
    c = cases.boundary_case()
    runs, _ = same(capi, c)
    aaat = D.class_id("AAAT")
    assert [x[0] for x in runs if x[3] == aaat] == [41, 42]                # two islands, never one across two reads
    _, st = same(capi, c, [c["reads"][24]])                                 # a pure 10 000-base read
    assert st["n_segments"] == 3 and st["n_periodic"] == st["n_windows"] == 10000 - c["k"] + 1
    for r in (6, 7, 12, 13):                                                 # each alone: its tiles start at offset 0
        same(capi, c, [c["reads"][r]])


def test_island_rule(capi):
    read, k = cases.gap_read(), 11
    _, cid, _ = R.read_windows(read, k)
    ac, aag = D.class_id("AC"), D.class_id("AAG")
    gap = int(np.diff(np.flatnonzero(cid == ac)).max())
    one, _ = same(capi, cases.case([read], k, gap, k))
    two, _ = same(capi, cases.case([read], k, gap - 1, k))
    assert [x[3] for x in one] == [ac, aag] and [x[3] for x in two] == [ac, aag, ac]
    span = two[0][2] - two[0][1]
    at, _ = same(capi, cases.case([read], k, gap - 1, span))
    above, _ = same(capi, cases.case([read], k, gap - 1, span + 1))
    assert [x[1] for x in at][:1] == [0] and 0 not in [x[1] for x in above]


def test_host_paths(capi, monkeypatch, capfd):
    c = cases.fuzz_case(40, seed=5)
    reads = c["reads"][:40]                                                  # without the 70 000-base read
    want, stats = R.scan(reads, c["k"], c["max_gap"], c["min_span"])
    assert len(want) > 20
    monkeypatch.setenv("NRA_DEBUG", "1")
    monkeypatch.setenv("NRA_TEST_SCAN_CHUNK_BYTES", "9000")
    monkeypatch.setenv("NRA_TEST_SCAN_SEG_CAP", "1")
    capfd.readouterr()
    got = capi.scan_repeats(reads, c["k"], c["max_gap"], c["min_span"])
    err = capfd.readouterr().err
    assert as_tuples(got) == want and {key: got["stats"][key] for key in COUNTERS} == stats
    assert got["stats"]["n_chunks"] == err.count("nra_scan_repeats: chunk of") >= 4
    assert err.count("segment list grows from 1 to") >= 1
    monkeypatch.delenv("NRA_DEBUG")
    monkeypatch.delenv("NRA_TEST_SCAN_CHUNK_BYTES")
    monkeypatch.delenv("NRA_TEST_SCAN_SEG_CAP")
    again = capi.scan_repeats(reads, c["k"], c["max_gap"], c["min_span"])    # two calls in a row, the variables re-read
    assert as_tuples(again) == want and again["stats"]["n_chunks"] == 1 and capfd.readouterr().err == ""

    # the capacity protocol
    lib = capi.load()
    data, off = capi.pack_reads(reads)
    for cap in (len(want) - 1, len(want)):
        out = [np.full(len(want), -7, np.int32) for _ in KEYS]
        n = C.c_int64(cap)
        rc = lib.nra_scan_repeats(0, len(reads), data, capi._ptr(off, C.c_int64), c["k"], c["max_gap"], c["min_span"],
                                  C.byref(n), *(capi._ptr(a, C.c_int32) for a in out), None)
        assert n.value == len(want)
        if cap < len(want):
            assert rc == capi.E_RANGE and all((a == -7).all() for a in out)
        else:
            assert rc == 0 and list(zip(*(a.tolist() for a in out))) == want

    # a permutation of the reads permutes the result
    order = np.random.default_rng(1).permutation(len(reads))
    shuffled = capi.scan_repeats([reads[i] for i in order], c["k"], c["max_gap"], c["min_span"])
    assert sorted((int(order[x[0]]),) + x[1:] for x in as_tuples(shuffled)) == sorted(want)


def test_fuzz(capi):
    c = cases.fuzz_case()
    assert len(c["reads"]) == 301 and len(c["reads"][-1]) > 60000
    runs, st = same(capi, c)
    assert len(runs) > 300 and len({x[3] for x in runs}) > 50 and st["n_segments"] > 5 * len(runs)


def test_command_finds_the_class_no_region_names(capi, tmp_path, capsys):
    """quantify_from_reads(discover_repeats=True): a panel of CAG regions (four reads of a 100-unit allele among its
    reads), 12 reads that span a 400-copy AAGGG run, 12 reads wholly inside such a run and 20 decoys holding
    (motif)x20."""
    from nanorepeat_amd import pipeline
    rng = np.random.default_rng(4)
    p = synth.panel(n_regions=2, n_chroms=1, anchor_len=400, reads_per_region=8, model="ont_q20", seed=9, units=["CAG"])
    chrom, st, en, _ = p["regions"][0]
    reads = list(p["reads"])
    for i in range(4):
        s = p["ref"][chrom][st - 450:st] + "CAG" * 100 + p["ref"][chrom][en:en + 450]
        reads.append((f"long{i}", synth.apply_errors(rng, s, "hifi")))
    for i in range(12):
        s = synth.rand_seq(rng, 1000) + "AAGGG" * 400 + synth.rand_seq(rng, 1000)
        reads.append((f"span{i:02d}", synth.apply_errors(rng, s, "hifi")))
    for i, s in enumerate(cases.planted_reads(rng, "AAGGG", "ont", 12)):
        reads.append((f"inside{i:02d}", s))
    for i, motif in enumerate((cases.TABLE_MOTIFS * 3)[:20]):
        reads.append((f"decoy{i:02d}", cases.decoy_reads(rng, motif, 1)[0]))
    p["reads"] = [reads[i] for i in rng.permutation(len(reads))]
    ref, bed, fq = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, mixture="gpu")
    pipeline.quantify_from_reads(fq, ref, bed, str(tmp_path / "off"), **common)
    capsys.readouterr()
    pipeline.quantify_from_reads(fq, ref, bed, str(tmp_path / "on"), discover_repeats=True, **common)
    err = capsys.readouterr().err
    assert "NOTICE: 1 repeat class(es) have runs" in err

    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_discovered.tsv").read_text().splitlines()]
    assert tuple(rows[0]) == D.CLASS_COLUMNS
    by_class = {r[0]: dict(zip(rows[0], r)) for r in rows[1:]}
    assert rows[1][0] == "AAGGG" and set(by_class) == {"AAGGG", "AGC"}       # no row from a decoy
    assert by_class["AAGGG"]["Catalogued_Regions"] == "0" and by_class["AAGGG"]["Spanned"] == "12"
    assert int(by_class["AAGGG"]["In_Repeat"]) >= 11 and int(by_class["AAGGG"]["Max_Copies"]) >= 390
    assert int(by_class["AGC"]["Catalogued_Regions"]) >= 1 and int(by_class["AGC"]["Spanned"]) >= 4
    runs = [l.split("\t") for l in (tmp_path / "on.discovered_runs.tsv").read_text().splitlines()]
    assert tuple(runs[0]) == D.RUN_COLUMNS and not any(r[0].startswith("decoy") for r in runs[1:])
    assert list(dict.fromkeys(r[0] for r in runs[1:])) == [n for n, _ in p["reads"] if n in {r[0] for r in runs[1:]}]

    # every file that existed before is byte for byte what it was
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    assert tree(tmp_path / "on.details") == tree(tmp_path / "off.details")
    new = {f.name[3:] for f in tmp_path.glob("on.*")} - {f.name[4:] for f in tmp_path.glob("off.*")}
    assert new == {"discovered_runs.tsv", "NanoRepeat_discovered.tsv"}
