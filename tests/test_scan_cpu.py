"""The repeat scan on the CPU: the two restatements of tests/scan_ref.py against each other on the
GPU tests' inputs, the class ids, the measurement behind the defaults, discover.py's rules and files through a stand-in
engine, and the error contract of nra_scan_repeats."""
import ctypes as C
import inspect
import os
import re
import struct
import sys

import numpy as np
import pytest

import methylation_cases as K
import scan_cases as cases
import scan_ref as R
from nanorepeat_amd import discover as D, pipeline, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_RANGE = -1, -2, -3
CASES = {"edges8": lambda: cases.edge_case(8), "edges11": lambda: cases.edge_case(11),
         "edges15": lambda: cases.edge_case(15), "boundaries": cases.boundary_case,
         "gap": lambda: cases.case([cases.gap_read()], 11, 71, 11), "fuzz": lambda: cases.fuzz_case(60)}


def ref_engine(seqs, k, max_gap, min_span, device=0):
    """A stand-in for _capi.scan_repeats: the restatement in the binding's shape."""
    runs, stats = R.scan(list(seqs), k, max_gap, min_span)
    cols = np.array(runs, np.int32).reshape(len(runs), 6).T
    out = dict(zip(("read", "start", "end", "cls", "windows", "fwd_windows"), cols))
    out["stats"] = stats
    return out


# ----------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_plain_python(name):
    c = CASES[name]()
    got = R.scan_numpy(c["reads"], c["k"], c["max_gap"], c["min_span"])
    want = R.scan_loops(c["reads"], c["k"], c["max_gap"], c["min_span"])
    assert got == want
    assert len(want[0]) > 0 and want[1]["n_segments"] >= len(want[0])


def _runs(reads, k, max_gap, min_span):
    return R.scan(reads, k, max_gap, min_span)[0]


def test_the_cases_hold_what_they_are_for():
    for k in (8, 11, 15):
        c = cases.edge_case(k)
        runs = _runs(c["reads"], k, c["max_gap"], c["min_span"])
        of = lambda r: [x for x in runs if x[0] == r]
        assert of(0) == [] and of(4) == [] and of(5) == []                 # k - 1 bases, empty, all N
        assert of(1) == [(1, 0, k, 0, 1, 1)] and of(2) == [(2, 0, k + 1, 0, 2, 2)]
        agc = D.class_id("CAG")
        assert of(6) == [(6, 0, 200, agc, 200 - k + 1, 200 - k + 1)]       # lower case; AGC is a rotation of CAG
        assert of(7) == [(7, 0, 177, agc, 177 - k + 1, 177 - k + 1)]       # mixed case, in phase
        assert [x[1:4] for x in of(8)] == [(0, 150, D.class_id("AAAG")), (151, 301, D.class_id("AAAG"))]
        # the smallest period, never a multiple
        for r, word in ((10, "A"), (11, "AC"), (12, "ACG"), (13, "AAC")):
            assert [x[3] for x in of(r)] == [D.class_id(word)], (k, r)
        # a read and its reverse complement: the same class, mirrored positions, the other strand
        for fwd, rev in ((16, 17), (18, 19), (20, 21)):
            n = len(c["reads"][fwd])
            a, b = of(fwd), of(rev)
            long_a, long_b = max(a, key=lambda x: x[2] - x[1]), max(b, key=lambda x: x[2] - x[1])
            assert long_a[3] == long_b[3] and (long_b[1], long_b[2]) == (n - long_a[2], n - long_a[1])
            assert long_a[4] == long_b[4]
            if fwd == 16:
                assert long_a[5] == long_a[4] and long_b[5] == 0 and D.class_word(long_a[3]) == "AAGGG"
            else:                                                           # AT and ACGT: forward on both strands
                assert long_a[5] == long_a[4] and long_b[5] == long_b[4]
    c = cases.boundary_case()
    runs, stats = R.scan(c["reads"], c["k"], c["max_gap"], c["min_span"])
    first = [x for x in runs if x[0] % 2 == 0 and x[0] < 24 and x[2] - x[1] >= 300]
    assert [x[1] for x in first] == [b + d for b in (16, 1024, 4096, 8192) for d in (-1, 0, 1)]
    last = [max(x[2] for x in runs if x[0] == r) - c["k"] for r in range(1, 24, 2)]
    assert [x for x in last] == [b + d for b in (16, 1024, 4096, 8192) for d in (-1, 0, 1)]
    assert R.scan([c["reads"][24]], 11, 3, 11)[1]["n_segments"] == 3      # 9990 windows of one class: one per tile
    offsets = np.cumsum([0] + [len(s) for s in c["reads"][:41]])[25:41]
    assert sorted(o % 16 for o in offsets - offsets[0]) == list(range(16))
    aaat = D.class_id("AAAT")
    assert [x[0] for x in runs if x[3] == aaat] == [41, 42]                # two islands, never one across the reads


def test_island_rule_at_its_bounds():
    read, k = cases.gap_read(), 11
    _, cid, _ = R.read_windows(read, k)
    ac, aag = D.class_id("AC"), D.class_id("AAG")
    pos = np.flatnonzero(cid == ac)
    gap = int(np.diff(pos).max())
    assert gap > 1
    one, two = _runs([read], k, gap, k), _runs([read], k, gap - 1, k)
    assert [x[3] for x in one] == [ac, aag] and one[0][1:3] == (0, len(read))       # X, then Y inside X's gap
    assert [x[3] for x in two] == [ac, aag, ac]
    span = two[0][2] - two[0][1]                                                    # of the island that starts at 0
    assert [x[1] for x in _runs([read], k, gap - 1, span)][:1] == [0]
    assert 0 not in [x[1] for x in _runs([read], k, gap - 1, span + 1)]


# ----------------------------------------------------------------------------------- class ids
def test_class_ids_round_trip_over_all_words():
    n = 0
    for p in range(1, 7):
        for v in range(4 ** p):
            word = "".join("ACGT"[(v >> (2 * (p - 1 - j))) & 3] for j in range(p))
            n += 1
            assert D.class_word((4 ** p - 4) // 3 + v) == word
            cid = D.class_id(word)
            canon = D.class_word(cid)
            assert D.class_id(canon) == cid
            if not any(word == word[i:] + word[:i] for i in range(1, p)):     # primitive: the scan's own table
                assert (cid, True) == R.classify_word(canon) and cid == R.classify_word(word)[0]
                assert D.class_id(synth.revcomp(word)) == cid and D.class_id(word[1:] + word[:1]) == cid
    assert n == D.N_CLASS_IDS == 5460
    assert D.class_id("CAGCAG") == D.class_id("CTG") == D.class_id("agc") and D.class_word(D.class_id("CTG")) == "AGC"
    for bad in ("", "ACN", "AAAAAAC", None):
        with pytest.raises(ValueError):
            D.class_id(bad)
    for bad in (-1, 5460):
        with pytest.raises(ValueError):
            D.class_word(bad)


def test_self_complementary_classes_are_always_forward():
    for word in ("AT", "ACGT", "CG", "AATT", "GATC", "AAATTT", "ACGCGT"):
        for w in (word, synth.revcomp(word), word[1:] + word[:1]):
            assert R.classify_word(w)[1] is True, w
    assert R.classify_word("AAGGG")[1] is True and R.classify_word("CCCTT")[1] is False
    assert R.window_class("CTGCTGCTGCT") == (D.class_id("CAG"), False)


# ----------------------------------------------------------------------------------- the defaults
def default_table(k, max_gap, min_span, n_reads=200, seed=3, models=("ont", "hifi")):
    """The measurements of DESIGN.md 29.4 with the committed restatement -> dict: per model the lowest share of a
    planted read covered by the largest island of its class, that island's shortest span and the reads with more than
    one island of their class of at least min_span bases; the longest island of any class in random reads and in decoys
    holding (motif)x20."""
    rng = np.random.default_rng(seed)
    out = {}
    for model in models:
        cover, spans, split, total = [], [], 0, 0
        for motif in cases.TABLE_MOTIFS:
            cid = D.class_id(motif)
            for read in cases.planted_reads(rng, motif, model, n_reads):
                mine = [e - s for _, s, e, c, _, _ in _runs([read], k, max_gap, k) if c == cid]
                best = max(mine, default=0)
                cover.append(best / len(read))
                spans.append(best)
                split += sum(x >= min_span for x in mine) > 1
                total += 1
        out[model] = dict(lowest_cover=min(cover), shortest_span=min(spans), split=split, reads=total)
    longest = lambda reads: max((e - s for _, s, e, _, _, _ in _runs(reads, k, max_gap, k)), default=0)
    out["random"] = longest(cases.decoy_reads(rng, None, 3 * n_reads))
    out["decoy"] = max(longest(cases.decoy_reads(rng, motif, n_reads // 2)) for motif in cases.TABLE_MOTIFS)
    return out


def test_default_table():
    sig = inspect.signature(pipeline.discover_repeats).parameters
    k, max_gap, min_span = sig["k"].default, sig["max_gap"].default, sig["min_span"].default
    assert (k, max_gap, min_span) == tuple(inspect.signature(D.scan_reads).parameters[n].default
                                           for n in ("k", "max_gap", "min_span"))
    t = default_table(k, max_gap, min_span)
    print(f"\nk {k} max_gap {max_gap} min_span {min_span}: {t}")                  # shown with pytest -s
    assert max(t["random"], t["decoy"]) < min_span, t
    for model in ("ont", "hifi"):
        assert t[model]["shortest_span"] >= min_span and t[model]["lowest_cover"] >= 0.5, (model, t[model])
        assert t[model]["split"] * 100 <= t[model]["reads"], (model, t[model])


# ----------------------------------------------------------------------------------- discover.py
def _fixed_engine(runs):
    def engine(seqs, k, max_gap, min_span, device):
        cols = np.array(runs, np.int32).reshape(len(runs), 6).T
        return dict(zip(("read", "start", "end", "cls", "windows", "fwd_windows"), cols))
    return engine


def test_kinds_strand_and_fields(tmp_path):
    edge, n = 100, 1000
    read = synth.rand_seq(np.random.default_rng(1), n).lower()
    cag, a = D.class_id("CAG"), D.class_id("A")
    runs = [(0, 0, 1000, cag, 990, 495), (0, edge, 400, cag, 290, 144), (0, edge + 1, n - edge - 1, cag, 788, 788),
            (0, edge + 1, n - edge, a, 789, 0), (0, 100, 900, a, 790, 395)]
    path = tmp_path / "r.fasta"
    path.write_text(f">r0 x\n{read[:500]}\n{read[500:]}\n")
    rows = D.scan_reads(str(path), engine=_fixed_engine(runs))
    assert [r["kind"] for r in rows] == ["in_repeat", "left_open", "spanned", "right_open", "in_repeat"]
    assert [r["strand"] for r in rows] == ["+", "-", "+", "-", "+"]                     # a tie is +
    assert [r["unit"] for r in rows] == [read[s:s + p].upper() for s, p in ((0, 3), (100, 3), (101, 3), (101, 1), (100, 1))]
    assert [r["copies"] for r in rows] == [333, 100, 266, 799, 800]
    assert rows[0]["density"] == 990 / (1000 - 11 + 1) and rows[0]["ref"] == rows[0]["ref_start"] == "-"
    assert D.run_kind(0, 50, 60, 100) == "in_repeat"


def test_both_files_sorting_and_the_catalogue(tmp_path, capsys):
    rng = np.random.default_rng(2)
    flank = lambda m: "T" + synth.rand_seq(rng, m - 2) + "T"                          # no run goes on into a T
    reads = [("s1", flank(300) + cases.pure("AAGGG", 1500) + flank(300)),
             ("i1", synth.revcomp(cases.pure("AAGGG", 900))),
             ("c1", flank(250) + cases.pure("CTG", 240) + flank(250)),
             ("none", flank(800)),
             ("two", cases.pure("AC", 260) + flank(400) + cases.pure("AAGGG", 700, 2)),
             ("c2", flank(150) + cases.pure("CAG", 330) + flank(150))]
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join(f"@{n} c\n{s}\n+\n{'5' * len(s)}\n" for n, s in reads))
    bed = tmp_path / "cat.bed"
    bed.write_text("chr1\t100\t130\tCAG\nchr2\t5\t50\tGCAGCA\nchr2\t500\t550\tAAAAG\nchr3\t1\t9\tACGTACGTA\n")
    prefix = str(tmp_path / "out")
    classes = pipeline.discover_repeats(str(fq), prefix, str(bed), engine=ref_engine)
    err = capsys.readouterr().err
    assert err.count("NOTICE") == 1 and "2 repeat class(es)" in err
    lines = [l.split("\t") for l in open(prefix + ".NanoRepeat_discovered.tsv").read().splitlines()]
    assert tuple(lines[0]) == D.CLASS_COLUMNS
    assert [l[0] for l in lines[1:]] == ["AAGGG", "AGC", "AC"] == [c["Class"] for c in classes]
    aagg = dict(zip(lines[0], lines[1]))
    assert (aagg["Period"], aagg["Reads"], aagg["Runs"], aagg["In_Repeat"], aagg["Right_Open"], aagg["Spanned"]) == \
        ("5", "3", "3", "1", "1", "1")
    assert aagg["Max_Span"] == "1500" and aagg["Max_Copies"] == "300" and aagg["Median_Spanned_Copies"] == "300"
    assert aagg["Total_Bases"] == str(1500 + 900 + 700) and aagg["Catalogued_Regions"] == "0"
    agc = dict(zip(lines[0], lines[2]))
    assert agc["Catalogued_Regions"] == "2" and agc["Spanned"] == "2" and agc["Median_Spanned_Copies"] == "95"
    ac = dict(zip(lines[0], lines[3]))
    assert ac["Left_Open"] == "1" and ac["Median_Spanned_Copies"] == "-" and ac["Catalogued_Regions"] == "0"
    runs = [l.split("\t") for l in open(prefix + ".discovered_runs.tsv").read().splitlines()]
    assert tuple(runs[0]) == D.RUN_COLUMNS
    assert [(l[0], l[7], l[9], l[13]) for l in runs[1:]] == [
        ("s1", "AAGGG", "+", "spanned"), ("i1", "AAGGG", "-", "in_repeat"), ("c1", "AGC", "-", "spanned"),
        ("two", "AC", "+", "left_open"), ("two", "AAGGG", "+", "right_open"), ("c2", "AGC", "+", "spanned")]
    assert runs[1][2:4] == ["-", "-"] and runs[1][4:7] == ["300", "1800", "1500"] and runs[1][8] == "AAGGG"
    assert re.fullmatch(r"[01]\.\d{3}", runs[1][12])
    # without a BED file: "-", and every class is counted; with no_details: the summary only
    other = str(tmp_path / "bare")
    pipeline.discover_repeats(str(fq), other, no_details=True, engine=ref_engine)
    assert "3 repeat class(es)" in capsys.readouterr().err
    assert not os.path.exists(other + ".discovered_runs.tsv")
    assert all(l.split("\t")[-1] == "-" for l in open(other + ".NanoRepeat_discovered.tsv").read().splitlines()[1:])


def test_bam_input_primary_records_and_their_reference(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "pysam", None)
    rng = np.random.default_rng(3)
    seq = synth.rand_seq(rng, 200) + cases.pure("GAA", 400) + synth.rand_seq(rng, 200)
    other = cases.pure("AAAG", 500)
    refs = [("chrA", 100000), ("chrB", 5000)]
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(f"@SQ\tSN:{n}\tLN:{l}\n".encode() for n, l in refs)
    raw = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in refs:
        raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", l)
    for name, s, tid, pos, flag in (("prim", seq, 0, 1234, 0), ("sec", seq, 0, 1300, 0x100), ("sup", seq, 0, 1400, 0x800),
                                    ("rev", synth.revcomp(seq), 1, 77, 0x10), ("unmapped", other, -1, -1, 0x4)):
        raw += K.record(name, s, tid, pos, 50, flag)
    path = str(tmp_path / "t.bam")
    with open(path, "wb") as f:
        f.write(b"".join(K._bgzf_block(raw[u:u + 500]) for u in range(0, len(raw), 500)) + K._bgzf_block(b""))
    rows = D.scan_reads(path, engine=ref_engine, chunk_bases=900)                       # several chunks
    assert [(r["name"], r["ref"], r["ref_start"], r["cls"], r["strand"]) for r in rows] == [
        ("prim", "chrA", 1234, "AAG", "+"), ("rev", "chrB", 77, "AAG", "-"), ("unmapped", "*", "*", "AAAG", "+")]
    from nanorepeat_amd import bam as B
    f = B.BamFile(path)
    assert [r.query_name for r in f.records()] == ["prim", "sec", "sup", "rev", "unmapped"]
    f.close()


def test_the_switch_is_off_by_default():
    assert inspect.signature(pipeline.quantify_from_reads).parameters["discover_repeats"].default is False


# ----------------------------------------------------------------------------------- the error contract
def _call(capi, reads, k=11, max_gap=100, min_span=200, capacity=8, n=None, off=None, data="", arrays=True,
          n_runs=True):
    lib = capi.load()
    packed, offsets = capi.pack_reads(reads)
    out = [np.zeros(max(capacity, 1), np.int32) for _ in range(6)]
    cap = C.c_int64(capacity)
    rc = lib.nra_scan_repeats(0, len(reads) if n is None else n, packed if data == "" else data,
                              capi._ptr(offsets if off is None else off, C.c_int64), k, max_gap, min_span,
                              C.byref(cap) if n_runs else None,
                              *((capi._ptr(a, C.c_int32) if arrays else None) for a in out), None)
    return rc, lib.nra_last_error().decode(errors="replace") if rc else ""


def test_bad_arguments_give_their_code_before_the_device_is_touched(capi):
    ok = ["ACGTACGTACGTACGT"]
    bad = [(dict(k=7), E_ARG, "k must be in 8..15"), (dict(k=16), E_ARG, "k must be in 8..15"),
           (dict(max_gap=0), E_ARG, "max_gap must be in 1..100000"),
           (dict(max_gap=100001), E_ARG, "max_gap must be in 1..100000"),
           (dict(min_span=10), E_ARG, "min_span must be at least k"),
           (dict(n=-1), E_ARG, "negative read count"), (dict(n_runs=False), E_ARG, "n_runs is NULL"),
           (dict(capacity=-1), E_ARG, "negative run capacity"), (dict(arrays=False), E_ARG, "NULL output array"),
           (dict(data=None), E_ARG, "seqs is NULL"),
           (dict(off=np.array([-1, 5], np.int64)), E_ARG, "negative read offset"),
           (dict(off=np.array([6, 0], np.int64)), E_ARG, "read offsets must not decrease")]
    for over, code, text in bad:
        assert _call(capi, ok, **over) == (code, text), over
    assert _call(capi, ["ACG", "A" * 4000001]) == (E_RANGE, "read 1 is longer than 4000000 bases")
    with pytest.raises(capi.NraError) as e:
        capi.scan_repeats(ok, k=16)
    assert e.value.code == E_ARG


def test_good_arguments_without_a_device_fail_loudly(capi):
    """n_reads = 0 too: like the other entry points, the call still looks for its device.  Where there is one, the
    same calls succeed."""
    have = capi.load().nra_device_count() > 0
    for reads in (["ACGCGT", "", "cgN", "A" * 4000000], []):
        rc, text = _call(capi, reads, k=8, min_span=8)
        assert (rc == 0) if have else (rc == E_DEVICE and "no HIP device" in text), (rc, text)


def test_symbol_is_declared_exported_and_additive(capi):
    assert "nra_scan_repeats" in capi.EXPORTS and hasattr(capi.load(), "nra_scan_repeats")
    header = open(os.path.join(ROOT, "include", "nanorepeat_amd.h")).read()
    assert re.search(r"int nra_scan_repeats\(int device, int32_t n_reads, const char\* seqs, const int64_t\* seq_off, "
                     r"int32_t k,\s+int32_t max_gap, int32_t min_span, int64_t\* n_runs, int32_t\* run_read, "
                     r"int32_t\* run_start,\s+int32_t\* run_end, int32_t\* run_class, int32_t\* run_windows, "
                     r"int32_t\* run_fwd_windows,\s+nra_scan_stats_t\* stats\);", header)
    assert capi.load().nra_abi_version() == 4
    assert C.sizeof(capi.ScanStats) == 40
