"""Repeat structure without a GPU: the plain restatement against a brute force, path replay, the numpy form against the
plain one, hand cases of the unit derivation, both commands with read_structure=True (restatement as engine, oracle as
scorer), and the argument checks of nra_read_structure."""
import ctypes as C
import sys

import numpy as np
import pytest

from nanorepeat_amd import structure, synth
from structure_ref import plain_align, plain_units, ref_read_structure, MATCH, MISMATCH, INSERTION


def _levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[-1]


def _brute(s, u):
    """min over phase phi and length L of the plain edit distance between s and (u u u ...)[phi:phi + L]."""
    s = s.upper()
    p = len(u)
    inf = (u * (len(s) // p + 3))
    return min(_levenshtein(s, inf[phi:phi + L]) for phi in range(p) for L in range(0, 2 * len(s) + p + 1)
               if phi + L <= len(inf))


def _small_cases(seed, count=40):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        p = int(rng.integers(1, 6))
        u = synth.rand_unit(rng, p) if p > 1 else "ACGT"[i % 4]
        n_units = int(rng.integers(0, 5))
        base = (u * (n_units + 2))[int(rng.integers(0, p)):][:n_units * p + int(rng.integers(0, p))]
        kind = i % 4
        s = base if kind == 0 else synth.apply_errors(rng, base, (0.2, 0.15, 0.15)) if kind == 1 else \
            synth.rand_seq(rng, int(rng.integers(0, 9))) if kind == 2 else base.lower() + "N"
        out.append((s, u))
    return out


def _replay(s, u, start, path):
    """-> (read bases spelled, motif string consumed, cost)."""
    p = len(u)
    c, read, motif, cost = start, "", "", 0
    for i, b in enumerate(path):
        op, nd = b & 3, b >> 2
        read += s[i]
        if op == INSERTION:
            cost += 1
        else:
            motif += u[c % p]
            cost += op == MISMATCH
            assert (op == MATCH) == (s[i].upper() == u[c % p])
            c += 1
        for _ in range(nd):
            motif += u[c % p]
            c += 1
            cost += 1
        assert nd < p
    return read, motif, cost


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plain_edits_equal_brute_force_and_paths_replay(seed):
    for s, u in _small_cases(seed):
        edits, start, path = plain_align(s, u)
        assert edits == _brute(s, u), (s, u)
        assert len(path) == len(s) and 0 <= start < len(u)
        read, motif, cost = _replay(s, u, start, path)
        assert read == s and cost == edits
        assert motif == (u * (len(motif) // len(u) + 2))[start:start + len(motif)]


def test_numpy_form_equals_plain_form():
    rng = np.random.default_rng(4)
    motifs, tracts, rm = [], [], []
    for p in (1, 2, 3, 5, 7, 16, 33, 64):
        motifs.append(synth.rand_unit(rng, p) if p > 1 else "T")
        for i in range(12):
            base = (motifs[-1] * 60)[int(rng.integers(0, p)):][:int(rng.integers(0, 300))]
            t = synth.apply_errors(rng, base, "ont") if i % 3 else base
            tracts.append(t.lower() if i % 5 == 4 else t[:10] + "N" + t[10:] if i % 5 == 3 else t)
            rm.append(len(motifs) - 1)
    a = ref_read_structure(motifs, tracts, rm)
    b = ref_read_structure(motifs, tracts, rm, vectorised=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _units(s, u):
    e, st, path = plain_align(s, u)
    got = structure.derive_units(s.upper(), len(u), st, path)
    want = plain_units(s.upper(), u, st, path)
    if want is None:
        assert got is None
        return e, None
    assert got == (want["purity"], want["pure_units"], want["longest_pure_run"], want["interruptions"])
    return e, want


def test_hand_cases():
    e, w = _units("CAG" * 10 + "CAA" + "CAG" * 5, "CAG")
    assert e == 1 and w["pure_units"] == 15 and w["longest_pure_run"] == 10 and w["interruptions"] == [(10, "CAA")]
    e, w = _units("CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * 10, "CGG")
    assert e == 2 and w["interruptions"] == [(9, "AGG"), (19, "AGG")] and w["pure_units"] == 28
    e, w = _units("TATTG" * 7, "TATTG")
    assert e == 0 and w["interruptions"] == [] and w["purity"] == 1.0 and w["longest_pure_run"] == 7
    rs = structure.ReadStructure(35, 0, 1.0, 7, 7, [])
    assert rs.fields()[-1] == "-"
    # an insertion at a unit boundary belongs to the slot the counter points at: the next one
    e, st, path = plain_align("CAG" * 4 + "T" + "CAG" * 4, "CAG")
    assert e == 1 and st == 0 and path[12] == INSERTION
    assert structure.derive_units("CAG" * 4 + "T" + "CAG" * 4, 3, st, path)[3] == [(4, "TCAG")]
    # a deleted base: the slot keeps its p positions and is not pure
    e, st, path = plain_align("CAG" * 4 + "CG" + "CAG" * 4, "CAG")
    assert e == 1 and structure.derive_units("CAG" * 4 + "CG" + "CAG" * 4, 3, st, path)[3] == [(4, "CG")]
    # a tract that starts mid-unit: slot 0 is partial
    e, st, path = plain_align("AG" + "CAG" * 5, "CAG")
    assert e == 0 and st == 1
    assert structure.derive_units("AG" + "CAG" * 5, 3, st, path)[1:3] == (5, 5)
    # empty tract, p = 1
    assert plain_align("", "CAG") == (0, 0, b"")
    assert structure.derive_units("", 3, 0, b"") is None
    e, w = _units("AAAAACAAAA", "A")
    assert e == 1 and w["interruptions"] == [(5, "C")] and w["pure_units"] == 9 and w["longest_pure_run"] == 5
    assert structure.ReadStructure(0).fields() == ["0", "-", "-", "-", "-", "-"]


# ---------------------------------------------------------------------------- the commands
def _run_both(tmp_path, command, oracle, extra):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  **extra)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    src = str(tmp_path / ("in.bam" if command is pipeline.quantify_from_bam else "in.fastq"))
    command(src, ref, bed, str(tmp_path / "off"), **common)
    regions = command(src, ref, bed, str(tmp_path / "on"), read_structure=True, structure_engine=ref_read_structure,
                      **common)
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_structure.tsv")} == off
    return regions, on, (tmp_path / "on.NanoRepeat_structure.tsv").read_text()


def _check_outputs(regions, tree, summary):
    files = sorted(k for k in tree if k.endswith(".read_structure.tsv"))
    assert len(files) == 2                                       # the third region has no reads
    for region in regions[:2]:
        text = tree[[k for k in files if region.repeat_unit_seq in k][0]].decode()
        lines = text.split("\n")
        assert lines[0] == f"##RepeatRegion={region.to_unique_id()}" and lines[1] == f"##Motif={region.repeat_unit_seq}"
        assert lines[2].startswith("#Read_Name\tAllele_ID\tRepeat_Size\tTract_Len\tEdits\tPurity")
        rows = [l.split("\t") for l in lines[3:] if l]
        sized = [n for n, r in region.read_dict.items() if r.round3_repeat_size is not None]
        assert sorted(r[0] for r in rows) == sorted(sized)
        phased = open(region.out_prefix + ".phased_reads.txt").read().split("\n")[2:]
        phased = [l.split("\t") for l in phased if l]
        assert [(r[0], r[1]) for r in rows[:len(phased)]] == [(r[0], r[1]) for r in phased]
        assert [r[2] for r in rows[:len(phased)]] == [r[3] for r in phased]          # Repeat_Size, %.1f
        for r in rows:
            assert len(r) == 9
            if r[3] != "0":
                assert 0.0 <= float(r[5]) <= 1.0 and int(r[4]) >= 0
    srows = [l.split("\t") for l in summary.split("\n")[1:] if l]
    assert summary.startswith("#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Structure\n")
    assert len(srows) == 3 and srows[2][4:] == ["0", "-"]
    for row in srows[:2]:
        assert row[4] == "2"
        for cell in row[5].split("|"):
            label, n, purity, pure, longest, rec = cell.split(":")
            assert int(n) >= 5 and 0.5 < float(purity) <= 1.0


def test_bam_command_writes_structure_files(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    _check_outputs(*_run_both(tmp_path, pipeline.quantify_from_bam, oracle, {}))


def test_fastq_command_writes_structure_files(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    from test_screen_cpu import _bam_reads, _write_fastq
    from screen_ref import RefScreen
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    _write_fastq(tmp_path / "in.fastq", _bam_reads(tmp_path))
    _check_outputs(*_run_both(tmp_path, pipeline.quantify_from_reads, oracle, dict(screener=RefScreen)))


def test_no_details_writes_only_the_summary(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"),
                               str(tmp_path / "o"), data_type="ont_q20", anchor_len=400, seed=1, no_details=True,
                               aligner=oracle.align_pairs, scorer=oracle.round3_1d, read_structure=True,
                               structure_engine=ref_read_structure)
    assert not (tmp_path / "o.details").exists()
    assert len((tmp_path / "o.NanoRepeat_structure.tsv").read_text().split("\n")) == 5


def test_unsupported_motif_gets_dash_fields():
    class Read:
        round3_repeat_size, left_buffer_len, right_buffer_len = 12.0, 2, 2

    class Region:
        repeat_unit_seq = "CAGN"
        read_dict = {"a": Read()}
        read_core_seq_dict = {"a": "TTCAGCAGTT"}

    calls = []
    structure.structure_regions([Region], engine=lambda *a, **k: calls.append(a))
    assert not calls and Region.read_structure["a"].fields() == ["6", "-", "-", "-", "-", "-"]


# ---------------------------------------------------------------------------- C ABI checks
def test_read_structure_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    lib = capi.load()
    if lib.nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for motif, code in (("", -1), ("A" * 65, -3), ("CAN", -1), ("cag", -1)):
        with pytest.raises(capi.NraError) as e:
            capi.read_structure([motif], ["CAGCAG"], [0])
        assert e.value.code == code, motif
    with pytest.raises(capi.NraError) as e:
        capi.read_structure(["CAG"], ["CAG"], [1])
    assert e.value.code == -1
    with pytest.raises(capi.NraError) as e:
        capi.read_structure(["CAG"], ["A" * 200001], [0])
    assert e.value.code == -3
    data, off = capi.pack_reads(["CAG"])
    assert lib.nra_read_structure(0, 0, data, capi._ptr(off, C.c_int64), 0, None, None, None, None, None, None) == -1
    assert lib.nra_read_structure(0, 1, data, None, 0, None, None, None, None, None, None) == -1
    with pytest.raises(capi.NraError) as e:
        capi.read_structure(["CAG", "A" * 64], ["CAGCAG", ""], [0, 1])
    assert e.value.code == -2 and "no HIP device" in str(e.value)
