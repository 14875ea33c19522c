"""The anchor screen on the MI355X: nra_screen_reads against the numpy restatement of its contract (same pairs, same
order, same counts), and the FASTQ command end to end against the BAM command and the CPU engines."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nanorepeat_amd import synth
from screen_ref import RefScreen, as_tuples

pytestmark = pytest.mark.gpu

LDS_MAP = 128        # NRA_SCREEN_MAP: (region, side) counters a workgroup keeps in LDS
TILE = 4096          # NRA_SCREEN_TILE


def _anchors(p, anchor_len):
    return [(p["ref"][c][max(0, st - anchor_len):st], p["ref"][c][en:en + anchor_len]) for c, st, en, _ in p["regions"]]


@pytest.fixture(scope="module")
def panel300():
    p = synth.panel(300, anchor_len=1000, reads_per_region=3, edge_overlaps=(150, 300), n_decoys=240, shared=24, seed=7)
    return p, _anchors(p, 1000), [s for _, s in p["reads"]]


def _gpu(anchors, reads, k=15, max_occ=16, min_hits=4):
    from nanorepeat_amd.screen import Screen
    with Screen(anchors, k=k, max_occ=max_occ) as scr:
        return scr.screen_reads(reads, min_hits), scr.stats()


def _same(got, want):
    for key in ("read", "region", "hits_left", "hits_right"):
        assert np.array_equal(got[key], want[key]), key


def test_screen_parity_300_regions(capi, panel300):
    p, anchors, reads = panel300
    assert 2000 <= len(reads) <= 2500
    got, st = _gpu(anchors, reads)
    ref = RefScreen(anchors)
    _same(got, ref.screen_reads(reads))
    assert st["n_masked_max_occ"] > 0 and st["n_keys"] == ref.stats()["n_keys"]
    assert st["n_postings"] == ref.stats()["n_postings"] and st["n_masked_periodic"] == ref.stats()["n_masked_periodic"]
    assert st["bases_screened"] == sum(len(s) for s in reads) and st["kernel_ms"] > 0
    names = [n for n, _ in p["reads"]]
    offered = {(names[r], g) for r, g in zip(got["read"].tolist(), got["region"].tolist())}
    # every truth read with >= 300 bases of each anchor (one with 150 may keep too few intact k-mers)
    assert all((n, g) in offered for n, (g, _) in p["truth"].items() if min(p["overlap"][n]) >= 300)
    assert not any(n.startswith("decoy_") and not n.startswith("decoy_single") for n, _ in offered)


@pytest.mark.parametrize("k", [11, 13])
def test_screen_parity_other_k(capi, panel300, k):
    _, anchors, reads = panel300
    got, _ = _gpu(anchors[:120], reads[:800], k=k, max_occ=8, min_hits=6)
    _same(got, RefScreen(anchors[:120], k=k, max_occ=8).screen_reads(reads[:800], 6))


def test_one_long_read_over_many_tiles_and_full_lds_maps(capi, panel300):
    """A 1.5 Mb read of 20-base pieces of 300 regions' anchors: 367 tiles, each hitting more (region, side) sets
    than a workgroup's LDS map holds, so hits overflow to global entries (and the entry list grows)."""
    _, anchors, _ = panel300
    rng = np.random.default_rng(9)
    flat = [a for pair in anchors for a in pair]
    pieces = []
    for _ in range(1_500_000 // 20):
        a = flat[int(rng.integers(0, len(flat)))]
        o = int(rng.integers(0, len(a) - 20))
        pieces.append(a[o:o + 20])
    long_read = "".join(pieces)
    reads = ["ACGT" * 3, long_read, synth.rand_seq(rng, 5000)]
    ref = RefScreen(anchors)
    read, sets, _ = ref.hits([long_read[:TILE + 14]])
    assert len(set(sets.tolist())) > LDS_MAP                      # the first tile overflows its map
    got, _ = _gpu(anchors, reads)
    _same(got, ref.screen_reads(reads))
    assert (got["read"] == 1).sum() > 200


def test_two_calls_on_one_handle_and_capacity(capi, panel300):
    from nanorepeat_amd.screen import Screen
    _, anchors, reads = panel300
    ref = RefScreen(anchors)
    with Screen(anchors) as scr:
        a = scr.screen_reads(reads[:700])
        b = scr.screen_reads(reads[700:1500])
        _same(a, ref.screen_reads(reads[:700]))
        _same(b, ref.screen_reads(reads[700:1500]))
        st = scr.stats()
        assert st["n_calls"] == 2 and st["sum_kernel_ms"] >= st["kernel_ms"] > 0
        want = ref.screen_reads(reads[:700])
        n_want = len(want["read"])
        assert n_want > 10
        lib = capi.load()
        seqs, off = capi.pack_reads(reads[:700])
        out = [np.full(n_want, -7, np.int32) for _ in range(4)]
        n = C.c_int64(n_want - 1)
        rc = lib.nra_screen_reads(scr._h, 700, seqs, capi._ptr(off, C.c_int64), 4, C.byref(n),
                                  *(capi._ptr(x, C.c_int32) for x in out))
        assert rc == capi.E_RANGE and n.value == n_want
        assert all((x == -7).all() for x in out)                   # nothing written
        n = C.c_int64(n_want)
        assert lib.nra_screen_reads(scr._h, 700, seqs, capi._ptr(off, C.c_int64), 4, C.byref(n),
                                    *(capi._ptr(x, C.c_int32) for x in out)) == 0
        assert n.value == n_want
        for x, key in zip(out, ("read", "region", "hits_left", "hits_right")):
            assert np.array_equal(x, want[key]), key
        got = capi.screen_reads(scr._h, reads[:700], capacity=3)   # the binding's retry
        _same(got, want)


def test_bad_arguments_on_a_device(capi):
    from nanorepeat_amd.screen import Screen
    with pytest.raises(capi.NraError) as e:
        capi.screen_create([("ACGT" * 10, "TTGA" * 10)], k=12)
    assert e.value.code == -1
    with Screen([("ACGTTGCAAGTCCATGACTTGA", "TTGACCATGACCAGTACAGGAT")]) as scr:
        with pytest.raises(capi.NraError) as e:
            scr.screen_reads(["ACGT"], min_hits=0)
        assert e.value.code == -1
        got = scr.screen_reads(["", "ACG"])
        assert len(got["read"]) == 0


# ---------------------------------------------------------------------------- end to end
def test_fastq_command_gpu_equals_bam_command_gpu_and_oracle(capi, oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    from test_screen_cpu import _bam_reads, _decoys, _write_fastq, _tree
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    mixed = _bam_reads(tmp_path)
    for j, d in enumerate(_decoys(tmp_path, np.random.default_rng(11))):
        mixed.insert((7 * j) % (len(mixed) + 1), d)
    _write_fastq(tmp_path / "in.fastq", mixed)
    ref, bed, fq = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"), str(tmp_path / "in.fastq")
    common = dict(data_type="ont_q20", anchor_len=400, seed=1)
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), ref, bed, str(tmp_path / "bam"), **common)
    pipeline.quantify_from_reads(fq, ref, bed, str(tmp_path / "fq"), **common)
    pipeline.quantify_from_reads(fq, ref, bed, str(tmp_path / "cpu"), aligner=oracle.align_pairs,
                                 scorer=oracle.round3_1d, screener=RefScreen, **common)
    tsv = (tmp_path / "fq.NanoRepeat_output.tsv").read_bytes()
    assert tsv == (tmp_path / "bam.NanoRepeat_output.tsv").read_bytes()
    assert tsv == (tmp_path / "cpu.NanoRepeat_output.tsv").read_bytes()
    got = _tree(tmp_path / "fq.details")
    assert got == _tree(tmp_path / "bam.details") and got == _tree(tmp_path / "cpu.details")
    assert any(n.endswith(".allele2.fastq") for n in got)


def test_screened_equals_exhaustive_on_a_panel(capi, tmp_path):
    from nanorepeat_amd import pipeline
    p = synth.panel(12, anchor_len=1000, reads_per_region=8, edge_overlaps=(150, 300, 600, 1000), n_decoys=36,
                    shared=0, seed=21)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont", anchor_len=1000, seed=3)
    a = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "s"), **common)
    b = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "x"), screen=False, **common)
    n_found = 0
    for ra, rb in zip(a, b):
        assert sorted(ra.read_dict) == sorted(rb.read_dict), ra.to_unique_id()
        assert {n: r.round3_repeat_size for n, r in ra.read_dict.items()} == \
               {n: r.round3_repeat_size for n, r in rb.read_dict.items()}
        n_found += len(ra.read_dict)
    assert n_found >= 12 * 8
    assert (tmp_path / "s.NanoRepeat_output.tsv").read_text() == (tmp_path / "x.NanoRepeat_output.tsv").read_text()


def test_scale_1000_regions(capi):
    p = synth.panel(1000, anchor_len=1000, reads_per_region=46, edge_overlaps=(150, 300), n_decoys=1000, shared=40,
                    seed=33)
    anchors = _anchors(p, 1000)
    names = [n for n, _ in p["reads"]]
    seqs = [s for _, s in p["reads"]]
    assert len(seqs) >= 50000
    got, st = _gpu(anchors, seqs)
    sample = np.sort(np.random.default_rng(5).choice(len(seqs), 2000, replace=False))
    want = RefScreen(anchors).screen_reads([seqs[i] for i in sample])
    keep = np.isin(got["read"], sample)
    sub = {key: v[keep] for key, v in got.items()}
    sub["read"] = np.searchsorted(sample, sub["read"]).astype(np.int32)
    _same(sub, want)
    offered = {(names[r], g) for r, g in zip(got["read"].tolist(), got["region"].tolist())}
    for n, (g, _) in p["truth"].items():
        if min(p["overlap"][n]) >= 300:
            assert (n, g) in offered, n
