"""FASTQ / FASTA input through the anchor screen, without a GPU: the screen's numpy restatement against a plain
one, `io.iter_reads`, the FASTQ command against the BAM command with the CPU oracle engines, and the argument
checks of the nra_screen_* entry points."""
import gzip
import os
import sys

import numpy as np
import pytest

from nanorepeat_amd import io as nr_io, synth
from screen_ref import RefScreen, plain_screen, as_tuples
from test_bam import _bam_case
from nanorepeat_amd import bam as B

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------- the restatements agree
def _small_case(seed, k):
    rng = np.random.default_rng(seed)
    n = 6
    anchors = []
    shared = synth.rand_seq(rng, 40)
    for g in range(n):
        left, right = synth.rand_seq(rng, int(rng.integers(0, 120))), synth.rand_seq(rng, int(rng.integers(20, 120)))
        if g % 3 == 0:
            left = left[:10] + shared + left[10:]            # in 2 or 3 sets: masked at max_occ 1 and 2
        if g == 1:
            left = "CAG" * 12 + left[:30].lower()            # periodic k-mers, lowercase
        if g == 2:
            right = "ATATATATATATATATAT"                     # periodic only: an empty right set
        if g == 4:
            left, right = "ACGTNACGTRACGTNAC", "AC"          # no valid window on either side: an empty region
        if g == 5:
            right = right[:30] + "N" + right[30:] + "y" + "ACGT"
        anchors.append((left, right))
    reads = []
    for i in range(30):
        g = int(rng.integers(0, n))
        left, right = anchors[g]
        s = left[int(rng.integers(0, max(1, len(left)))):] + synth.rand_seq(rng, 20) + right[:int(rng.integers(0, len(right) + 1))]
        if i % 5 == 0:
            s = synth.revcomp(s)
        if i % 7 == 0:
            s = s.lower()
        if i % 6 == 0:
            s = s[:15] + "NRYK"[i % 4] + s[15:]
        if i % 11 == 0:
            s = s[:k - 1]                                    # shorter than k
        reads.append(s)
    reads += [shared * 2, "", "ACG", synth.rand_seq(rng, 200)]
    return anchors, reads


@pytest.mark.parametrize("k", [11, 13, 15])
@pytest.mark.parametrize("max_occ", [1, 2, 16])
def test_numpy_restatement_equals_plain_restatement(k, max_occ):
    for seed in range(3):
        anchors, reads = _small_case(seed * 10 + k, k)
        for min_hits in (1, 4):
            want = plain_screen(anchors, reads, k, max_occ, min_hits)
            with RefScreen(anchors, k=k, max_occ=max_occ) as scr:
                got = as_tuples(scr.screen_reads(reads, min_hits))
                assert scr.stats()["n_empty_regions"] >= 1
            assert got == want, (seed, min_hits)
            assert any(r[2] == 0 and r[3] == 0 for r in got)  # the empty region takes reads


def test_panel_reads_pass_their_regions():
    p = synth.panel(6, anchor_len=400, reads_per_region=4, edge_overlaps=(300,), n_decoys=12, seed=3)
    regions = [(p["ref"][c][max(0, st - 400):st], p["ref"][c][en:en + 400]) for c, st, en, _ in p["regions"]]
    names = [n for n, _ in p["reads"]]
    got = RefScreen(regions).screen_reads([s for _, s in p["reads"]])
    offered = {(names[r], g) for r, g in zip(got["read"], got["region"])}
    for name, (g, _) in p["truth"].items():
        assert (name, g) in offered, name
    assert not any(n.startswith("decoy") for n, _ in offered)


# ---------------------------------------------------------------------------- io.iter_reads
def test_iter_reads_formats_and_chunks(tmp_path):
    recs = [("r1", "ACGTACGTAC", "IIIIIIIIII"), ("r2", "", ""), ("r3", "acgtnN", "!!!!!!"), ("r4", "A" * 95, "5" * 95)]
    fq = tmp_path / "a.fastq"
    fq.write_text("".join(f"@{n} extra words\n{s}\n+\n{q}\n" for n, s, q in recs))
    fa = tmp_path / "a.fa"
    fa.write_text("\n" + "".join(f">{n} desc\n" + "".join(s[i:i + 7] + "\n" for i in range(0, len(s), 7)) for n, s, _ in recs))
    gz = tmp_path / "a.fastq.gz"
    with gzip.open(gz, "wt") as f:
        f.write(fq.read_text())
    for path, with_q in ((fq, True), (fa, False), (gz, True)):
        chunks = list(nr_io.iter_reads(str(path), 1 << 20))
        assert len(chunks) == 1
        names, seqs, quals = chunks[0]
        assert names == [r[0] for r in recs] and seqs == [r[1] for r in recs]
        assert quals == ([r[2] for r in recs] if with_q else [None] * 4)
        small = list(nr_io.iter_reads(str(path), 10))
        assert [len(c[0]) for c in small] == [1, 3]         # a chunk ends at the record that reaches 10 bases
        assert sum((c[1] for c in small), []) == seqs
    (tmp_path / "bad.txt").write_text("hello\n")
    with pytest.raises(ValueError):
        list(nr_io.iter_reads(str(tmp_path / "bad.txt")))
    (tmp_path / "empty.fq").write_text("")
    assert list(nr_io.iter_reads(str(tmp_path / "empty.fq"))) == []


# ---------------------------------------------------------------------------- FASTQ command == BAM command
def _decoys(tmp_path, rng, n=50):
    """Reads the screen must not offer: random sequence, N runs, slices of the reference away from the BED
    windows (lowercase too), one anchor only, reads shorter than k."""
    chrom = "".join(l.strip() for l in (tmp_path / "ref.fa").read_text().split("\n")[1:])
    rows = [l.split("\t") for l in (tmp_path / "r.bed").read_text().split("\n") if l]
    s1, e1, s2 = int(rows[0][1]), int(rows[0][2]), int(rows[1][1])
    out = []
    for i in range(n):
        kind = i % 6
        if kind == 0:
            s = synth.rand_seq(rng, 800)
        elif kind == 1:
            s = synth.rand_seq(rng, 300) + "N" * 40 + synth.rand_seq(rng, 300)
        elif kind in (2, 3):
            lo = e1 + 500 + int(rng.integers(0, 100))         # between the two regions' windows (400 bases)
            s = chrom[lo:lo + 300]
            s = s.lower() if kind == 3 else s
        elif kind == 4:
            s = chrom[s1 - 400:s1] + synth.rand_seq(rng, 200)   # the left anchor only
        else:
            s = synth.rand_seq(rng, 9)
        out.append((f"decoy{i:02d}", s, [20] * len(s)))
    assert s2 - 400 > e1 + 500 + 100 + 300
    return out


def _bam_reads(tmp_path):
    bam = B.BamFile(str(tmp_path / "in.bam"))
    recs = [(r.query_name, r.query_sequence, r.query_qualities) for r in bam.fetch("chr7", 0, 1 << 30)]
    bam.close()
    return recs


def _write_fastq(path, recs):
    with open(path, "w") as f:
        for name, seq, quals in recs:
            f.write(f"@{name}\n{seq}\n+\n{''.join(chr(q + 33) for q in quals)}\n")


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_fastq_command_equals_bam_command_with_oracle(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    recs = _bam_reads(tmp_path)
    rng = np.random.default_rng(11)
    mixed = list(recs)
    for j, d in enumerate(_decoys(tmp_path, rng)):
        mixed.insert((7 * j) % (len(mixed) + 1), d)
    _write_fastq(tmp_path / "in.fastq", mixed)
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    pipeline.quantify_from_bam(str(tmp_path / "in.bam"), ref, bed, str(tmp_path / "bam"), **common)
    regions = pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / "fq"),
                                           screener=RefScreen, **common)
    assert (tmp_path / "bam.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "fq.NanoRepeat_output.tsv").read_bytes()
    want, got = _tree(tmp_path / "bam.details"), _tree(tmp_path / "fq.details")
    assert sorted(want) == sorted(got)
    for name in want:
        assert want[name] == got[name], name
    assert any(n.endswith(".allele1.fastq") for n in got) and any(n.endswith(".repeat_size.txt") for n in got)
    assert len(regions[0].read_dict) == 20 and len(regions[1].read_dict) == 20


def _sizes(regions):
    return [{n: r.round3_repeat_size for n, r in region.read_dict.items()} for region in regions]


def test_fasta_and_gzip_inputs_give_the_same_sizes(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    recs = _bam_reads(tmp_path) + _decoys(tmp_path, np.random.default_rng(2), 12)
    _write_fastq(tmp_path / "in.fastq", recs)
    with gzip.open(tmp_path / "in.fastq.gz", "wt") as f:
        f.write((tmp_path / "in.fastq").read_text())
    (tmp_path / "in.fa").write_text("".join(f">{n} x\n" + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60))
                                            for n, s, _ in recs))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    base = _sizes(pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / "a"), **common))
    assert base[0] and base[1]
    for src, out in (("in.fastq.gz", "b"), ("in.fa", "c")):
        regions = pipeline.quantify_from_reads(str(tmp_path / src), ref, bed, str(tmp_path / out), **common)
        assert _sizes(regions) == base, src
    fa_reads = (tmp_path / "c.details" / "chr7").glob("*.reads.fastq")
    texts = [p.read_text() for p in fa_reads]
    assert any(texts)
    for text in texts:
        lines = text.split("\n")
        for i in range(0, len(lines) - 1, 4):
            assert set(lines[i + 3]) <= {"."} and len(lines[i + 3]) == len(lines[i + 1])


def test_small_chunks_give_the_same_result(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    recs = _bam_reads(tmp_path) + _decoys(tmp_path, np.random.default_rng(4), 12)
    _write_fastq(tmp_path / "in.fastq", recs)
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen)
    ref, bed = str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / "one"), **common)
    pipeline.quantify_from_reads(str(tmp_path / "in.fastq"), ref, bed, str(tmp_path / "many"), chunk_bases=3000, **common)
    assert (tmp_path / "one.NanoRepeat_output.tsv").read_text() == (tmp_path / "many.NanoRepeat_output.tsv").read_text()
    assert _tree(tmp_path / "one.details") == _tree(tmp_path / "many.details")


def test_region_whose_reference_fails_to_extract_fails_the_command(tmp_path):
    from nanorepeat_amd import pipeline
    (tmp_path / "ref.fa").write_text(">chr1\n" + "ACGT" * 50 + "\n")
    (tmp_path / "r.bed").write_text("chr1\t10\t900\tCAG\n")
    (tmp_path / "in.fq").write_text("@a\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError):
        pipeline.quantify_from_reads(str(tmp_path / "in.fq"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"),
                                     str(tmp_path / "o"), screener=RefScreen)


# ---------------------------------------------------------------------------- C ABI checks
def test_screen_entry_points_check_arguments_and_need_a_device(capi):
    """Arguments are checked before the device is touched (NRA_E_ARG); with good arguments and no device the
    create call returns NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers those paths."""
    import ctypes as C
    lib = capi.load()
    if lib.nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    anchors = [("ACGTACGTTGCATGCAAGT", "TTGACCATGACCAGTACAG")]
    for kw in (dict(k=14), dict(k=9), dict(k=17), dict(max_occ=0), dict(max_occ=256)):
        with pytest.raises(capi.NraError) as e:
            capi.screen_create(anchors, **kw)
        assert e.value.code == -1, kw
    data, off = capi.pack_reads(["ACGT", "ACGT"])
    h = C.c_void_p()
    assert lib.nra_screen_create(0, 1, data, None, 15, 16, C.byref(h)) == -1
    assert lib.nra_screen_create(0, 0, data, capi._ptr(off, C.c_int64), 15, 16, C.byref(h)) == -1
    assert lib.nra_screen_create(0, 1, data, capi._ptr(off, C.c_int64), 15, 16, None) == -1
    bad = np.array([0, 4, 2], np.int64)
    assert lib.nra_screen_create(0, 1, data, capi._ptr(bad, C.c_int64), 15, 16, C.byref(h)) == -1
    with pytest.raises(capi.NraError) as e:
        capi.screen_create(anchors)
    assert e.value.code == -2 and "no HIP device" in str(e.value)
    n = C.c_int64(0)
    assert lib.nra_screen_reads(None, 1, data, capi._ptr(off, C.c_int64), 4, C.byref(n), None, None, None, None) == -1
    st = capi.ScreenStats()
    assert lib.nra_screen_stats(None, C.byref(st)) == -1
    assert lib.nra_screen_destroy(None) == 0
