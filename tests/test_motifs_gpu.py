"""Tandem motifs on the GPU: k_tract_motifs (nra_tract_motifs) against the numpy restatement bit for bit -- n_tandem and
the top classes -- over every max_period and top_n, tract kinds, lengths up to 200 kb, forced small chunks and a
config-4-scale call, and the FASTQ command end to end on synth.motif_panel."""

import numpy as np
import pytest

from nanorepeat_amd import motifs, synth
from motif_ref import ref_tract_motifs

pytestmark = pytest.mark.gpu

KINDS = ("pure", "interrupted", "ont", "random", "n", "lower", "mixed")


def _tract(rng, kind, n):
    p = int(rng.integers(1, 7))
    u = synth.rand_unit(rng, p) if p > 1 else "ACGT"[int(rng.integers(0, 4))]
    pure = (u * (n // p + 2))[int(rng.integers(0, p)):][:n]
    if kind == "pure":
        return pure
    if kind == "interrupted":
        s = pure
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + synth.rand_seq(rng, int(rng.integers(1, 8))) + s[at:]
        return s
    if kind == "ont":
        return synth.apply_errors(rng, pure, "ont")
    if kind == "random":
        return synth.rand_seq(rng, n)
    if kind == "n":
        s = list(synth.apply_errors(rng, pure, "hifi"))
        for _ in range(max(1, len(s) // 40)):
            if s:
                s[int(rng.integers(0, len(s)))] = "NRY-"[int(rng.integers(0, 4))]
        return "".join(s)
    if kind == "lower":
        return pure.lower() if rng.random() < 0.5 else pure[:n // 2].lower() + pure[n // 2:]
    v = synth.rand_unit(rng, int(rng.integers(2, 7)))
    return pure[:n // 2] + (v * n)[:n - n // 2]


def _case(seed, count, max_len=700):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = 0 if i % 29 == 0 else int(rng.integers(1, 12)) if i % 7 == 3 else int(rng.integers(1, max_len))
        out.append(_tract(rng, KINDS[i % len(KINDS)], n))
    return out


def _same(got, want):
    for k in ("n_tandem", "top_p", "top_code", "top_count"):
        assert got[k].shape == want[k].shape, k
        bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
        assert len(bad) == 0, f"{k}: {len(bad)} tracts differ, first {bad[:5]}"


def test_kernel_equals_restatement_every_period_and_top_n(capi):
    tracts = _case(1, 397)
    for max_period in range(1, 7):
        want = ref_tract_motifs(tracts, max_period, 8)
        for top_n in range(1, 9):
            got = capi.tract_motifs(tracts, max_period, top_n)
            _same(got, dict(n_tandem=want["n_tandem"], top_p=want["top_p"][:, :top_n],
                            top_code=want["top_code"][:, :top_n], top_count=want["top_count"][:, :top_n]))


def test_long_tracts_and_a_200kb_homopolymer(capi):
    rng = np.random.default_rng(2)
    tracts = ["A" * 200000, _tract(rng, "ont", 200000)[:200000], synth.rand_seq(rng, 199999),
              "AAGGG" * 40000, "CAG" * 5000 + "N" + "CAG" * 5000] + _case(3, 120, max_len=5000)
    got = capi.tract_motifs(tracts)
    _same(got, ref_tract_motifs(tracts))
    assert got["top_count"][0, 0] == 199999 and list(got["n_tandem"][0]) == [199999, 0, 0, 0, 0, 0]
    with pytest.raises(capi.NraError) as e:
        capi.tract_motifs(["CAG", "A" * 200001])
    assert e.value.code == capi.E_RANGE


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch):
    tracts = _case(4, 500, max_len=3000)
    monkeypatch.delenv("NRA_TEST_MOTIF_CHUNK_BYTES", raising=False)
    one = capi.tract_motifs(tracts, 6, 5)
    monkeypatch.setenv("NRA_TEST_MOTIF_CHUNK_BYTES", "4096")
    many = capi.tract_motifs(tracts, 6, 5)
    _same(many, one)
    _same(one, ref_tract_motifs(tracts, 6, 5))


def test_config4_scale_call_matches_on_a_sample(capi):
    d = synth.config4(1000, 1000)
    tracts = [s[100:max(100, len(s) - 100)] for s in d["reads"]]
    got = capi.tract_motifs(tracts)
    rr = d["read_region"]
    rng = np.random.default_rng(9)
    sample = np.sort(np.concatenate([rng.choice(np.nonzero(rr == g)[0], 3, replace=False)
                                     for g in range(len(d["regions"]))]))
    want = ref_tract_motifs([tracts[i] for i in sample])
    _same({k: v[sample] for k, v in got.items()}, want)
    # the regions' motifs come out on top of most of their reads
    hits = [motifs.class_string(int(got["top_p"][i, 0]), int(got["top_code"][i, 0])) ==
            motifs.bed_class(d["regions"][rr[i]][1]) for i in sample]
    assert np.mean(hits) > 0.9


def test_fastq_command_finds_planted_motifs(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    p = synth.motif_panel(model="hifi", seed=5)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), discover_motifs=True, **common)
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_motifs.tsv")} == off
    assert sum(k.endswith(".read_motifs.tsv") for k in on) == 4
    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_motifs.tsv").read_text().split("\n")[1:] if l]
    assert len(rows) == 4
    groups = [{c.split(":")[0]: c.split(":")[1:] for c in row[5].split(",")} for row in rows]
    # through the groups: a read that round 2 or 3 cannot size never reaches phasing
    assert abs(float(groups[0]["AAGGG"][1]) - 200) <= 2 and int(groups[0]["AAGGG"][0]) >= 6
    assert abs(float(groups[1]["CCTG"][1]) - 120) <= 2 and int(groups[1]["CCTG"][0]) >= 6
    assert any("ATTTC" in cell.split(":")[3].split(",") for cell in rows[2][6].split("|")), rows[2]
    control = regions[3]
    assert control.read_motifs and all(rm.differs is False for rm in control.read_motifs.values())
    text = on[[k for k in on if k.endswith(".read_motifs.tsv") and "TATTG" in k][0]].decode()
    assert all(l.split("\t")[5] == "no" for l in text.split("\n")[4:] if l)
