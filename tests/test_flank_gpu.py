"""Flank haplotypes on the GPU: nra_flank_phase (k_flank_align, k_flank_count, k_split_phase) against tests/flank_ref.py,
every output field bit for bit -- the corner cases of the contract against the full matrix, 150 seeded groups with
ragged coverage over every band class (a third of them with a planted second haplotype), a 20 kb side, forced small
pointer chunks, shuffled groups and rows, the FASTQ command end to end on synth.flank_panel(), and the argument checks
on a device."""

import numpy as np
import pytest

from nanorepeat_amd import synth
import flank_ref as R
from flank_cases import corner_cases, seeded_groups, long_group

pytestmark = pytest.mark.gpu

CLASS_STATS = ("aligned_64", "aligned_128", "aligned_256", "aligned_512", "aligned_1024", "widened")


def _same(got, want, what=""):
    for k in R.RES_FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in R.FIELDS:
        assert len(got[k]) == len(want[k]), (what, k)
        for g, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape and np.array_equal(a, b), (what, k, g, a, b)


def test_corner_cases_equal_the_full_matrix(capi):
    for q, (groups, bbs, kw) in enumerate(corner_cases()):
        _same(capi.flank_phase(groups, bbs, **kw), R.ref_flank_phase(groups, bbs, banded=False, **kw), f"call {q}")


def test_150_seeded_groups_run_every_band_class(capi):
    groups, bbs = seeded_groups(150)
    got = capi.flank_phase(groups, bbs)
    want = R.ref_flank_phase(groups, bbs, banded=True)
    st, ref = got["stats"], want["stats"]
    print(st)
    # what the seed was chosen for, on the restatement alone
    assert all(ref.get(k, 0) > 0 for k in CLASS_STATS)
    assert sum(int((d == -1).sum()) for d in want["dist"]) > 0 and (want["undecided"] > 0).any()
    assert want["phased"].sum() >= 15
    _same(got, want)
    assert {k: st[k] for k in CLASS_STATS} == {k: ref[k] for k in CLASS_STATS}
    assert all(st[f"rows_{w}"] > 0 for w in (64, 128, 256, 512, 1024))
    assert st["sites"] == int(got["n_sites"].sum()) and st["groups_phased"] == int(got["phased"].sum())
    small = [q for q, g in enumerate(groups) if max(len(s) for row in g for s in row) <= 400][:40]
    assert len(small) >= 15
    kw = dict(min_sites=1, skip=5)
    _same(capi.flank_phase([groups[q] for q in small], [bbs[q] for q in small], **kw),
          R.ref_flank_phase([groups[q] for q in small], [bbs[q] for q in small], banded=False, **kw), "full matrix")


def test_20kb_side(capi):
    g, bb = long_group()
    g2, bb2 = seeded_groups(3, seed=5)
    groups, bbs = [g, g2[0]], [bb, bb2[0]]
    got = capi.flank_phase(groups, bbs)
    _same(got, R.ref_flank_phase(groups, bbs, banded=True))
    # three bases are planted in every other row; a site needs all three of them to show its base (min_count 3)
    assert got["phased"][0] == 1 and (got["n0"][0], got["n1"][0]) == (3, 3)
    assert {int(s[0]) for s in got["sites"][0] if s[11]} <= {3000, 11111, 17002}
    assert (got["end"][0][:, 0] > 18000).all() and (got["end"][0][:, 1] == 0).all()


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch):
    groups, bbs = seeded_groups(50, seed=21, max_len=1200)
    monkeypatch.delenv("NRA_TEST_CONS_PTR_BYTES", raising=False)
    one = capi.flank_phase(groups, bbs)
    monkeypatch.setenv("NRA_TEST_CONS_PTR_BYTES", "65536")
    many = capi.flank_phase(groups, bbs)
    _same(many, one)
    assert many["stats"]["launches"] > 4 * one["stats"]["launches"]
    assert many["stats"]["max_pointer_bytes"] < one["stats"]["max_pointer_bytes"]


def test_shuffled_groups_and_rows(capi):
    groups, bbs = seeded_groups(70, seed=22, max_len=800)
    groups, bbs = groups + [[], [("", ""), ("", "")]], bbs + [("CAGCAG", "TTG"), ("CAG", "")]
    one = capi.flank_phase(groups, bbs)
    rng = np.random.default_rng(4)
    order = rng.permutation(len(groups))
    perms = [rng.permutation(len(groups[i])) for i in order]
    two = capi.flank_phase([[groups[i][j] for j in p] for i, p in zip(order, perms)], [bbs[i] for i in order])
    for at, (i, p) in enumerate(zip(order, perms)):
        for k in R.RES_FIELDS:
            assert two[k][at] == one[k][i], (k, i)
        assert np.array_equal(two["sites"][at], one["sites"][i])
        for k in ("label", "dist", "end"):
            assert np.array_equal(two[k][at], one[k][i][p]), (k, i)
        assert np.array_equal(two["site_sym"][at], one["site_sym"][i][:, p])


def test_fastq_command_device_equals_restatement_and_recovers_the_panel(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    from test_flank_cpu import check_planted_panel, check_files
    p = synth.flank_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3, partial_reads=True, flank_phase=True)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "dev"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), flank_engine=R.ref_flank_phase, **common)
    name = "NanoRepeat_flank_phase.tsv"
    assert (tmp_path / f"dev.{name}").read_bytes() == (tmp_path / f"ref.{name}").read_bytes()
    dev, want = _tree(tmp_path / "dev.details"), _tree(tmp_path / "ref.details")
    assert len([k for k in dev if k.endswith(".flank_phase.tsv")]) == 5 and dev == want
    check_planted_panel(p, regions)
    check_files(regions, str(tmp_path / "dev"))


def test_bad_arguments_on_a_device(capi):
    from test_flank_cpu import check_bad_arguments
    check_bad_arguments(capi)
    out = capi.flank_phase([], [])
    assert out["label"] == [] and out["stats"]["launches"] == 0
    row = ("CAGCAGTTGACCATG", "TTGACCAGT")
    out = capi.flank_phase([[row] * 3], [row], max_sites=4096, max_iter=64, min_share_pct=100, skip=0, max_dist=500)
    assert (out["n0"][0], out["phased"][0], out["n_sites"][0]) == (3, 0, 0)
    assert out["dist"][0].tolist() == [[0, 0]] * 3 and out["end"][0].tolist() == [[15, 9]] * 3
