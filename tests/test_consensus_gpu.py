"""Allele consensus on the GPU: nra_tract_consensus (k_cons_align, k_cons_build) against tests/consensus_ref.py, every
output field bit for bit -- the corner cases of the contract against the full matrix, 200 seeded alleles, 20 kb tracts,
forced small pointer chunks, shuffled groups, config 2 and config 4 at full size against the banded restatement, and
the FASTQ command end to end."""

import numpy as np
import pytest

from nanorepeat_amd import synth
import consensus_ref as R
from consensus_cases import edge_groups, seeded_alleles, long_allele

pytestmark = pytest.mark.gpu

FLANK = 100


def _same(got, want, what=""):
    assert got["consensus"] == want["consensus"], what
    for g, (a, b) in enumerate(zip(got["support"], want["support"])):
        assert np.array_equal(a, b), (what, g)
    for k in ("n_rounds", "converged", "voted", "left_out"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def test_corner_cases_equal_the_full_matrix(capi):
    for q, (groups, max_dist) in enumerate(edge_groups()):
        got = capi.tract_consensus(groups, max_dist=max_dist)
        _same(got, R.ref_tract_consensus(groups, max_dist=max_dist, banded=False), f"call {q}")
    groups, _ = edge_groups()[-1]
    got = capi.tract_consensus(groups, max_rounds=1)
    _same(got, R.ref_tract_consensus(groups, max_rounds=1, banded=False), "one round")
    assert (got["n_rounds"] == 1).all()


def test_200_seeded_alleles_run_every_band_class(capi):
    groups = seeded_alleles(200)
    got = capi.tract_consensus(groups)
    _same(got, R.ref_tract_consensus(groups, banded=True))
    st = got["stats"]
    for width in (64, 128, 256, 512, 1024):
        assert st[f"aligned_{width}"] > 0 and st[f"rows_{width}"] > 0, st
    assert st["widened"] > 0, st
    # the full matrix on the alleles small enough for it
    small = [g for g in groups if max(len(t) for t in g) <= 400][:40]
    assert len(small) >= 20
    _same(capi.tract_consensus(small), R.ref_tract_consensus(small, banded=False), "full matrix")


def test_20kb_tracts(capi):
    groups = [long_allele(), seeded_alleles(3, seed=5)[1]]
    got = capi.tract_consensus(groups)
    _same(got, R.ref_tract_consensus(groups, banded=True))
    assert len(got["consensus"][0]) > 19000 and got["voted"][0] == len(groups[0])
    with pytest.raises(capi.NraError) as e:
        capi.tract_consensus([["A" * 200001]])
    assert e.value.code == capi.E_RANGE


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch):
    groups = seeded_alleles(60, seed=21, max_len=1500)
    monkeypatch.delenv("NRA_TEST_CONS_PTR_BYTES", raising=False)
    one = capi.tract_consensus(groups)
    monkeypatch.setenv("NRA_TEST_CONS_PTR_BYTES", "65536")
    many = capi.tract_consensus(groups)
    _same(many, one)
    assert many["stats"]["launches"] > 4 * one["stats"]["launches"]
    assert many["stats"]["max_pointer_bytes"] < one["stats"]["max_pointer_bytes"]


def test_shuffled_groups_give_each_group_the_same_result(capi):
    groups = seeded_alleles(80, seed=22, max_len=1200) + [[], ["", ""]]
    one = capi.tract_consensus(groups)
    order = np.random.default_rng(4).permutation(len(groups))
    two = capi.tract_consensus([groups[i] for i in order])
    back = dict(consensus=[None] * len(groups), support=[None] * len(groups),
                **{k: np.zeros(len(groups), np.int32) for k in ("n_rounds", "converged", "voted", "left_out")})
    for at, i in enumerate(order):
        back["consensus"][i], back["support"][i] = two["consensus"][at], two["support"][at]
        for k in ("n_rounds", "converged", "voted", "left_out"):
            back[k][i] = two[k][at]
    _same(back, one)


def test_config2_full_size_two_alleles(capi):
    d = synth.config2()
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    groups = [[t for t, k in zip(tracts, d["k_true"]) if k == a] for a in (40, 150)]      # one per true allele
    assert min(len(g) for g in groups) > 4000
    got = capi.tract_consensus(groups)
    _same(got, R.ref_tract_consensus(groups, banded=True))
    assert got["consensus"][0].count("TATTG") >= 38 and got["consensus"][1].count("TATTG") >= 140


def test_config4_every_tenth_region(capi):
    d = synth.config4()
    rr, kt = np.asarray(d["read_region"]), np.asarray(d["k_true"])
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    groups, region_of = [], []
    for g in range(len(d["regions"])):                          # one group per true allele of every region
        mine = np.nonzero(rr == g)[0]
        for a in sorted(set(kt[mine].tolist())):
            groups.append([tracts[i] for i in mine[kt[mine] == a]])
            region_of.append(g)
    got = capi.tract_consensus(groups)
    pick = [q for q in range(len(groups)) if region_of[q] % 10 == 0]
    want = R.ref_tract_consensus([groups[q] for q in pick], banded=True)
    sub = dict(consensus=[got["consensus"][q] for q in pick], support=[got["support"][q] for q in pick],
               **{k: got[k][pick] for k in ("n_rounds", "converged", "voted", "left_out")})
    _same(sub, want)


def test_fastq_command_device_equals_restatement_files(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    p = synth.panel(12, anchor_len=1000, reads_per_region=8, edge_overlaps=(150, 300), n_decoys=36, shared=0, seed=21)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont", anchor_len=1000, seed=3, allele_consensus=True)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "dev"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), consensus_engine=R.ref_tract_consensus, **common)
    assert (tmp_path / "dev.NanoRepeat_consensus.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_consensus.tsv").read_bytes()
    dev, want = _tree(tmp_path / "dev.details"), _tree(tmp_path / "ref.details")
    fasta = [k for k in dev if k.endswith(".allele_consensus.fasta")]
    assert len(fasta) == 12 and dev == want


def test_fastq_command_returns_the_planted_tracts(capi, tmp_path):
    from nanorepeat_amd import pipeline
    p = synth.structure_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), data_type="hifi", anchor_len=1000,
                                           seed=3, allele_consensus=True)
    planted = [["CAG" * 17 + "CAA" + "CAG", "CAG" * 36 + "CAA" + "CAG"],
               ["CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * m for m in (10, 28)],
               ["TATTG" * 12, "TATTG" * 30]]
    for region, tracts, inter in zip(regions, planted, p["planted"]):
        assert [ac.sequence for ac in region.allele_consensus] == tracts
        for ac, want in zip(region.allele_consensus, inter):
            assert ac.converged == 1 and ac.left_out == 0
            assert [(b, k) for k, b in ac.interruptions] == want


def test_bad_arguments_on_a_device(capi):
    for kw, code in ((dict(max_dist=-1), -1), (dict(max_dist=1001), -3), (dict(max_rounds=0), -1),
                     (dict(max_rounds=65), -3)):
        with pytest.raises(capi.NraError) as e:
            capi.tract_consensus([["CAGCAG"]], **kw)
        assert e.value.code == code, kw
    out = capi.tract_consensus([])
    assert out["consensus"] == [] and out["stats"]["rounds"] == 0
