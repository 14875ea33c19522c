"""Allele split on the GPU: nra_allele_split (k_split_align, k_split_count, k_split_phase) against tests/split_ref.py,
every output field bit for bit -- the corner cases of the contract against the full matrix, 200 seeded groups over every
band class (a third of them with a planted second haplotype), a 20 kb group, forced small pointer chunks, shuffled
groups, config 2 at full size with a planted haplotype, every tenth region of config 4, and the FASTQ command end to
end."""

import numpy as np
import pytest

from nanorepeat_amd import synth
import split_ref as R
from split_cases import corner_cases, seeded_groups, long_group

pytestmark = pytest.mark.gpu

FLANK = 100
FIELDS = ("label", "dist", "sites", "site_sym")


def _same(got, want, what=""):
    for k in R.RES_FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in FIELDS:
        assert len(got[k]) == len(want[k]), (what, k)
        for g, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape and np.array_equal(a, b), (what, k, g)


def _pick(out, idx):
    sub = {k: [out[k][i] for i in idx] for k in FIELDS}
    sub.update({k: out[k][idx] for k in R.RES_FIELDS})
    return sub


def test_corner_cases_equal_the_full_matrix(capi):
    for q, (groups, bbs, kw) in enumerate(corner_cases()):
        _same(capi.allele_split(groups, bbs, **kw), R.ref_allele_split(groups, bbs, banded=False, **kw), f"call {q}")


def test_200_seeded_groups_run_every_band_class(capi):
    groups, bbs = seeded_groups(200)
    got = capi.allele_split(groups, bbs)
    want = R.ref_allele_split(groups, bbs, banded=True)
    _same(got, want)
    st = got["stats"]
    for width in (64, 128, 256, 512, 1024):
        assert st[f"aligned_{width}"] > 0 and st[f"rows_{width}"] > 0, st
    assert st["widened"] > 0 and st["sites"] == int(got["n_sites"].sum()) and st["groups_split"] == int(got["split"].sum())
    assert got["split"].sum() >= 20                             # of the planted third; many of those are too thin to call
    assert (got["left_out"] > 0).any() and (got["undecided"] > 0).any()
    small = [q for q, g in enumerate(groups) if max(len(t) for t in g) <= 400][:40]
    assert len(small) >= 20
    _same(capi.allele_split([groups[q] for q in small], [bbs[q] for q in small], min_sites=1),
          R.ref_allele_split([groups[q] for q in small], [bbs[q] for q in small], banded=False, min_sites=1), "full matrix")


def test_20kb_group(capi):
    g, bb = long_group()
    g2, bb2 = seeded_groups(3, seed=5)
    groups, bbs = [g, g2[1]], [bb, bb2[1]]
    got = capi.allele_split(groups, bbs)
    _same(got, R.ref_allele_split(groups, bbs, banded=True))
    # three bases are planted in every other read; a site needs all three of them to show its base (min_count 3)
    assert got["split"][0] == 1 and (got["n0"][0], got["n1"][0]) == (3, 3)
    assert {int(s[0]) for s in got["sites"][0] if s[11]} <= {3000, 11111, 17002}
    with pytest.raises(capi.NraError) as e:
        capi.allele_split([["A" * 200001]], ["ACGT"])
    assert e.value.code == capi.E_RANGE
    with pytest.raises(capi.NraError) as e:
        capi.allele_split([["ACGT"]], ["A" * 200001])
    assert e.value.code == capi.E_RANGE


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch):
    groups, bbs = seeded_groups(60, seed=21, max_len=1500)
    monkeypatch.delenv("NRA_TEST_CONS_PTR_BYTES", raising=False)
    one = capi.allele_split(groups, bbs)
    monkeypatch.setenv("NRA_TEST_CONS_PTR_BYTES", "65536")
    many = capi.allele_split(groups, bbs)
    _same(many, one)
    assert many["stats"]["launches"] > 4 * one["stats"]["launches"]
    assert many["stats"]["max_pointer_bytes"] < one["stats"]["max_pointer_bytes"]


def test_shuffled_groups_and_tracts(capi):
    groups, bbs = seeded_groups(80, seed=22, max_len=1200)
    groups, bbs = groups + [[], ["", ""]], bbs + ["CAGCAG", "CAG"]
    one = capi.allele_split(groups, bbs)
    rng = np.random.default_rng(4)
    order = rng.permutation(len(groups))
    perms = [rng.permutation(len(groups[i])) for i in order]
    two = capi.allele_split([[groups[i][j] for j in p] for i, p in zip(order, perms)], [bbs[i] for i in order])
    for at, (i, p) in enumerate(zip(order, perms)):
        for k in R.RES_FIELDS:
            assert two[k][at] == one[k][i], (k, i)
        assert np.array_equal(two["sites"][at], one["sites"][i])
        assert np.array_equal(two["label"][at], one["label"][i][p]) and np.array_equal(two["dist"][at], one["dist"][i][p])
        assert np.array_equal(two["site_sym"][at], one["site_sym"][i][:, p])


def test_config2_full_size_with_a_planted_haplotype(capi):
    d = synth.config2()
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    short = [t for t, k in zip(tracts, d["k_true"]) if k == 40]
    n_long = sum(1 for k in d["k_true"] if k == 150)
    assert min(len(short), n_long) > 4000
    truth = "TATTG" * 150
    other = "TATTG" * 75 + "TATCG" + "TATTG" * 74                 # one unit substituted, before the error channel
    rng = np.random.default_rng(77)
    long_ = synth.apply_errors_batch(rng, [other if q % 2 else truth for q in range(n_long)], "ont")
    groups, bbs = [short, long_], ["TATTG" * 40, truth]
    for kw in (dict(min_sites=1), {}):
        got = capi.allele_split(groups, bbs, **kw)
        want = R.ref_allele_split(groups, bbs, banded=True, **kw)
        print({k: got[k].tolist() for k in R.RES_FIELDS})
        _same(got, want, str(kw))


def test_config4_every_tenth_region(capi):
    d = synth.config4()
    rr, kt = np.asarray(d["read_region"]), np.asarray(d["k_true"])
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    groups, bbs, region_of = [], [], []
    for g in range(len(d["regions"])):                          # one group per true allele of every region
        mine = np.nonzero(rr == g)[0]
        for a in sorted(set(kt[mine].tolist())):
            groups.append([tracts[i] for i in mine[kt[mine] == a]])
            bbs.append(synth.config4_region(g)["unit"] * int(a))
            region_of.append(g)
    got = capi.allele_split(groups, bbs)
    pick = [q for q in range(len(groups)) if region_of[q] % 10 == 0]
    want = R.ref_allele_split([groups[q] for q in pick], [bbs[q] for q in pick], banded=True)
    _same(_pick(got, pick), want)


def test_fastq_command_device_equals_restatement_files(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    import consensus_ref
    p = synth.panel(12, anchor_len=1000, reads_per_region=8, edge_overlaps=(150, 300), n_decoys=36, shared=0, seed=21)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont", anchor_len=1000, seed=3, allele_split=True)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "dev"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), split_engine=R.ref_allele_split,
                                 consensus_engine=consensus_ref.ref_tract_consensus, **common)
    assert (tmp_path / "dev.NanoRepeat_split.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_split.tsv").read_bytes()
    dev, want = _tree(tmp_path / "dev.details"), _tree(tmp_path / "ref.details")
    assert len([k for k in dev if k.endswith(".allele_split.tsv")]) == 12 and dev == want
    assert not [k for k in dev if k.endswith(".allele_consensus.fasta")]


def test_fastq_command_recovers_the_planted_panel(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_split_cpu import check_planted_panel
    p = synth.split_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), data_type="hifi", anchor_len=1000,
                                           seed=3, allele_split=True)
    check_planted_panel(p, regions)


def test_bad_arguments_on_a_device(capi):
    for kw, code in ((dict(max_dist=-1), -1), (dict(max_dist=1001), -3), (dict(min_count=0), -1), (dict(min_sites=0), -1),
                     (dict(min_share_pct=0), -1), (dict(min_share_pct=101), -3), (dict(min_purity_pct=-5), -1),
                     (dict(min_purity_pct=101), -3), (dict(max_sites=0), -1), (dict(max_sites=4097), -3),
                     (dict(max_iter=0), -1), (dict(max_iter=65), -3)):
        with pytest.raises(capi.NraError) as e:
            capi.allele_split([["CAGCAG"]], ["CAGCAG"], **kw)
        assert e.value.code == code, kw
    with pytest.raises(capi.NraError) as e:
        capi.allele_split([["CAGCAG"]], ["CAGNAG"])
    assert e.value.code == -1
    out = capi.allele_split([], [])
    assert out["label"] == [] and out["stats"]["launches"] == 0
    out = capi.allele_split([["CAGCAG"] * 3], ["CAGCAG"], max_sites=4096, max_iter=64, min_share_pct=100)
    assert (out["n0"][0], out["split"][0], out["n_sites"][0]) == (3, 0, 0)
