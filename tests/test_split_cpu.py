"""Allele split without a GPU: the two restatements of the contract (full matrix, banded with the widening rule) against
each other, the invariants of the rule (permuted tracts, haplotype 0 the larger one), the corner cases of the header,
what the rule achieves on noisy reads (quality_table: DESIGN.md section 19.3), the FASTQ and BAM commands with
allele_split=True on small panels with the restatements as engines, and the C ABI's argument checks.

A haplotype cannot run empty under the contract: per site the most voted base of a haplotype's rows mismatches no more
of them than any other sequence does, so the rows of a haplotype cannot all be strictly nearer to the other one, and
both haplotypes start with a row (n[a] >= n[b] >= min_count >= 1).  The corner that does occur, and is covered here,
is a haplotype none of whose rows shows a base at a site: it takes the site's a (haplotype 0) or b (1).
"""
import re
import sys

import numpy as np
import pytest

from nanorepeat_amd import synth
import consensus_ref
import split_ref as R
from split_cases import corner_cases, seeded_groups
from structure_ref import ref_read_structure


# ---------------------------------------------------------------------------- the two restatements
def test_banded_restatement_equals_the_full_matrix():
    seen = dict(no_tracts=0, all_left=0, no_site=0, one_site=0, cut=0, undecided=0, silent_hap=0, split=0, iters=0)
    for q, (groups, bbs, kw) in enumerate(corner_cases()):
        full = R.ref_allele_split(groups, bbs, banded=False, **kw)
        band = R.ref_allele_split(groups, bbs, banded=True, **kw)
        assert R.same_result(full, band), q
        assert (full["n0"] >= full["n1"]).all()
        m = np.array([len(g) for g in groups])
        assert np.array_equal(full["n0"] + full["n1"] + full["undecided"] + full["left_out"], m)
        seen["no_tracts"] += int((m == 0).sum())
        seen["all_left"] += int(((m > 0) & (full["left_out"] == m)).sum())
        seen["no_site"] += int(((full["left_out"] < m) & (full["n_sites"] == 0)).sum())
        seen["one_site"] += int((full["n_sites"] == 1).sum())
        seen["cut"] += int(("max_sites" in kw) and (full["n_sites"] == kw["max_sites"]).all() and kw["max_sites"] < 12)
        seen["undecided"] += int((full["undecided"] > 0).sum())
        seen["silent_hap"] += sum(int(((s[:, 3:7].sum(axis=1) == 0) | (s[:, 7:11].sum(axis=1) == 0)).any())
                                  for s in full["sites"] if len(s))
        seen["split"] += int(full["split"].sum())
        seen["iters"] = max(seen["iters"], int(full["iterations"].max(initial=0)))
    assert all(seen.values()) and seen["iters"] >= 2, seen
    groups, bbs = seeded_groups(60, seed=31, max_len=500)
    for kw in ({}, dict(max_dist=25, min_sites=1, min_count=2)):
        assert R.same_result(R.ref_allele_split(groups, bbs, banded=False, **kw),
                             R.ref_allele_split(groups, bbs, banded=True, **kw))


def test_hand_cases():
    b, alt = "CAG" * 20 + "CAA" + "CAG", "CAG" * 22
    out = R.ref_allele_split([[b] * 5 + [alt] * 4, [alt] * 4 + [b] * 5, [b] * 9, []], [b, b, b, b], min_sites=1,
                             banded=False)
    assert list(out["split"]) == [1, 1, 0, 0] and list(out["n_sites"]) == [1, 1, 0, 0]
    assert list(out["label"][0]) == [0] * 5 + [1] * 4 and list(out["label"][1]) == [1] * 4 + [0] * 5
    assert list(out["sites"][0][0]) == [62, 0, 2, 5, 0, 0, 0, 0, 0, 4, 0, 1]      # column, A / G, counts, supported
    assert out["site_sym"][0].tolist() == [[0] * 5 + [2] * 4] and list(out["dist"][0]) == [0] * 5 + [1] * 4
    # one supported site is too few for min_sites 2
    out = R.ref_allele_split([[b] * 5 + [alt] * 4], [b], banded=True, min_sites=2)
    assert (out["split"][0], out["n_supported"][0], out["n0"][0], out["n1"][0]) == (0, 1, 5, 4)
    # left out by max_dist: no row, label -1, distance -1; the others carry on
    far = "T" * len(b)
    out = R.ref_allele_split([[b] * 5 + [far] + [alt] * 4], [b], max_dist=5, min_sites=1)
    assert out["label"][0][5] == -1 and out["dist"][0][5] == -1 and out["left_out"][0] == 1 and out["split"][0] == 1
    assert out["site_sym"][0][0, 5] == R.NO_ROW
    for bad in (dict(min_count=0), dict(min_share_pct=101), dict(max_sites=4097), dict(max_iter=0), dict(max_dist=1001)):
        with pytest.raises(ValueError):
            R.ref_allele_split([[b]], [b], **bad)
    with pytest.raises(ValueError):
        R.ref_allele_split([[b]], ["CAGN"])


def test_permuting_the_tracts_permutes_the_labels():
    rng = np.random.default_rng(8)
    groups, bbs = seeded_groups(30, seed=33, max_len=300)
    for groups, bbs, kw in [(groups, bbs, {})] + corner_cases()[-4:]:
        one = R.ref_allele_split(groups, bbs, **kw)
        perms = [rng.permutation(len(g)) for g in groups]
        two = R.ref_allele_split([[g[j] for j in p] for g, p in zip(groups, perms)], bbs, **kw)
        for k in R.RES_FIELDS:
            assert np.array_equal(one[k], two[k]), k
        for g, p in enumerate(perms):
            assert np.array_equal(two["label"][g], one["label"][g][p]) and np.array_equal(two["dist"][g], one["dist"][g][p])
            assert np.array_equal(two["sites"][g], one["sites"][g])
            assert np.array_equal(two["site_sym"][g], one["site_sym"][g][:, p])


# ---------------------------------------------------------------------------- what the rule achieves
CASES = (("HTT", "CAG" * 20 + "CAACAG", "CAG" * 22), ("FMR1", "CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * 10,
                                                      "CGG" * 9 + "AGG" + "CGG" * 20),
         ("RFC1", "AAGGG" * 40, "AAAAG" * 40))
MODELS = ("hifi", "ont_q20", "ont")
SHAPES = ((6, 6), (8, 8), (15, 15), (30, 30), (6, 14), (9, 21))          # reads per haplotype; the last two: 30 / 70


def quality_table(seeds=40, min_sites=(1, 2, 3), models=MODELS, shapes=SHAPES, seed=19):
    """[(model, case, n_a, n_b, {min_sites: (planted splits found, mean read accuracy where found, false splits)})],
    each over `seeds` groups of n_a + n_b reads of the two sequences and `seeds` groups of n_a + n_b reads of the first
    sequence alone; the backbone is the group's consensus, as in split.py."""
    rng = np.random.default_rng(seed)
    rows = []
    for model in models:
        for name, ta, tb in CASES:
            for na, nb in shapes:
                mixed, plain, truth = [], [], []
                for _ in range(seeds):
                    hap = np.array([0] * na + [1] * nb)[rng.permutation(na + nb)]
                    truth.append(hap)
                    mixed.append([synth.apply_errors(rng, tb if h else ta, model) for h in hap])
                    plain.append([synth.apply_errors(rng, ta, model) for _ in hap])
                bbs = consensus_ref.ref_tract_consensus(mixed + plain)["consensus"]
                cell = {}
                for ms in min_sites:
                    out = R.ref_allele_split(mixed + plain, bbs, min_sites=ms)
                    found, acc = 0, []
                    for q, hap in enumerate(truth):
                        if out["split"][q]:
                            lab = out["label"][q]
                            right = max(int((lab == hap).sum()), int((lab == 1 - hap).sum()))
                            found += 1
                            acc.append(right / len(hap))
                    cell[ms] = (found, float(np.mean(acc)) if acc else 0.0, int(out["split"][seeds:].sum()))
                rows.append((model, name, na, nb, cell))
    return rows


def test_hifi_has_no_false_split_at_the_default():
    """The condition of DESIGN.md section 19.3 on a slice of its table (the whole table takes minutes: run
    quality_table() for it): no false split on HiFi at the default min_sites, and the planted pairs are found.  The
    bounds for "found" sit below what the rule's first trial showed on HiFi (19 of 20 found, 0.96 of the reads right):
    8 of 10 and 0.9."""
    ms = R.DEFAULTS["min_sites"]
    rows = quality_table(seeds=10, min_sites=(ms,), models=("hifi",), shapes=((8, 8), (6, 14)))
    for row in rows:
        print(row)
    assert len(rows) == 6 and all(row[4][ms][2] == 0 for row in rows)
    assert all(row[4][ms][0] >= 8 and row[4][ms][1] >= 0.9 for row in rows)


# ---------------------------------------------------------------------------- the commands
def check_planted_panel(p, regions):
    """The planted pairs of synth.split_panel, and no other allele, split; every read of a pair is on its planted
    haplotype; the sub-allele consensuses are the planted tracts."""
    for g, (region, planted) in enumerate(zip(regions, p["planted"])):
        assert len(region.allele_split) == len(planted), g
        for sp, pair in zip(region.allele_split, planted):
            assert sp.split == (pair is not None), (g, sp.allele_id)
            if pair is None:
                assert not sp.sub_alleles
                continue
            assert sp.n0 == sp.n1 == 8 and sp.undecided == sp.left_out == 0
            hap = np.array([p["haplotype"][n] for n in sp.read_names])
            assert np.array_equal(sp.labels, hap) or np.array_equal(sp.labels, 1 - hap)
            assert sorted(sub.sequence for sub in sp.sub_alleles) == sorted(pair)
            assert [sub.allele_id for sub in sp.sub_alleles] == [f"{sp.allele_id}a", f"{sp.allele_id}b"]
            assert all(sub.converged == 1 and sub.voted == 8 for sub in sp.sub_alleles)


def test_planted_panel_comes_back(oracle, tmp_path, capsys):
    from nanorepeat_amd import pipeline, split
    from screen_ref import RefScreen
    p = synth.split_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), data_type="hifi", anchor_len=1000,
                                           seed=3, allele_split=True, aligner=oracle.align_pairs,
                                           scorer=oracle.round3_1d, screener=RefScreen,
                                           consensus_engine=consensus_ref.ref_tract_consensus,
                                           split_engine=R.ref_allele_split, structure_engine=ref_read_structure)
    check_planted_panel(p, regions)
    assert "NOTICE: allele split: 3 of 6 allele(s)" in capsys.readouterr().err
    # the interruption that tells the HTT pair apart is in one sub-allele's structure and not in the other's
    htt = regions[0].allele_split[0]
    assert sorted(len(sub.interruptions) for sub in htt.sub_alleles) == [0, 1]
    assert not list(tmp_path.glob("on.NanoRepeat_consensus.tsv"))            # no consensus file on the split's account
    # the files
    summary = (tmp_path / "on.NanoRepeat_split.tsv").read_text().split("\n")
    assert summary[0] == "#Chrom\tStart\tEnd\tMotif\tNum_Alleles\tAllele_Split" and len(summary) == 6
    for line, region in zip(summary[1:], regions):
        f = line.split("\t")
        assert f[3] == region.repeat_unit_seq and int(f[4]) == len(region.allele_split)
        for cell, sp in zip(f[5].split("|"), region.allele_split):
            c = cell.split(":", 7)
            assert [int(x) for x in c[:7]] == [sp.allele_id, sp.split, sp.n0, sp.n1, sp.undecided, sp.left_out, sp.n_sites]
            assert (c[7] == "-") == (not sp.supported_sites())
            assert all(re.fullmatch(r"\d+:[ACGT]/[ACGT]", s) for s in c[7].split(",")) or c[7] == "-"
    for region in regions:
        text = open(f"{region.out_prefix}.allele_split.tsv").read().split("\n")
        body = [l.split("\t") for l in text if l and not l.startswith("#")]
        assert text[0].startswith("##RepeatRegion=") and "#Read_Name\tAllele_ID\tSub_Allele\tSite_Symbols" in text
        assert len(body) == sum(len(sp.read_names) for sp in region.allele_split)
        for sp in region.allele_split:
            mine = [l for l in body if l[1] == str(sp.allele_id)]
            assert [l[0] for l in mine] == sp.read_names
            assert {l[2] for l in mine} == ({"a", "b"} if sp.split else {"-"})
            assert all(len(l[3]) == max(1, sp.n_sites) and set(l[3]) <= set(split.SYMBOLS) for l in mine)
        fasta = open(f"{region.out_prefix}.allele_split.fasta").read()
        heads = [l for l in fasta.split("\n") if l.startswith(">")]
        assert len(heads) == 2 * sum(sp.split for sp in region.allele_split)
        assert all(re.match(r">allele\d+[ab] reads=\d+ left_out=\d+ len=\d+ units=[\d.]+ rounds=\d+ converged=[01]$", h)
                   for h in heads)


def test_off_is_byte_for_byte_the_command_without_the_keyword(oracle, tmp_path, monkeypatch):
    from nanorepeat_amd import pipeline
    from test_bam import _bam_case
    from test_screen_cpu import _tree
    monkeypatch.setitem(sys.modules, "pysam", None)
    _bam_case(tmp_path)
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d)
    src, ref, bed = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed")
    pipeline.quantify_from_bam(src, ref, bed, str(tmp_path / "absent"), **common)
    pipeline.quantify_from_bam(src, ref, bed, str(tmp_path / "off"), allele_split=False, **common)
    regions = pipeline.quantify_from_bam(src, ref, bed, str(tmp_path / "on"), allele_split=True,
                                         split_engine=R.ref_allele_split, structure_engine=ref_read_structure,
                                         consensus_engine=consensus_ref.ref_tract_consensus, **common)
    out = (tmp_path / "absent.NanoRepeat_output.tsv").read_bytes()
    assert (tmp_path / "off.NanoRepeat_output.tsv").read_bytes() == out == (tmp_path / "on.NanoRepeat_output.tsv").read_bytes()
    absent, off, on = (_tree(tmp_path / f"{n}.details") for n in ("absent", "off", "on"))
    assert absent == off and {k: v for k, v in on.items() if ".allele_split." not in k} == off
    for name in ("absent", "off"):
        assert sorted(p.name for p in tmp_path.glob(f"{name}.*")) == [f"{name}.NanoRepeat_output.tsv", f"{name}.details"]
    assert sorted(p.name for p in tmp_path.glob("on.*")) == ["on.NanoRepeat_output.tsv", "on.NanoRepeat_split.tsv",
                                                             "on.details"]
    assert len([k for k in on if k.endswith(".allele_split.tsv")]) == len([k for k in on if k.endswith(".allele_split.fasta")]) == 2
    assert all(sp.split == 0 for region in regions for sp in getattr(region, "allele_split", []))


# ---------------------------------------------------------------------------- C ABI
def test_symbol_is_declared_and_exported(capi):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int nra_allele_split(" in open(os.path.join(root, "include", "nanorepeat_amd.h")).read()
    assert "nra_allele_split" in capi.EXPORTS and hasattr(capi.load(), "nra_allele_split")
    assert capi.load().nra_abi_version() == 4
    assert capi.SPLIT_DEFAULTS == R.DEFAULTS


def test_allele_split_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for kw, code in ((dict(max_dist=-1), -1), (dict(max_dist=1001), -3), (dict(min_count=0), -1), (dict(min_sites=0), -1),
                     (dict(min_share_pct=0), -1), (dict(min_share_pct=101), -3), (dict(min_purity_pct=101), -3),
                     (dict(max_sites=0), -1), (dict(max_sites=4097), -3), (dict(max_iter=0), -1), (dict(max_iter=65), -3)):
        with pytest.raises(capi.NraError) as e:
            capi.allele_split([["CAGCAG"]], ["CAGCAG"], **kw)
        assert e.value.code == code, kw
    for groups, bbs, code in (([["A" * 200001]], ["ACGT"], -3), ([["ACGT"]], ["A" * 200001], -3), ([["ACGT"]], ["ACNT"], -1)):
        with pytest.raises(capi.NraError) as e:
            capi.allele_split(groups, bbs)
        assert e.value.code == code
    with pytest.raises(TypeError):
        capi.allele_split([["ACGT"]], ["ACGT"], min_site=1)
    with pytest.raises(capi.NraError) as e:
        capi.allele_split([["CAGCAG", "CAGCAA"], []], ["CAGCAG", ""])
    assert e.value.code == -2 and "no HIP device" in str(e.value)
