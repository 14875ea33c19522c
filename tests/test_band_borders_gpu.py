"""Every band class of the banded tract alignment (cons_band_align<C, FREE_END> and its walk-back, C = 1, 2, 4, 8, 16)
at its borders on the GPU: nra_allele_split, nra_tract_consensus and nra_flank_phase on the cases of
tests/band_border_cases.py, every output field bit for bit against the full matrix (banded=False: it knows nothing of
bands), never against the banded restatement.  The marker tracts of every group make every backbone column a site, so
site_sym holds, and the comparison sees, the whole walked path of every tract.  The class counters of a one-pass call
equal B.route_stats: the classes the widening rule takes from the true distances, which tests/test_band_borders_cpu.py
shows to be the banded restatement's own counts.  Parametrised by class, so a failure names the instantiation."""
import pytest

import band_border_cases as B
import consensus_ref as CR
import flank_ref as FR
from test_consensus_gpu import _same as same_consensus
from test_flank_gpu import _same as same_flank
from test_split_gpu import _same as same_split

pytestmark = pytest.mark.gpu


def _class_counts(st):
    return dict(B.class_stats(st), left_out_by_length=st["left_out_by_length"])


@pytest.mark.parametrize("C", B.CLASSES)
def test_split_of_one_class_equals_the_full_matrix(capi, C):
    for max_dist in B.split_max_dists(C):
        groups, (gs, bbs, kw), full = B.split_case(C, max_dist)
        got = capi.allele_split(gs, bbs, **kw)
        for g, grp in enumerate(groups):                                    # the whole row of every tract is compared
            assert got["n_sites"][g] == len(grp["backbone"]), (C, max_dist, g)
            assert (got["dist"][g][grp["n_probes"]:] >= 0).all(), (C, max_dist, g)
        same_split(got, full, f"class {C}, max_dist {max_dist}")
        routes = B.split_routes(groups, max_dist)
        want = dict(B.class_stats(B.route_stats(routes)), left_out_by_length=B.by_length(groups, max_dist))
        assert _class_counts(got["stats"]) == want, (C, max_dist)
        assert got["stats"][f"aligned_{64 * C}"] >= sum(1 for g in groups for x in g["tracts"] if x["cls"] == C) > 0


@pytest.mark.parametrize("C", B.CLASSES)
def test_consensus_of_one_class_equals_the_full_matrix(capi, C):
    for max_dist in B.split_max_dists(C):
        for max_rounds in (1, 2):
            labelled, groups, full = B.consensus_case(C, max_dist, max_rounds)
            got = capi.tract_consensus(groups, max_dist=max_dist, max_rounds=max_rounds)
            same_consensus(got, full, f"class {C}, max_dist {max_dist}, {max_rounds} round(s)")
            assert got["consensus"] == [g["backbone"] for g in labelled]
            if max_rounds == 1:                            # later rounds start a tract in the class that decided it
                routes = B.split_routes(labelled, max_dist)
                want = dict(B.class_stats(B.route_stats(routes)), left_out_by_length=B.by_length(labelled, max_dist))
                assert _class_counts(got["stats"]) == want, (C, max_dist)


@pytest.mark.parametrize("C", B.CLASSES)
def test_flanks_of_one_class_equal_the_full_matrix(capi, C):
    for max_dist in B.flank_max_dists(C):
        groups, (gs, bbs, kw), full = B.flank_case(C, max_dist)
        got = capi.flank_phase(gs, bbs, **kw)
        for g, grp in enumerate(groups):
            tl, tr = len(grp["sides"][0]), len(grp["sides"][1])
            cols = got["sites"][g][:, 0]
            assert (cols < tl).sum() >= tl - 2 and (cols >= tl).sum() >= tr - 2, (C, max_dist, g)
        same_flank(got, full, f"class {C}, max_dist {max_dist}")
        routes = B.flank_routes(groups, full, max_dist)
        want = dict(B.class_stats(B.route_stats(routes)), left_out_by_length=0)
        assert _class_counts(got["stats"]) == want, (C, max_dist)
        assert got["stats"][f"aligned_{64 * C}"] >= sum(1 for g in groups for x in g["rows"] if x["cls"] == C) > 0


def _with_and_without_small_chunks(monkeypatch, call, same, want):
    """One call in launches of the usual pointer budget and of 64 KB (a tract and its widened re-run then fall into
    different launches): both equal the full matrix, hence each other, and count the same classes."""
    monkeypatch.delenv("NRA_TEST_CONS_PTR_BYTES", raising=False)
    one = call()
    monkeypatch.setenv("NRA_TEST_CONS_PTR_BYTES", B.PTR_BYTES)
    many = call()
    monkeypatch.delenv("NRA_TEST_CONS_PTR_BYTES", raising=False)
    same(one, want, "one chunk")
    same(many, want, "small chunks")
    same(many, one, "small chunks against one chunk")
    assert many["stats"]["launches"] > one["stats"]["launches"]
    assert many["stats"]["max_pointer_bytes"] < one["stats"]["max_pointer_bytes"]
    return one, many


def test_host_routing_of_a_mix_of_every_class(capi, monkeypatch):
    mixed, _, want = B.routing_split()
    gs, bbs, kw = B.split_call(mixed, CR.MAX_DIST)
    one, many = _with_and_without_small_chunks(monkeypatch, lambda: capi.allele_split(gs, bbs, **kw), same_split, want)
    assert _class_counts(many["stats"]) == _class_counts(one["stats"])
    assert all(one["stats"][f"aligned_{w}"] > 0 for w in (64, 128, 256, 512, 1024))

    mixed, _, want = B.routing_flank()
    gs, bbs, kw = B.flank_call(mixed, FR.MAX_DIST)
    one, many = _with_and_without_small_chunks(monkeypatch, lambda: capi.flank_phase(gs, bbs, **kw), same_flank, want)
    assert _class_counts(many["stats"]) == _class_counts(one["stats"])
    assert all(one["stats"][f"aligned_{w}"] > 0 for w in (64, 128, 256, 512, 1024))

    groups, want = B.routing_consensus()
    one, many = _with_and_without_small_chunks(monkeypatch, lambda: capi.tract_consensus(groups, max_rounds=2),
                                               same_consensus, want)
    assert all(one["stats"][f"aligned_{w}"] > 0 for w in (64, 128, 256, 512, 1024))
