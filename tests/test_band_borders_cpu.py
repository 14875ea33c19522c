"""The cases of tests/band_border_cases.py on the CPU: for every band class C = 1, 2, 4, 8, 16 and each of the three
restatements, the banded rule (banded=True: the formulas the device shares) equals the full matrix (banded=False) in
every field; every distance, end and class a case claims holds on the full matrix; the banded restatement ran exactly
the classes the rule takes from the true distances (B.route_stats, which the GPU test holds the device's counts
against); and the marker tracts make every backbone column a site, so the comparison sees the whole walked path.
tests/test_band_borders_gpu.py holds the device to the same full-matrix results."""
import numpy as np
import pytest

import band_border_cases as B
import consensus_ref as CR
import flank_ref as FR
import split_ref as SR


def _check_labels(routes, max_dist, what):
    """The claims of every labelled tract against its true distance and the route the rule takes from it.
    -> the classes that decided a labelled tract."""
    decided = set()
    for q, (x, d, run, ok) in enumerate(routes):
        assert ok == (d <= max_dist), (what, q, d)
        if x["dist"] is not None:
            assert (d == x["dist"]) if x["dist"] >= 0 else (d > max_dist), (what, q, x["dist"], d)
        if x["cls"] is not None:
            assert run and run[-1] == x["cls"], (what, q, x["cls"], run, d)
            decided.add(run[-1])
        elif x["dist"] == -1:
            assert not run, (what, q, run)                   # claimed to be ruled out by its length alone
    return decided


@pytest.mark.parametrize("C", B.CLASSES)
def test_split_band_equals_the_full_matrix(C):
    decided = set()
    for max_dist in B.split_max_dists(C):
        groups, (gs, bbs, kw), full = B.split_case(C, max_dist)
        band = SR.ref_allele_split(gs, bbs, banded=True, **kw)
        assert SR.same_result(band, full), (C, max_dist)
        for g, grp in enumerate(groups):
            t = len(grp["backbone"])
            assert full["n_sites"][g] == t, (C, max_dist, g)                  # the whole row of every tract is compared
            assert (full["dist"][g][grp["n_probes"]:] >= 0).all()               # no marker left out
            assert full["site_sym"][g].shape == (t, len(grp["tracts"]))
        routes = B.split_routes(groups, max_dist)
        assert [d if ok else -1 for _, d, _, ok in routes] == np.concatenate(full["dist"]).tolist()
        decided |= _check_labels(routes, max_dist, (C, max_dist))
        assert B.class_stats(band["stats"]) == B.class_stats(B.route_stats(routes)), (C, max_dist)
    assert C in decided


@pytest.mark.parametrize("C", B.CLASSES)
def test_consensus_band_equals_the_full_matrix(C):
    decided = set()
    for max_dist in B.split_max_dists(C):
        for max_rounds in (1, 2):
            labelled, groups, full = B.consensus_case(C, max_dist, max_rounds)
            band = CR.ref_tract_consensus(groups, max_dist=max_dist, max_rounds=max_rounds, banded=True)
            assert CR.same_result(band, full), (C, max_dist, max_rounds)
            assert full["consensus"] == [g["backbone"] for g in labelled]
            if max_rounds > 1:
                continue
            routes = B.split_routes(labelled, max_dist)
            decided |= _check_labels(routes, max_dist, (C, max_dist))
            left = [sum(1 for _, _, _, ok in routes[7 * g:7 * g + 7] if not ok) for g in range(len(labelled))]
            assert full["left_out"].tolist() == left
            assert B.class_stats(band["stats"]) == B.class_stats(B.route_stats(routes)), (C, max_dist)
    assert C in decided


@pytest.mark.parametrize("C", B.CLASSES)
def test_flank_band_equals_the_full_matrix(C):
    decided = set()
    for max_dist in B.flank_max_dists(C):
        groups, (gs, bbs, kw), full = B.flank_case(C, max_dist)
        band = FR.ref_flank_phase(gs, bbs, banded=True, **kw)
        assert FR.same_result(band, full), (C, max_dist)
        for g, grp in enumerate(groups):
            tl, tr = len(grp["sides"][0]), len(grp["sides"][1])
            cols = full["sites"][g][:, 0]
            assert (cols < tl).sum() >= tl - 2 and (cols >= tl).sum() >= tr - 2, (C, max_dist, g)
        routes = B.flank_routes(groups, full, max_dist)
        for q, (x, d, e, run, ok) in enumerate(routes):
            assert ok == (d >= 0)
            if x["cls"] is None and x["dist"] is None:
                assert d >= 0, (C, max_dist, q)                                 # no marker left out
            if x["dist"] is not None:
                assert (d, e) == (x["dist"], x["end"]), (C, max_dist, q, d, e, x["dist"], x["end"])
            if x["cls"] is not None:
                assert run[-1] == x["cls"], (C, max_dist, q, run, d)
                decided.add(run[-1])
        assert B.class_stats(band["stats"]) == B.class_stats(B.route_stats(routes)), (C, max_dist)
    assert C in decided


def test_routing_mix_of_every_class_shuffled():
    """What the GPU routing test compares the device with: the default-max_dist groups of every class in one call with
    the rows of every group shuffled give, row for row, the results of the separate calls."""
    mixed, perms, want = B.routing_split()
    gs, bbs, kw = B.split_call(mixed, CR.MAX_DIST)
    assert SR.same_result(SR.ref_allele_split(gs, bbs, banded=True, **kw), want)
    assert any((p != np.arange(len(p))).any() for p in perms)
    mixed, perms, want = B.routing_flank()
    gs, bbs, kw = B.flank_call(mixed, FR.MAX_DIST)
    assert FR.same_result(FR.ref_flank_phase(gs, bbs, banded=True, **kw), want)
