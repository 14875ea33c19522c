"""What keeps tests/test_sweep_classes_gpu.py from hiding anything, proved without a device from the plans
(nra_plan1d_digest / nra_plan2d_digest) and the oracle:

  - every (form, class, N) of tests/sweep_class_cases.py plans exactly one bucket, of the intended rows per lane and the
    intended form -- so the instantiation that runs is the one the case is named for;
  - no class of NRA_R_LIST is missing for any form, but for the half-wave forms above NRA_RING32_MAX_R, which have no
    kernel; nothing is sampled, skipped or expected to fail (share of left-out cases: 0);
  - the inputs are what they claim to be, by the oracle alone;
  - the inputs of test_gpu_parity.test_large_row_counts_park_the_junction_in_agprs plan no bucket of 28 or more rows
    per lane under the flags the test had, and do under NRA_CHAIN_FROM = 3072."""
import numpy as np
import pytest

import sweep_class_cases as S

FORMS_1D, FORMS_2D = S.forms_1d(), S.forms_2d()
R_LIST = S.r_list()
PARKED = [R for R in R_LIST if R >= S.PARK_FROM_R]


def _env(monkeypatch, env):
    for k in S.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_no_class_is_missing_for_any_form():
    assert len(R_LIST) == 24 and PARKED == [28, 32, 40, 48]
    half = [R for R in R_LIST if R <= S.RING32_MAX_R]
    assert len(half) == 20
    n = 0
    for name, f in FORMS_1D.items():
        # the one exception: reads of more than 32 * NRA_RING32_MAX_R bases have no half-wave kernel
        assert S.classes_of(f) == (half if f["unit"] == 32 else R_LIST), name
        n += 2 * len(S.classes_of(f))
    assert n == 2 * (3 * 20 + 8 * 24)
    # every switch of the issue's table is in some form, the ring switches on both wave forms
    A = S.A
    flags = {f["flags"] for f in FORMS_1D.values()}
    for fl in (0, A.F_NO_QUANTA, A.F_TIE_EXTENTS, A.F_NO_HALF_WAVE, A.F_NO_HALF_WAVE | A.F_NO_QUANTA,
               A.F_NO_HALF_WAVE | A.F_FULL_ANCHORS, A.F_NO_HALF_WAVE | A.F_TIE_EXTENTS, A.F_DPP_SWEEP, A.F_BRUTE_FORCE,
               A.F_ALL_EXTENTS):
        assert fl in flags, fl
    flags2 = {(f["flags"], f["grid"], f["given"], f["refine"]) for f in FORMS_2D.values()}
    assert flags2 >= {(0, False, True, False), (0, False, False, False), (A.F_NO_JOINT_PACK, False, True, False),
                      (0, True, True, False), (A.F_JOINT_NO_CHAIN, True, True, False), (A.F_JOINT_TAILS, True, True, False),
                      (0, True, True, True)}


@pytest.mark.parametrize("name", list(FORMS_1D))
def test_1d_every_class_plans_one_bucket_of_its_form(capi, monkeypatch, name):
    f = FORMS_1D[name]
    seen = []
    for R in S.classes_of(f):
        _env(monkeypatch, S.env_of(f, R))
        for with_n in (False, True):
            d = S.batch_1d(R, f["unit"], with_n)
            assert len(d["reads"]) == 7
            plans = [S.plan_1d(d, f["flags"], simds) for simds in (1024, 16)]
            for scalars, buckets in plans:
                assert len(buckets) == 1, (name, R, with_n, buckets)
                b = buckets[0]
                assert b["R"] == R, (name, R, with_n, b["R"])
                assert {k: b[k] for k in f["bucket"]} == f["bucket"], (name, R, with_n, b)
                assert int(scalars["brute"]) == f["brute"], (name, R, with_n)
                if not f["brute"]:
                    assert b["n_sweep"] == (2 if b["half"] else 4), (name, R, b["n_sweep"])     # the last task is short
            # the same plan whatever the device's size
            assert plans[0] == plans[1], (name, R, with_n)
            seen.append((R, with_n))
    assert seen == [(R, n) for R in S.classes_of(f) for n in (False, True)]


@pytest.mark.parametrize("name", list(FORMS_2D))
def test_2d_every_class_plans_one_bucket_of_its_form(capi, name):
    f = FORMS_2D[name]
    for R in R_LIST:
        for with_n in (False, True):
            j = S.batch_2d(R, with_n)
            assert 5 <= len(j["reads"]) <= 7 and {1, -1} == set(j["strand"].tolist())
            steps = S.plan_2d(j, f)
            s = steps[0]
            assert "error" not in s and len(s["buckets"]) == 1, (name, R, with_n, s.get("error"), s["buckets"])
            b = s["buckets"][0]
            assert b["R"] == R and b["chain"] == 0, (name, R, with_n, b)
            assert (b["n_jlpk"] > 0) == (b["n_jrpk"] > 0) == f["packed"], (name, R, with_n, b)
            assert (b["n_pair"] > 0) == (not f["given"]) and s["all_strands_given"] == str(int(f["given"])), (name, R, with_n, b)
            assert b["n_jbwd"] == 7
            if f["grid"]:
                chained = int(not f["flags"] & (S.A.F_JOINT_NO_CHAIN | S.A.F_JOINT_TAILS))
                assert (s["joint_v2"], s["joint_chain"]) == (str(int(not f["flags"] & S.A.F_JOINT_TAILS)), str(chained)), (name, R)
            if f["refine"]:
                # the coarse grid keeps its column states and the refinement takes them: k_joint_midscan and
                # k_joint_combine from kept states
                assert s["keep"] == "1" and len(steps) == 2 and "error" not in steps[1] and "rf_mid" in steps[1], (name, R, steps[1])


def _oracle_1d(oracle, d):
    return oracle.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=oracle.default_scoring(**d["sc"]))


@pytest.mark.parametrize("R", R_LIST)
def test_1d_inputs_are_what_they_claim(oracle, R):
    match = oracle.default_scoring().match
    for unit in (32, 64):
        if unit == 32 and R > S.RING32_MAX_R:
            continue
        d, dn = S.batch_1d(R, unit, False), S.batch_1d(R, unit, True)
        lo, hi = S.length_range(R, unit)
        assert [len(r) for r in d["reads"]][:3] == [hi, hi, hi - 1] and len(d["reads"][6]) == lo
        assert sum("N" in r for r in dn["reads"]) == 1 and not any("N" in r for r in d["reads"])
        assert all(5 <= b - a + 1 <= 6 or a == 0 for a, b in zip(d["kmin"], d["kmax"]))
        o, on = _oracle_1d(oracle, d), _oracle_1d(oracle, dn)
        # the error-free full-length read: every base a match, so the best cell is the last row of the last lane
        if R >= 3:
            assert o["status"][0] == 0 and o["best_score"][0] == match * hi, (R, unit, o["best_score"][0])
            assert o["sum_k"][0] == d["k_true"][0] * o["n_ties"][0]
        # three reads with a size from every batch whose reads reach 64 bases; the 32-base half-wave class 1 has the
        # two its longest reads give (min_dp_score = 20)
        assert (o["status"] == 0).sum() >= (3 if hi >= 64 else 2), (R, unit, o["status"])
        assert (on["status"] == 0).sum() >= (3 if hi >= 64 else 2), (R, unit, on["status"])
        assert {1} <= set(o["status"].tolist())                                  # and a read that fails the flank test
        # the N lies on a path
        assert (o["cand_score"] != on["cand_score"]).any(), (R, unit)


@pytest.mark.parametrize("R", R_LIST)
def test_2d_inputs_are_what_they_claim(capi, oracle, R):
    j, jn = S.batch_2d(R, False), S.batch_2d(R, True)
    lo, hi = S.length_range(R, 64)
    assert [len(r) for r in j["reads"]] == [hi, hi, hi - 1, (lo + hi) // 2, (lo + hi) // 2, lo, lo]
    cr, k1, k2 = capi.joint_grid_cells(S.grids_2d(j)[0])
    assert len(cr) <= 9 * 7 and set(cr.tolist()) == set(range(7))
    sc = oracle.default_scoring(**j["sc"])
    o = oracle.joint_2d(j["region"], j["reads"], cr, k1, k2, read_strand=j["strand"], sc=sc)
    on = oracle.joint_2d(jn["region"], jn["reads"], cr, k1, k2, read_strand=jn["strand"], sc=sc)
    probed = oracle.joint_2d(j["region"], j["reads"], cr, k1, k2, sc=sc)
    assert (o["status"] == 0).sum() >= 3, (R, o["status"])
    if R >= 2:                     # (64 R_prev + 1 = 1 base in class 1: no strand to find)
        assert np.array_equal(probed["read_strand"], j["strand"]), R
    first = cr == 0
    assert o["status"][0] == 0 and o["cell_score"][first].max() == sc.match * hi, R
    assert (o["cell_score"] != on["cell_score"]).any(), R


def test_the_agpr_test_reaches_the_parked_classes_only_under_chain_from(capi, monkeypatch):
    """test_gpu_parity.test_large_row_counts_park_the_junction_in_agprs: its reads of 1.7 - 3.0 kb plan row blocks
    (k_sweep_ringmt) under the flags it had; the legs it gained under NRA_CHAIN_FROM = 3072 plan one-block ring buckets
    of 28 - 48 rows per lane, where the forward sweep parks the junction."""
    A = S.A
    d = S.agpr_test_inputs()
    _env(monkeypatch, {})
    for flags in (0, A.F_TIE_EXTENTS):
        _, buckets = S.plan_1d(d, flags)
        assert [(b["R"], b["chain"], b["mt"]) for b in buckets] == [(12, 1, 1)], (flags, buckets)
    _, buckets = S.plan_1d(d, A.F_DPP_SWEEP)
    assert [b["R"] for b in buckets] == PARKED[::-1] and not any(b["ring"] or b["chain"] for b in buckets)
    _env(monkeypatch, S.CHAIN_FROM_ENV)
    for flags in (0, A.F_TIE_EXTENTS, A.F_NO_QUANTA):
        _, buckets = S.plan_1d(d, flags)
        assert [b["R"] for b in buckets] == PARKED[::-1], (flags, buckets)
        assert all(b["ring"] and not b["chain"] and not b["half"] and b["quanta"] == (flags != A.F_NO_QUANTA) for b in buckets)
