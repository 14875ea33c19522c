"""The saturation exit of the forward sweeps in quanta: a sweep whose wave state repeats from one unit
boundary to the next ends there and writes its last value for every repeat count left.  It may change no result: every case
runs one batch three ways -- with the exit, with NRA_TEST_SAT=0 and as two launches per bucket (NRA_F_NO_QUANTA, the untouched
kernels) -- with NRA_TEST_POISON_OUTPUTS, so that a candidate the exit left unwritten would show, and requires identical
results; a sample of the reads is compared with the CPU oracle.  `saturation()` says whether the exit was taken at all."""
import functools

import numpy as np
import pytest

from nanorepeat_amd import synth

pytestmark = pytest.mark.gpu

PER_READ = ("best_score", "sum_k", "n_ties", "status")
KEYS_1D = PER_READ + ("cand_score", "cand_tstart", "cand_tend")
UNITS = {1: "A", 2: "AC", 5: "TATTG", 8: "ACGGTCAT"}        # the unit length is the forward sweep's skew


def make_batch(unit, n=12, anchor=150, flank=40, k_true=10, kmin=1, kmax=150, model="ont", seed=0, with_n=False):
    """One region with anchors of `anchor` bases; n reads of `flank` + unit * k_true + `flank` bases before errors.  k_true,
    kmin and kmax: one value for all reads or one per read."""
    rng = np.random.default_rng(7000 + 100 * len(unit) + seed)
    left, right = synth.rand_seq(rng, anchor), synth.rand_seq(rng, anchor)
    per = lambda v: [int(x) for x in (np.full(n, v) if np.isscalar(v) else v)]
    ks, lo, hi = per(k_true), per(kmin), per(kmax)
    reads = []
    for i in range(n):
        s = synth.apply_errors(rng, left[anchor - flank:] + unit * ks[i] + right[:flank], model)
        if with_n and i % 2 == 0:
            p = rng.integers(5, len(s) - 5, size=3)
            s = "".join("N" if j in p else c for j, c in enumerate(s))
        reads.append(s)
    return dict(regions=[(left, unit, right)], reads=reads, kmin=np.array(lo, np.int32), kmax=np.array(hi, np.int32),
                read_region=None)


def run_once(capi, d, flags=0, runs=1):
    b = capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d.get("read_region"),
                             sc=capi.default_scoring(), flags=flags)
    try:
        outs = []
        for _ in range(runs):
            b.run()
            b.sync()
            outs.append((b.fetch(), b.saturation()))
        return outs
    finally:
        b.close()


def same(a, b, what):
    for k in KEYS_1D:
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:8])


def three_ways(capi, monkeypatch, d, flags=0, qsteps=None, what=""):
    """The batch with the exit, without it and as two launches per bucket: identical results.  Returns the first run's
    results and what its `saturation()` reports."""
    monkeypatch.setenv("NRA_TEST_POISON_OUTPUTS", "1")
    if qsteps is not None:
        monkeypatch.setenv("NRA_TEST_QSTEPS", str(qsteps))
    (g, sat), = run_once(capi, d, flags)
    monkeypatch.setenv("NRA_TEST_SAT", "0")
    (off, sat_off), = run_once(capi, d, flags)
    monkeypatch.delenv("NRA_TEST_SAT")
    (two, sat_two), = run_once(capi, d, flags | capi.F_NO_QUANTA)
    print(what, "saturation", sat)
    same(g, off, what + ": exit against NRA_TEST_SAT=0")
    same(g, two, what + ": exit against two launches")
    assert sat["sweeps_total"] > 0 and sat["steps_total"] > 0
    assert 0 <= sat["sweeps"] <= sat["sweeps_total"] and 0 <= sat["steps"] < sat["steps_total"]
    assert (sat["sweeps"] > 0) == (sat["steps"] > 0)
    assert sat_off["sweeps"] == 0 and sat_off["steps"] == 0 and sat_off["sweeps_total"] == sat["sweeps_total"]
    assert sat_two == dict(sweeps=0, steps=0, sweeps_total=0, steps_total=0)
    return g, sat


def oracle_sample(oracle, d, g, pick, what):
    """The reads `pick` of the result g against the oracle on those reads alone: the per-read results, the scores of every
    candidate, and the extents the library computed (the default mode computes them for ambiguous ties only)."""
    pick = np.asarray(pick)
    o = oracle.round3_1d(d["regions"], [d["reads"][i] for i in pick], d["kmin"][pick], d["kmax"][pick],
                         sc=oracle.default_scoring())
    for k in PER_READ:
        assert np.array_equal(g[k][pick], o[k]), (what, k)
    n_cand = np.maximum(d["kmax"].astype(np.int64) - d["kmin"] + 1, 0)
    off = np.concatenate([[0], np.cumsum(n_cand)])
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in pick])
    assert np.array_equal(g["cand_score"][idx], o["cand_score"]), (what, "cand_score")
    have = g["cand_tstart"][idx] >= 0
    assert np.array_equal(g["cand_tstart"][idx][have], o["cand_tstart"][have]), (what, "cand_tstart")
    assert np.array_equal(g["cand_tend"][idx][have], o["cand_tend"][have]), (what, "cand_tend")


@functools.lru_cache(maxsize=None)
def shape_batch(m):
    return make_batch(UNITS[m])


# ------------------------------------------------------------------ the shapes: the exit is taken
@pytest.mark.parametrize("qsteps", [64, 128, 384])
@pytest.mark.parametrize("m", [1, 2, 5, 8])
def test_exit_is_taken_and_changes_nothing(capi, oracle, monkeypatch, m, qsteps):
    """Anchors of 150 bases, a dozen reads of 40 + unit * 10 + 40 bases with ONT errors, k in [1, 150]: the column state stops
    changing long before k = 150 for every unit length.  A forward sweep has 331 steps with a unit of one base and 1598 with
    one of eight, so where the exit falls differs over the grid: with a unit of one base and parts of 384 steps in the
    sweep's last part, with the longer units or parts of 64 steps in an earlier part, whose later parts then find the sweep
    finished and leave.  No single cell of the grid covers all of that; the grid does."""
    d = shape_batch(m)
    g, sat = three_ways(capi, monkeypatch, d, qsteps=qsteps, what=f"m={m} qsteps={qsteps}")
    assert sat["sweeps"] > 0 and sat["steps"] > 0
    oracle_sample(oracle, d, g, [0, 5, 11], f"m={m} qsteps={qsteps}")


@pytest.mark.parametrize("sat_steps", [0, 64, 192])
def test_checkpoint_spacing(capi, oracle, monkeypatch, sat_steps):
    """NRA_TEST_SAT_STEPS: checks at the starts of the parts only (0), and checkpoints every 64 and 192 steps."""
    monkeypatch.setenv("NRA_TEST_SAT_STEPS", str(sat_steps))
    d = make_batch("TATTG", anchor=400, flank=60, seed=1)
    g, sat = three_ways(capi, monkeypatch, d, qsteps=128, what=f"sat_steps={sat_steps}")
    assert sat["sweeps"] > 0 and sat["steps"] > 0
    oracle_sample(oracle, d, g, [1, 6], f"sat_steps={sat_steps}")


def test_default_parts(capi, oracle, monkeypatch):
    """No NRA_TEST_QSTEPS: a batch of fewer tasks than SIMDs runs a forward sweep as two parts, the second one with
    checkpoints inside it."""
    d = shape_batch(5)
    g, sat = three_ways(capi, monkeypatch, d, what="default parts")
    assert sat["sweeps"] > 0 and sat["steps"] > 0


# ------------------------------------------------------------------ beyond the shapes
def test_allele_near_kmax(capi, oracle, monkeypatch):
    """k_true = 145 of kmax = 150: the state repeats, if at all, a few boundaries before the end (no counter asserted)."""
    d = make_batch("TATTG", n=8, k_true=145, seed=2)
    g, _ = three_ways(capi, monkeypatch, d, qsteps=128, what="near kmax")
    oracle_sample(oracle, d, g, [0, 7], "near kmax")


@pytest.mark.parametrize("qsteps", [64, 384])
def test_window_that_starts_late(capi, oracle, monkeypatch, qsteps):
    """kmin = 120 with k_true = 10: the state repeats long before the first emission, and the sweep has to go on to it."""
    d = make_batch("TATTG", n=8, kmin=120, seed=3)
    g, _ = three_ways(capi, monkeypatch, d, qsteps=qsteps, what="late window")
    oracle_sample(oracle, d, g, [0, 3], "late window")


@pytest.mark.parametrize("flags", ["half", "full"])
def test_reads_of_a_task_with_different_windows(capi, oracle, monkeypatch, flags):
    """The reads of a pair (of a half-wave task: of two pairs) with windows of their own: the exit writes every read's own
    candidates and no other."""
    n = 10
    d = make_batch("AC", n=n, kmin=[1 + 7 * (i % 4) for i in range(n)], kmax=[150 - 11 * (i % 3) for i in range(n)], seed=4)
    g, sat = three_ways(capi, monkeypatch, d, flags=0 if flags == "half" else capi.F_NO_HALF_WAVE, qsteps=128, what="windows")
    oracle_sample(oracle, d, g, [0, 1, 2, 3], "windows")


@pytest.mark.parametrize("flags", ["half", "full"])
def test_reads_of_a_pair_that_stop_changing_apart(capi, oracle, monkeypatch, flags):
    """Alleles of 5 and 60 units side by side: a wave leaves only when both reads of its pair, and both halves of a half-wave
    task, repeat."""
    n = 6
    d = make_batch("TATTG", n=n, flank=35, k_true=[5 if i % 2 else 60 for i in range(n)], seed=5)
    g, sat = three_ways(capi, monkeypatch, d, flags=0 if flags == "half" else capi.F_NO_HALF_WAVE, qsteps=128, what="apart")
    oracle_sample(oracle, d, g, [0, 1], "apart")


@pytest.mark.parametrize("n", [1, 5, 6])
def test_half_wave_tasks_with_an_empty_or_odd_half(capi, oracle, monkeypatch, n):
    """One read, five reads (a pair of one read) and six (three pairs: a task whose upper half has no reads)."""
    d = make_batch("TATTG", n=n, seed=6)
    g, sat = three_ways(capi, monkeypatch, d, qsteps=128, what=f"{n} reads")
    assert sat["sweeps"] > 0
    oracle_sample(oracle, d, g, [0, n - 1], f"{n} reads")


def test_reads_with_n(capi, oracle, monkeypatch):
    d = make_batch("TATTG", n=8, seed=7, with_n=True)
    assert any("N" in r for r in d["reads"])
    g, sat = three_ways(capi, monkeypatch, d, qsteps=128, what="N")
    assert sat["sweeps"] > 0
    oracle_sample(oracle, d, g, [0, 1, 2], "N")


@pytest.mark.parametrize("relax_c", [0, 64])
def test_relaxed_anchor_columns_on_and_off(capi, oracle, monkeypatch, relax_c):
    """NRA_RELAX_C=64: the relaxed steps are on with anchors of 150 bases (the taint scheme); 0: the exact cell alone."""
    monkeypatch.setenv("NRA_RELAX_C", str(relax_c))
    d = shape_batch(5)
    b = capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"])
    try:
        assert (b.resweeps()["tasks_total"] > 0) == (relax_c > 0)
    finally:
        b.close()
    g, sat = three_ways(capi, monkeypatch, d, qsteps=128, what=f"relax_c={relax_c}")
    assert sat["sweeps"] > 0
    oracle_sample(oracle, d, g, [2, 9], f"relax_c={relax_c}")


def test_two_runs_of_one_batch(capi, monkeypatch):
    """The arrival words and the counters are words of the run: a second run starts clean and reports the same."""
    monkeypatch.setenv("NRA_TEST_POISON_OUTPUTS", "1")
    monkeypatch.setenv("NRA_TEST_QSTEPS", "128")
    d = shape_batch(2)
    (g1, s1), (g2, s2) = run_once(capi, d, runs=2)
    same(g1, g2, "second run")
    assert s1 == s2 and s1["sweeps"] > 0


@pytest.mark.parametrize("family", ["half", "full"])
def test_families_by_read_length(capi, oracle, monkeypatch, family):
    """Reads of about 330 bases (two pairs per wave) and of about 900 (one pair per wave, 15 rows per lane), anchors of 400
    bases; the window leaves the full wave its 64 boundaries of pipeline behind the allele."""
    k_true, kmax = (50, 200) if family == "half" else (160, 320)
    d = make_batch("TATTG", n=6, anchor=400, flank=50, k_true=k_true, kmin=5, kmax=kmax, seed=8)
    q = [len(r) for r in d["reads"]]
    assert max(q) <= 768 if family == "half" else min(q) > 768
    g, sat = three_ways(capi, monkeypatch, d, what=family)
    assert sat["sweeps"] > 0 and sat["steps"] > 0
    oracle_sample(oracle, d, g, [0, 5], family)
