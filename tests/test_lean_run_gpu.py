"""The lean 1D run: the switch from the relaxed to the exact cell at the margin itself (any step, not a
multiple of 64), no per-run clear of an array that a kernel of the run writes in full, the give-up words inside the result
block.  The column tables at the ends of their blocks of columns are checked too.  None of it may change a result: every case is
compared with the CPU oracle, and with the library's own other forms where there is one.

Against the oracle, `cand_tstart` / `cand_tend` are compared in full where the mode computes the extents of every tie (the
oracle does); the default mode runs the extents kernel only for ties whose flank verdict is ambiguous, so there the extents
it did compute must be the oracle's, everything else must read -1, and the per-read results carry the rest."""
import functools

import numpy as np
import pytest

from nanorepeat_amd import synth

pytestmark = pytest.mark.gpu

KEYS_1D = ("best_score", "sum_k", "n_ties", "status", "cand_score", "cand_tstart", "cand_tend")


def run_batch(capi, d, flags=0, runs=1, clears=None):
    """`runs` runs of one batch, each fetched: the later ones start from what the earlier ones left on the device.
    `clears`: what a run of the batch must report to clear first (nra_batch1d_clears)."""
    b = capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d.get("read_region"),
                             sc=capi.default_scoring(), flags=flags)
    try:
        if clears is not None:
            assert b.clears() == clears
        outs = []
        for _ in range(runs):
            b.run()
            b.sync()
            outs.append(b.fetch())
        return outs, b.resweeps()
    finally:
        b.close()


def same(a, b, what=""):
    for k in KEYS_1D:
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:8])


def same_as_oracle(g, o, every_tie, what=""):
    for k in KEYS_1D[:5]:
        assert np.array_equal(g[k], o[k]), (what, k, np.nonzero(np.asarray(g[k]) != np.asarray(o[k]))[0][:8])
    if every_tie:
        assert np.array_equal(g["cand_tstart"], o["cand_tstart"]) and np.array_equal(g["cand_tend"], o["cand_tend"]), what
        return
    have = g["cand_tstart"] >= 0
    assert (o["cand_tstart"][have] >= 0).all(), what                    # extents only at ties
    assert np.array_equal(g["cand_tstart"][have], o["cand_tstart"][have]), what
    assert np.array_equal(g["cand_tend"][have], o["cand_tend"][have]), what
    assert (g["cand_tstart"][~have] == -1).all() and (g["cand_tend"][~have] == -1).all(), what


def oracle_1d(oracle, d, flags=0):
    return oracle.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d.get("read_region"),
                            sc=oracle.default_scoring(), flags=flags)


# ------------------------------------------------------------------ the switch step
SWITCH_C = 200          # NRA_RELAX_C of the switch-step cases: anchors of delta + 200 bases, T = delta


@functools.lru_cache(maxsize=None)
def switch_batch(m, delta):
    """One region with anchors of delta + SWITCH_C bases and a unit of m bases: nine reads of 100 - 400 bases (the
    half-wave bucket, an odd number) and five of about 800 (the full-wave bucket), none reaching more than 120 bases
    into an anchor."""
    rng = np.random.default_rng(1000 * m + delta)
    anchor = delta + SWITCH_C
    left, right, unit = synth.rand_seq(rng, anchor), synth.rand_seq(rng, anchor), synth.rand_unit(rng, m)
    reads, kmin, kmax = [], [], []
    for i in range(14):
        if i < 9:
            fl, fr = 30 + 10 * i, 120 - 10 * i
            k = max(1, (40 + 25 * i) // m)
        else:
            fl, fr = 90 + 5 * (i - 9), 110 - 5 * (i - 9)
            k = (600 + 7 * (i - 9)) // m
        reads.append(synth.apply_errors(rng, left[anchor - fl:] + unit * k + right[:fr], "ont_q20"))
        kmin.append(max(0, k - 4 - i % 2)); kmax.append(k + 4)
    return dict(regions=[(left, unit, right)], reads=reads, kmin=np.array(kmin, np.int32), kmax=np.array(kmax, np.int32),
                read_region=None)


@functools.lru_cache(maxsize=None)
def switch_oracle(oracle, m, delta):
    return oracle_1d(oracle, switch_batch(m, delta))


@pytest.mark.parametrize("qsteps", [64, 384])
@pytest.mark.parametrize("m", [1, 3, 5, 8])
@pytest.mark.parametrize("delta", [63, 64, 65, 127, 129, 191])
def test_switch_step_at_the_margin(capi, oracle, monkeypatch, delta, m, qsteps):
    """flank - c = delta: no relaxed step (63), T = 64 on a cut of 64-step parts, 65 one step behind it, 127 / 129 / 191
    inside a part or behind a cut, and all of them inside part 0 of 384-step parts.  The unit length is the forward sweep's
    skew.  (A bucket whose longest sweep would make more than NRA_Q_MAX_PARTS parts of 64 steps gets parts of 128: the
    full-wave bucket from m = 3 on; the half-wave bucket keeps parts of 64 for every m.)"""
    monkeypatch.setenv("NRA_RELAX_C", str(SWITCH_C))
    monkeypatch.setenv("NRA_TEST_QSTEPS", str(qsteps))
    d = switch_batch(m, delta)
    assert sum(len(r) <= 400 for r in d["reads"]) == 9 and sum(len(r) > 768 for r in d["reads"]) == 5
    (g,), rs = run_batch(capi, d)
    (f,), rs_full = run_batch(capi, d, flags=capi.F_FULL_ANCHORS)
    same(g, f, "full anchors")
    same_as_oracle(g, switch_oracle(oracle, m, delta), False)
    print("re-swept", rs)
    assert rs["tasks_total"] > 0 and rs["reads_total"] == len(d["reads"]) and rs_full["tasks_total"] == 0


# ------------------------------------------------------------------ poisoned outputs
@functools.lru_cache(maxsize=None)
def mixed_batch(row_block):
    """Every kernel family and corner of the selection in one batch: a full-wave pair, five half-wave reads (a task of four
    and a task with an empty upper half), a pair whose windows differ, a read with kmax < kmin, reads built to tie (a unit
    that lost a base, a base inserted into the tract), a unit of 9 bases (the DPP sweeps) and, with `row_block`, a read of
    about 3.2 kb (row blocks as concurrent waves)."""
    rng = np.random.default_rng(606)
    L0, R0 = synth.rand_seq(rng, 400), synth.rand_seq(rng, 400)
    L1, R1, u9 = synth.rand_seq(rng, 300), synth.rand_seq(rng, 300), "ACGGTCATG"
    regions = [(L0, "CAG", R0), (L1, u9, R1)]
    core = lambda k, fl=80, fr=80: L0[400 - fl:] + "CAG" * k + R0[:fr]
    reads, rr, kmin, kmax = [], [], [], []

    def add(seq, region, lo, hi):
        reads.append(seq); rr.append(region); kmin.append(lo); kmax.append(hi)
    for k in (215, 222):                                                # a full-wave pair (> 768 bases)
        add(synth.apply_errors(rng, core(k, 90, 90), "ont_q20"), 0, k - 6, k + 6)
    for k in (20, 31, 44, 57, 70):                                      # half-wave: 4 + 1
        add(synth.apply_errors(rng, core(k), "ont"), 0, max(0, k - 8), k + 8)
    add(core(12), 0, 5, 4)                                              # skipped: kmax < kmin
    add(synth.apply_errors(rng, core(90, 100, 100), "hifi"), 0, 80, 95)  # a pair of one length class, windows that differ
    add(synth.apply_errors(rng, core(92, 100, 100), "hifi"), 0, 70, 110)
    for k in (6, 10, 14):                                               # ties, as tests/test_gpu_parity.py builds them
        s = L0[-70:] + "CAG" * k + R0[:70]
        add(s, 0, 0, 22); add(s[:70 + 9] + s[70 + 10:], 0, 0, 22); add(s[:70 + 6] + "T" + s[70 + 6:], 0, 0, 22)
    for s in ("CAG" * 12, L0[-70:] + "CAG" * 9, "CAG" * 12 + R0[:60], L0[-70:] + "CAG" * 9 + R0[:1]):
        add(s, 0, 0, 20)                                                # a flank missing: ties on the junction
    for k in (7, 11, 12):                                               # a unit of 9 bases
        add(synth.apply_errors(rng, L1[-70:] + u9 * k + R1[:70], "ont_q20"), 1, max(0, k - 5), k + 5)
    if row_block:
        add(synth.apply_errors(rng, core(1000, 100, 100), "hifi"), 0, 996, 1004)
    return dict(regions=regions, reads=reads, kmin=np.array(kmin, np.int32), kmax=np.array(kmax, np.int32),
                read_region=np.array(rr, np.int32))


@pytest.mark.parametrize("mode", ["default", "BRUTE_FORCE", "ALL_EXTENTS", "TIE_EXTENTS"])
def test_poisoned_outputs_reach_no_result(capi, oracle, monkeypatch, mode):
    """NRA_TEST_POISON_OUTPUTS fills every array that a run no longer clears with 0x5a first.  Two poisoned runs of one
    batch (the second on top of the first one's results), and a run of a fresh batch without the hook, give the same
    results, the oracle's.  Brute force and NRA_F_ALL_EXTENTS hold one register block per read: no row-block read there."""
    flags = 0 if mode == "default" else getattr(capi, "F_" + mode)
    d = mixed_batch(mode in ("default", "TIE_EXTENTS"))
    if mode == "default":
        assert max(len(r) for r in d["reads"]) > 3072
    # the lean path is the one under test: the default mode clears neither scores nor extents (every kernel family of the
    # batch writes all its candidates), the other modes keep the clear of the scores, ALL_EXTENTS that of the extents too
    clears = dict(scores=mode != "default", extents=mode == "ALL_EXTENTS")
    monkeypatch.setenv("NRA_TEST_POISON_OUTPUTS", "1")
    (p1, p2), _ = run_batch(capi, d, flags=flags, runs=2, clears=clears)
    monkeypatch.delenv("NRA_TEST_POISON_OUTPUTS")
    (g,), _ = run_batch(capi, d, flags=flags)
    same(p1, g, "first poisoned run")
    same(p2, g, "second poisoned run")
    o = oracle_1d(oracle, d, flags=flags if mode == "ALL_EXTENTS" else 0)
    same_as_oracle(g, o, mode != "default", mode)
    assert (g["n_ties"] > 1).any()                                       # ties were summed ...
    if mode in ("BRUTE_FORCE", "TIE_EXTENTS"):                           # ... extents exactly at the ties, -1 elsewhere
        n_cand = np.maximum(d["kmax"] - d["kmin"] + 1, 0)
        ties = (g["cand_score"] >= 0) & (g["cand_score"] == np.repeat(g["best_score"], n_cand))
        assert ties.any() and np.array_equal(g["cand_tstart"] >= 0, ties) and np.array_equal(g["cand_tend"] >= 0, ties)


def test_an_empty_read_keeps_the_clears(capi, oracle, monkeypatch):
    """An empty read with a window is in no bucket: no sweep writes its candidates, so the batch keeps the clear of the
    scores, and the read comes out without a record, poisoned or not."""
    d = switch_batch(3, 127)
    d = dict(d, reads=list(d["reads"]) + [""], kmin=np.append(d["kmin"], 0).astype(np.int32),
             kmax=np.append(d["kmax"], 7).astype(np.int32))
    monkeypatch.setenv("NRA_TEST_POISON_OUTPUTS", "1")
    (p,), _ = run_batch(capi, d, clears=dict(scores=True, extents=False))
    monkeypatch.delenv("NRA_TEST_POISON_OUTPUTS")
    (g,), _ = run_batch(capi, d)
    same(p, g)
    same_as_oracle(g, oracle_1d(oracle, d), False)
    assert g["status"][-1] == 2 and (g["cand_score"][-8:] == -1).all()


# ------------------------------------------------------------------ the give-up word
@pytest.mark.parametrize("kind", ["quanta", "row_blocks"])
def test_give_up_word_fails_the_fetch(capi, oracle, monkeypatch, kind):
    """NRA_TEST_MT_GIVEUP starts a run with its give-up words set: the fetch (no sync before it) reports NRA_E_DEVICE
    instead of results; a fresh batch without the hook gives the oracle's."""
    rng = np.random.default_rng(17)
    left, right = synth.rand_seq(rng, 300), synth.rand_seq(rng, 300)
    ks = (40, 50, 60, 70) if kind == "quanta" else (700, 720)
    reads = [synth.apply_errors(rng, left[-100:] + "TATTG" * k + right[:100], "hifi") for k in ks]
    d = dict(regions=[(left, "TATTG", right)], reads=reads, kmin=np.array([k - 5 for k in ks], np.int32),
             kmax=np.array([k + 5 for k in ks], np.int32), read_region=None)
    if kind == "quanta":
        monkeypatch.setenv("NRA_TEST_QSTEPS", "128")        # several parts a sweep: parts that wait
    monkeypatch.setenv("NRA_TEST_MT_GIVEUP", "1")
    with capi.Batch.create_1d(d["regions"], reads, d["kmin"], d["kmax"]) as b:
        b.run()
        with pytest.raises(capi.NraError) as e:
            b.fetch()
        assert e.value.code == -2 and "timed out" in str(e.value)
        assert ("quanta" in str(e.value)) == (kind == "quanta")
    monkeypatch.delenv("NRA_TEST_MT_GIVEUP")
    (g,), _ = run_batch(capi, d)
    same_as_oracle(g, oracle_1d(oracle, d), False)
    assert (g["status"] == 0).all()


# ------------------------------------------------------------------ column tables at the ends of their blocks
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("ncols", [31, 32, 33, 63, 64, 65, 129])
def test_column_tables_at_block_boundaries(capi, oracle, monkeypatch, ncols, half):
    """Templates that end one column before, on and one column behind a block of 32 (half-wave) or 64 (full-wave) columns:
    the forward template L + unit^5 and the reverse template R have `ncols` columns each, and the tables a block start asks
    for lie outside the template from there on.  Parts of 64 steps: every part starts with a table of its own."""
    monkeypatch.setenv("NRA_TEST_QSTEPS", "64")
    rng = np.random.default_rng(ncols)
    k, unit = 5, "CAG"
    left, right = synth.rand_seq(rng, ncols - 3 * k), synth.rand_seq(rng, ncols)
    reads = [synth.apply_errors(rng, left[i % 5:] + unit * k + right[:ncols - i % 7], "ont_q20") for i in range(7)]
    reads.append(synth.rand_seq(rng, 20) + left + unit * k + right + synth.rand_seq(rng, 20))       # longer than the template
    n = len(reads)
    d = dict(regions=[(left, unit, right)], reads=reads, kmin=np.full(n, k, np.int32), kmax=np.full(n, k, np.int32),
             read_region=None)
    (g,), _ = run_batch(capi, d, flags=0 if half else capi.F_NO_HALF_WAVE)
    same_as_oracle(g, oracle_1d(oracle, d), False)
    assert (g["status"] == 0).any()
