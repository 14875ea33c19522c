"""The taint scheme of the 1D LDS-ring sweeps: a relaxed upper-bound cell over the anchor columns far
from the junction, an exact re-sweep of the read pairs where that bound may have reached a result.  Every result must
equal the exact sweeps over every anchor column (NRA_F_FULL_ANCHORS) and the CPU oracle, bit for bit."""
import numpy as np
import pytest

from nanorepeat_amd import synth

pytestmark = pytest.mark.gpu

KEYS_1D = ("best_score", "sum_k", "n_ties", "status", "cand_score", "cand_tstart", "cand_tend")


def run_batch(capi, d, flags=0, sc_over=None):
    sc = capi.default_scoring(**(sc_over or {}))
    b = capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d.get("read_region"), sc=sc,
                             flags=flags)
    try:
        b.run()
        b.sync()
        out = b.fetch()
        return out, b.resweeps()
    finally:
        b.close()


def same(a, b):
    for k in KEYS_1D:
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0][:8])


def with_env(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def test_config2_full_size_equals_full_anchors(capi):
    d = synth.config2()
    g, rs = run_batch(capi, d)
    f, rs_full = run_batch(capi, d, flags=capi.F_FULL_ANCHORS)
    same(g, f)
    assert rs_full["tasks_total"] == 0
    assert rs["tasks_total"] > 0 and rs["reads_total"] == len(d["reads"])
    print("re-swept", rs)
    assert rs["reads"] <= 0.05 * rs["reads_total"]


@pytest.mark.parametrize("flags", [0, "NO_QUANTA", "NO_HALF_WAVE", "NO_QUANTA|NO_HALF_WAVE"])
@pytest.mark.parametrize("c", [64, 256])
def test_forms_and_margins_agree_with_oracle(capi, oracle, monkeypatch, flags, c):
    fl = 0
    if flags:
        for name in flags.split("|"):
            fl |= getattr(capi, "F_" + name)
    with_env(monkeypatch, NRA_RELAX_C=c)
    fl |= capi.F_TIE_EXTENTS                 # (the extents of every tie, as the one-shot call and the oracle give them)
    d = synth.make_1d(40, "TATTG", (8, 30), "ont", kwin=(0, 42), anchor=600, flank=100, seed=5 + c)
    g, rs = run_batch(capi, d, flags=fl)
    f, _ = run_batch(capi, d, flags=fl | capi.F_FULL_ANCHORS)
    same(g, f)
    o = oracle.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=oracle.default_scoring())
    same(g, o)
    assert rs["tasks_total"] > 0


@pytest.mark.parametrize("qsteps", [128, 384])
@pytest.mark.parametrize("anchor", [900, 700])
def test_quanta_parts_agree(capi, monkeypatch, qsteps, anchor):
    # anchor 900 with c = 128: T = 768, on a part cut; anchor 700: T = 512, inside a 384-step part -- a loaded part then
    # runs relaxed, switches and runs exact
    with_env(monkeypatch, NRA_TEST_QSTEPS=qsteps, NRA_RELAX_C=128)
    d = synth.make_1d(60, "CAG", (5, 41), "ont_q20", kwin=(0, 50), anchor=anchor, flank=80, seed=qsteps)
    g, rs = run_batch(capi, d)
    f, _ = run_batch(capi, d, flags=capi.F_FULL_ANCHORS)
    same(g, f)
    assert rs["tasks_total"] > 0


@pytest.mark.parametrize("c", [64, 200])
def test_quanta_part_straddles_the_switch(capi, monkeypatch, c):
    # parts of 384 steps and T = 640 (c = 64) or 512 (c = 200) for a 740-base anchor: part 1 starts relaxed at step 384,
    # switches to the exact cell inside and runs on
    with_env(monkeypatch, NRA_TEST_QSTEPS=384, NRA_RELAX_C=c)
    d = synth.make_1d(80, "TATTG", (8, 30), "ont", kwin=(0, 40), anchor=740, flank=100, seed=c)
    g, rs = run_batch(capi, d)
    f, _ = run_batch(capi, d, flags=capi.F_FULL_ANCHORS)
    same(g, f)
    assert rs["tasks_total"] > 0


def test_adversarial_anchors_fire_the_resweep(capi, oracle, monkeypatch):
    # anchors that hold the core's flank and a tract of the unit far from the junction, junk reads, reads that reach
    # deep into an anchor, and an anchor shorter than the margin
    rng = np.random.default_rng(7)
    unit = "TATTG"
    flank = 100
    left = synth.rand_seq(rng, 1000)
    right = synth.rand_seq(rng, 1000)
    left = left[:100] + left[-flank:] + unit * 30 + left[100 + flank + 5 * 30:]
    right = right[:flank] + right[flank:500] + right[:flank] + unit * 20 + right[500 + flank + 100:]
    right = right[:1000]
    reads = []
    for i in range(48):
        k = 10 + (i % 20)
        kind = i % 4
        if kind == 0:
            core = left[-flank:] + unit * k + right[:flank]
        elif kind == 1:
            core = synth.rand_seq(rng, 300 + 10 * i)
        elif kind == 2:
            core = left[-700:] + unit * k + right[:700]
        else:
            core = left[-flank:] + unit * k + right[:flank] + right[:400]
        reads.append(synth.apply_errors(rng, core, "ont"))
    short = (left[-150:], unit, right[:150])
    regions = [(left, unit, right), short]
    read_region = np.array([i % 2 if i % 8 == 7 else 0 for i in range(len(reads))], np.int32)
    kmin = np.zeros(len(reads), np.int32)
    kmax = np.full(len(reads), 40, np.int32)
    d = dict(regions=regions, reads=reads, kmin=kmin, kmax=kmax, read_region=read_region)
    with_env(monkeypatch, NRA_RELAX_C=64)
    g, rs = run_batch(capi, d, flags=capi.F_TIE_EXTENTS)
    f, _ = run_batch(capi, d, flags=capi.F_TIE_EXTENTS | capi.F_FULL_ANCHORS)
    same(g, f)
    o = oracle.round3_1d(regions, reads, kmin, kmax, read_region=read_region, sc=oracle.default_scoring())
    same(g, o)
    assert rs["tasks"] > 0, rs


def test_tiny_margin_and_n_bases(capi, monkeypatch):
    with_env(monkeypatch, NRA_RELAX_C=64)
    d = synth.make_1d(30, "GGCCCC", (3, 12), "ont", kwin=(0, 20), anchor=1000, flank=100, seed=3)
    d["reads"] = [r[:40] + "N" * 3 + r[43:] if i % 3 == 0 else r for i, r in enumerate(d["reads"])]
    g, rs = run_batch(capi, d)
    f, _ = run_batch(capi, d, flags=capi.F_FULL_ANCHORS)
    same(g, f)
    assert rs["tasks_total"] > 0


def whole_anchor_reads(rng, left, unit, right, n, k):
    """Reads that cover a whole anchor from its far end: starting at L[0], or ending at R's last base, each with a
    two- to four-base deletion or insertion in the anchor's far columns (where the sweeps run the relaxed cell)."""
    reads = []
    for i in range(n):
        ll, rr = left, right
        at, d = 20 + 7 * i, 2 + i % 3
        if i % 2 == 0:
            ll = ll[:at] + ll[at + d:] if i % 4 == 0 else ll[:at] + synth.rand_seq(rng, d) + ll[at:]
        else:
            j = len(rr) - at
            rr = rr[:j] + rr[j + d:] if i % 4 == 1 else rr[:j] + synth.rand_seq(rng, d) + rr[j:]
        core = (ll if i % 3 != 2 else ll[len(ll) // 2:]) + unit * k + (rr if i % 3 != 1 else rr[:len(rr) // 2])
        reads.append(core if i % 5 else synth.apply_errors(rng, core, "hifi"))
    return reads


@pytest.mark.parametrize("c", [None, 64])
@pytest.mark.parametrize("anchor,unit,k", [(1000, "TATTG", 12), (340, "CAG", 20), (700, "AT", 30)])
def test_reads_covering_a_whole_anchor(capi, oracle, monkeypatch, c, anchor, unit, k):
    # the relaxed cell prices gaps of two or more bases below the exact cell: a read that reaches template column 0
    # (forward) or R's last base (reverse) must come out tainted, be swept again and equal the exact sweeps
    if c is not None:
        with_env(monkeypatch, NRA_RELAX_C=c)
    with_env(monkeypatch, NRA_CHAIN_FROM=3072)      # reads of 1-3 kb in one register block (LDS-ring sweeps), not row blocks
    rng = np.random.default_rng(anchor + (c or 0))
    left, right = synth.rand_seq(rng, anchor), synth.rand_seq(rng, anchor)
    reads = whole_anchor_reads(rng, left, unit, right, 16, k)
    kmin = np.full(len(reads), max(0, k - 6), np.int32)
    kmax = np.full(len(reads), k + 6, np.int32)
    d = dict(regions=[(left, unit, right)], reads=reads, kmin=kmin, kmax=kmax, read_region=None)
    o = oracle.round3_1d(d["regions"], reads, kmin, kmax, sc=oracle.default_scoring())
    for fl in (0, capi.F_NO_QUANTA, capi.F_NO_HALF_WAVE):
        g, rs = run_batch(capi, d, flags=fl | capi.F_TIE_EXTENTS)
        f, _ = run_batch(capi, d, flags=fl | capi.F_TIE_EXTENTS | capi.F_FULL_ANCHORS)
        same(g, f)
        same(g, o)
        if anchor - (c or 256) >= 64:
            assert rs["tasks"] > 0, rs


def test_scoring_outside_the_quadrupled_range_keeps_doubled_cells(capi, oracle):
    # large scores: the doubled cells hold them, the quadrupled ones would not -> today's doubled cells, same results
    d = synth.make_1d(16, "TATTG", (8, 30), "ont", kwin=(0, 40), anchor=600, flank=100, seed=9)
    over = dict(match=24, mismatch=24, gap_open1=24, gap_open2=40)
    g, rs = run_batch(capi, d, flags=capi.F_TIE_EXTENTS, sc_over=over)
    assert rs["tasks_total"] == 0
    f, _ = run_batch(capi, d, flags=capi.F_TIE_EXTENTS | capi.F_FULL_ANCHORS, sc_over=over)
    same(g, f)
    o = oracle.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=oracle.default_scoring(**over))
    same(g, o)
