"""BASELINE configs 3, 4 and 5 at the size and seed bench.py times, against the CPU oracle and against themselves.

At these sizes the planner takes the code paths the benchmark measures and the reduced tests of test_gpu_parity.py do
not: config 5 runs ticketed quanta beside row-block buckets, config 4 runs without quanta, mostly in the half-wave
kernels, and its one-shot call streams region blocks, config 3 runs the packed flank sweeps, kept column states and
round 3 routed on the device.  Per config one run over all reads (module-scoped fixtures), then
  A. a seeded sample of reads, their rows fetched from that run, against the oracle on those reads alone;
  B. every read, bit for bit, between independent code paths of the library;
  C. properties of the whole result that do not depend on its size.
Everything is exact integer equality.  Run with -s to see the wall-time split and the re-swept shares."""
import contextlib
import copy
import time

import numpy as np
import pytest

from nanorepeat_amd import dist as D, joint as J, synth

pytestmark = pytest.mark.gpu

PER_READ_1D = ("best_score", "sum_k", "n_ties", "status")
KEYS_1D = PER_READ_1D + ("cand_score", "cand_tstart", "cand_tend")
PER_READ_2D = ("read_strand", "best_wscore", "sum_k1", "sum_k2", "n_ties", "status")
N_ALIGNMENTS_CONFIG4 = 30_834_667          # sum(kmax - kmin + 1) of config4(1000, 1000) at the default seed


@contextlib.contextmanager
def clock(what):
    t0 = time.perf_counter()
    yield
    print(f"[full size] {what}: {time.perf_counter() - t0:.1f} s")


def cand_offsets(d):
    """Start of every read's candidates in the per-candidate arrays (n + 1 entries)."""
    return np.r_[0, np.cumsum(np.maximum(d["kmax"].astype(np.int64) - d["kmin"] + 1, 0))]


def cand_rows(off, reads):
    """Per-candidate positions of `reads` (in that order) and the read each one belongs to."""
    reads = np.asarray(reads, np.int64)
    n = off[reads + 1] - off[reads]
    owner = np.repeat(reads, n)
    within = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    return off[owner] + within, owner


def assert_equal_rows(got, want, what, key, owner):
    """got == want element by element; a difference names the read (owner[i] = read of element i)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, key, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {key} differs in {len(bad)} of {len(got)} entries, first at read {int(owner[i])} "
                             f"(entry {i}): {got[i]} != {want[i]}")


def assert_same_1d(a, b, what, d, keys=KEYS_1D, rows_a=None):
    """Results a and b of 1D runs are equal on `keys`.  rows_a: the reads of a (the run over the workload d) that b holds,
    in b's order (default: all of them)."""
    ra = np.arange(len(a["status"])) if rows_a is None else np.asarray(rows_a)
    idx = None
    for k in keys:
        if k.startswith("cand_"):
            if idx is None:
                idx, owner = cand_rows(cand_offsets(d), ra)
            assert_equal_rows(a[k][idx], b[k], what, k, owner)
        else:
            assert_equal_rows(a[k][ra], b[k], what, k, ra)


def run_resident_1d(capi, d, flags=0):
    with capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d.get("read_region"),
                              flags=flags) as b:
        b.run(); b.sync()
        return b.fetch(), b.stats(), b.resweeps()


def oracle_sample_1d(oracle, d, g, pick, what):
    """Section A, 1D: the rows of the reads `pick` of the full-size result g against the oracle on those reads alone."""
    rr = d.get("read_region")
    with clock(f"{what}: oracle on {len(pick)} reads"):
        o = oracle.round3_1d(d["regions"], [d["reads"][i] for i in pick], d["kmin"][pick], d["kmax"][pick],
                             read_region=None if rr is None else rr[pick])
    for k in PER_READ_1D:
        assert_equal_rows(g[k][pick], o[k], what, k, pick)
    idx, owner = cand_rows(cand_offsets(d), pick)
    assert_equal_rows(g["cand_score"][idx], o["cand_score"], what, "cand_score", owner)
    ties = o["cand_tstart"] >= 0
    assert ties.any()
    for k in ("cand_tstart", "cand_tend"):
        assert_equal_rows(g[k][idx][ties], o[k][ties], what, k, owner[ties])
    return o


def properties_1d(d, g, st, n_alignments, ok_share, near_share):
    """Section C, 1D (the batch ran with F_TIE_EXTENTS)."""
    n = len(d["reads"])
    assert st["n_alignments"] == n_alignments == len(g["cand_score"])
    for k in PER_READ_1D:
        assert len(g[k]) == n
    # every read has a record; nearly all of them the decomposition's own
    assert (g["status"] <= 1).all()
    ok = g["status"] == 0
    assert ok.mean() > ok_share and np.array_equal(g["n_ties"] >= 1, ok)
    est = g["sum_k"][ok] / g["n_ties"][ok]
    assert (est >= d["kmin"][ok]).all() and (est <= d["kmax"][ok]).all()
    assert np.mean(np.abs(est - d["k_true"][ok]) <= 1) > near_share
    qlen = np.fromiter(map(len, d["reads"]), np.int64, n)
    assert (g["best_score"] <= 2 * qlen).all()
    # a read's best score is the largest of its candidates', and the extents are there exactly for its ties
    off = cand_offsets(d)
    assert (np.diff(off) > 0).all()
    assert np.array_equal(np.maximum.reduceat(g["cand_score"], off[:-1]), g["best_score"])
    ties = g["cand_score"] == np.repeat(g["best_score"], np.diff(off))
    assert np.array_equal(g["cand_tstart"] >= 0, ties)
    assert (np.add.reduceat(ties.astype(np.int64), off[:-1]) >= g["n_ties"]).all()      # (the ties that pass the flank test)
    assert (g["cand_tend"][ties] > g["cand_tstart"][ties]).all()


def resweep_share(rs, what):
    share = rs["reads"] / max(rs["reads_total"], 1)
    print(f"[full size] {what}: re-swept {rs['reads']} of {rs['reads_total']} reads ({100 * share:.2f} %), "
          f"{rs['tasks']} of {rs['tasks_total']} sweep tasks")
    return share


# ------------------------------------------------------------------ config 5: 10 000 reads, K = 496
@pytest.fixture(scope="module")
def config5_run(capi):
    with clock("config 5: generate"):
        d = synth.config5(n_reads=10000, seed=synth.SEED)
    with clock("config 5: resident run"):
        g, st, rs = run_resident_1d(capi, d, flags=capi.F_TIE_EXTENTS)
    return d, g, st, rs


def test_config5_oracle_sample(oracle, config5_run):
    d, g, _, _ = config5_run
    rng = np.random.default_rng(1)
    pick = np.concatenate([rng.choice(np.nonzero(d["k_true"] == a)[0], 8, replace=False) for a in (60, 420)])
    qlen = np.array([len(d["reads"][i]) for i in pick])
    assert qlen[:8].max() < 768 and qlen[8:].min() > 2048           # the half-wave class and the row-block class
    oracle_sample_1d(oracle, d, g, pick, "config 5")


def test_config5_properties(config5_run):
    d, g, st, _ = config5_run
    properties_1d(d, g, st, len(d["reads"]) * 496, ok_share=0.98, near_share=0.95)


def test_config5_relaxed_equals_full_anchors(capi, config5_run):
    d, g, _, rs = config5_run
    f, _, rs_full = run_resident_1d(capi, d, flags=capi.F_TIE_EXTENTS | capi.F_FULL_ANCHORS)
    assert_same_1d(g, f, "config 5, relaxed against full anchors", d)
    # (the relaxed cells are the LDS-ring sweeps': the 2.3 kb reads in row blocks run the exact cell and do not count)
    assert rs["tasks_total"] > 0 and 0 < rs["reads_total"] <= len(d["reads"]) and rs_full["tasks_total"] == 0
    resweep_share(rs, "config 5")               # (reported, not asserted: nobody has set a figure for config 5)


def test_config5_forms_of_the_sweeps_agree(capi, config5_run, monkeypatch):
    """Quanta beside row blocks (the default) against two launches per bucket, and against the 2.3 kb reads in one register
    block of 40 rows per lane: F_SERIAL_CHAIN and NRA_CHAIN_FROM=3072 both do that to reads of up to 3072 rows (the flag
    takes every read out of the concurrent row blocks; longer reads, of which config 5 has none, would run their blocks
    one after the other)."""
    d, g, st, _ = config5_run
    keys = PER_READ_1D + ("cand_score",)
    f, st_f, _ = run_resident_1d(capi, d, flags=capi.F_NO_QUANTA)
    assert_same_1d(g, f, "config 5, quanta against two launches", d, keys)
    # the same cells in another launch shape: executed_cells cannot tell the forms apart, the wave states the quanta
    # park at their cuts (intermediate_bytes) can
    assert st_f["executed_cells"] == st["executed_cells"] and st_f["intermediate_bytes"] < st["intermediate_bytes"]
    f, st_f, _ = run_resident_1d(capi, d, flags=capi.F_SERIAL_CHAIN)
    assert_same_1d(g, f, "config 5, F_SERIAL_CHAIN", d, keys)
    assert st_f["executed_cells"] != st["executed_cells"]
    monkeypatch.setenv("NRA_CHAIN_FROM", "3072")
    f, st_f, _ = run_resident_1d(capi, d)
    assert_same_1d(g, f, "config 5, NRA_CHAIN_FROM=3072", d, keys)
    assert st_f["executed_cells"] != st["executed_cells"]


def test_config5_order_and_batching_invariance(capi, config5_run):
    d, g, _, _ = config5_run
    perm = np.random.default_rng(2).permutation(len(d["reads"]))[:3000]
    sub = capi.round3_1d(d["regions"], [d["reads"][i] for i in perm], d["kmin"][perm], d["kmax"][perm], per_candidate=False)
    assert_same_1d(g, sub, "config 5, a shuffled 3000-read subset in one call", d, PER_READ_1D, rows_a=perm)


# ------------------------------------------------------------------ config 4: 1000 regions x 1000 reads
@pytest.fixture(scope="module")
def config4_run(capi):
    with clock("config 4: generate"):
        d = synth.config4(1000, 1000, seed=synth.SEED)
    with clock("config 4: resident run"):
        g, st, rs = run_resident_1d(capi, d, flags=capi.F_TIE_EXTENTS)
    return d, g, st, rs


def test_config4_oracle_sample(oracle, config4_run):
    d, g, _, _ = config4_run
    rng = np.random.default_rng(1)
    regions = np.arange(0, 1000, 10)
    pick = np.concatenate([r * 1000 + np.sort(rng.choice(1000, 2, replace=False)) for r in regions])
    assert np.array_equal(d["read_region"][pick], np.repeat(regions, 2))
    assert {len(d["regions"][r][1]) for r in regions} == {3, 4, 5, 6}
    oracle_sample_1d(oracle, d, g, pick, "config 4")


def test_config4_properties(config4_run):
    d, g, st, _ = config4_run
    assert int((d["kmax"].astype(np.int64) - d["kmin"] + 1).sum()) == N_ALIGNMENTS_CONFIG4
    properties_1d(d, g, st, N_ALIGNMENTS_CONFIG4, ok_share=0.95, near_share=0.95)


def test_config4_relaxed_equals_full_anchors(capi, config4_run):
    d, g, _, rs = config4_run
    f, _, rs_full = run_resident_1d(capi, d, flags=capi.F_TIE_EXTENTS | capi.F_FULL_ANCHORS)
    assert_same_1d(g, f, "config 4, relaxed against full anchors", d)
    assert rs["tasks_total"] > 0 and 0 < rs["reads_total"] <= len(d["reads"]) and rs_full["tasks_total"] == 0
    resweep_share(rs, "config 4")               # (reported, not asserted: nobody has set a figure for config 4)


def test_config4_resident_equals_the_streamed_call(capi, config4_run):
    d, g, _, _ = config4_run
    with clock("config 4: one-shot call"):
        one = capi.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d["read_region"])
    assert_same_1d(g, one, "config 4, resident batch against the one-shot call", d)


def test_config4_one_shard_of_eight(capi, config4_run):
    """What rank 3 of an 8-GPU run computes: its regions by the cost model, materialised on their own, run alone."""
    d, g, _, _ = config4_run
    cost = np.array([synth.config4_region_cost(synth.config4_region(r), 1000) for r in range(1000)], np.int64)
    owner = D.lpt_assign(cost, 8)
    assert np.bincount(owner, minlength=8).min() > 0
    mine = np.nonzero(owner == 3)[0]
    with clock(f"config 4: generate the {len(mine)} regions of rank 3"):
        s = synth.config4(1000, 1000, seed=synth.SEED, only=mine)
    rid = s["read_id"]
    assert np.array_equal(s["region_id"], mine) and len(rid) == 1000 * len(mine)
    assert all(s["reads"][i] == d["reads"][rid[i]] for i in range(0, len(rid), 997))
    assert np.array_equal(s["kmin"], d["kmin"][rid]) and np.array_equal(s["kmax"], d["kmax"][rid])
    gs, st, _ = run_resident_1d(capi, s, flags=capi.F_TIE_EXTENTS)
    assert st["n_alignments"] == int((s["kmax"].astype(np.int64) - s["kmin"] + 1).sum())
    assert_same_1d(g, gs, "config 4, the full run against rank 3's shard", d, rows_a=rid)


def test_config4_order_invariance(capi, config4_run):
    d, g, _, _ = config4_run
    perm = np.random.default_rng(4).permutation(len(d["reads"]))
    got = capi.round3_1d(d["regions"], [d["reads"][i] for i in perm], d["kmin"][perm], d["kmax"][perm],
                         read_region=d["read_region"][perm], per_candidate=False)
    assert_same_1d(g, got, "config 4, all reads shuffled across regions", d, PER_READ_1D, rows_a=perm)


# ------------------------------------------------------------------ config 3: 5000 joint reads, both grid rounds
class RecordingSession(J.GridSession):
    """A one-group GridSession that keeps what every round saw and gave: the grid, the strands, the per-read rows, and the
    per-cell arrays of a round that ran as a grid of its own (a refinement lays its cells out per read)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        assert not self.subs
        self.seen = []

    def score_grid(self, grid, read_strand, refine=None):
        out, n_cells = super().score_grid(grid, read_strand, refine)
        cells = out if self.scorer is not None else None
        if self.scorer is None and out is not None and not self.refined:
            cells = self.batch.fetch(per_candidate=True)
        self.seen.append(dict(grid=grid, out=out, cells=cells, refined=self.refined,
                              stats=None if self.batch is None else self.batch.stats()))
        return out, n_cells


def config3_inputs(n=5000):
    """The joint workload as bench.py sets it up."""
    j = synth.config3(n)
    init, fq = J.Round1Estimation(), {}
    for i, s in enumerate(j["reads"]):
        init.repeat1_count_range_dict[f"r{i}"] = tuple(int(x) for x in j["range1"][i])
        init.repeat2_count_range_dict[f"r{i}"] = tuple(int(x) for x in j["range2"][i])
        init.read_strand_dict[f"r{i}"] = int(j["strand"][i])
        fq[f"r{i}"] = f"@r{i}\n{s}\n+\n{'!' * len(s)}\n"
    left, u1, mid, u2, right = j["region"]
    chrom = left + u1 * 19 + mid + u2 * 7 + right
    a = J.Repeat.parse(f"chr4:{len(left)}:{len(left) + 57}:{u1}:200")
    b = J.Repeat.parse(f"chr4:{len(left) + 57 + len(mid)}:{len(left) + 57 + len(mid) + 21}:{u2}:20")
    a.max_size += 10; b.max_size += 10
    return dict(j=j, init=init, fq=fq, chrom=chrom, a=a, b=b, region=J._joint_region(chrom, a, b))


def both_rounds(w, session, fq=None, **kw):
    session.new_run()
    return J.fine_tune_read_count(w["init"], fq or w["fq"], w["chrom"], copy.copy(w["a"]), copy.copy(w["b"]),
                                  session=session, **kw)


def sizes(est):
    return ({k: float(v) for k, v in est.repeat1_count_dict.items()}, {k: float(v) for k, v in est.repeat2_count_dict.items()})


@pytest.fixture(scope="module")
def config3_run(capi):
    with clock("config 3: generate"):
        w = config3_inputs()
    with clock("config 3: device-routed run, a second pass, two-grid-call run"):
        with RecordingSession(w["region"], w["fq"]) as sess:
            routed = both_rounds(w, sess)
            w["routed"] = dict(sizes=sizes(routed), refined=bool(getattr(routed, "refined", False)),
                               steps=(routed.step_size1, routed.step_size2), seen=sess.seen)
            sess.seen = []
            w["second_pass"] = sizes(both_rounds(w, sess))          # what a benchmark step does
        with RecordingSession(w["region"], w["fq"]) as sess:
            two = both_rounds(w, sess, refine=False)
            w["two_calls"] = dict(sizes=sizes(two), refined=bool(getattr(two, "refined", False)),
                                  steps=(two.step_size1, two.step_size2), seen=sess.seen)
    return w


def config3_sample(w):
    j = w["j"]
    pick = np.sort(np.random.default_rng(1).choice(len(j["reads"]), 100, replace=False))
    assert set(j["strand"][pick].tolist()) == {1, -1}
    assert {tuple(t) for t in j["truth"][pick].tolist()} == {(17, 10), (55, 7)}
    return pick, [f"r{i}" for i in pick]


def test_config3_oracle_sample_through_both_rounds(capi, oracle, config3_run):
    w = config3_run
    pick, names = config3_sample(w)
    fq = {name: w["fq"][name] for name in names}
    with clock("config 3: oracle on 100 reads through both rounds"):
        # the round-1 ranges of ALL reads: spans and step sizes come from all of them
        with RecordingSession(w["region"], fq, scorer=oracle.joint_2d) as osess:
            want = both_rounds(w, osess, fq=fq, scorer=oracle.joint_2d)
    routed, two = w["routed"], w["two_calls"]
    assert routed["refined"] and not two["refined"]                 # round 3 really was routed on the device
    assert len(routed["seen"]) == 1 and len(two["seen"]) == 2 and len(osess.seen) == 2
    # the same steps in all three runs: the coarse grid's, from all 5000 ranges, and (1, 1) at the end
    steps = (J.choose_best_step_size(w["a"], w["init"].repeat1_count_range_dict),
             J.choose_best_step_size(w["b"], w["init"].repeat2_count_range_dict))
    assert min(steps) > 1
    for seen in (routed["seen"], two["seen"], osess.seen):
        assert (seen[0]["grid"].axes[0][1], seen[0]["grid"].axes[1][1]) == steps
    assert routed["steps"] == two["steps"] == (want.step_size1, want.step_size2) == (1, 1)
    # the sizes of the product run over all 5000 reads, at the sampled reads, against the oracle's
    want_sizes = sizes(want)
    for axis in (0, 1):
        assert set(want_sizes[axis]) <= set(names)
        for name in names:
            assert routed["sizes"][axis].get(name) == want_sizes[axis].get(name), ("size", axis + 1, name)
    # per-read rows: the refinement's and the two grid calls' against the oracle's rounds
    for what, got, o in (("routed, final", routed["seen"][0]["out"], osess.seen[1]["out"]),
                         ("two calls, round 2", two["seen"][0]["out"], osess.seen[0]["out"]),
                         ("two calls, round 3", two["seen"][1]["out"], osess.seen[1]["out"])):
        for k in PER_READ_2D:
            assert_equal_rows(np.asarray(got[k])[pick], o[k], "config 3, " + what, k, pick)
    # per-cell arrays of both grid calls, fetched from the resident full-size batch, against the oracle on the same cells
    for r in (0, 1):
        cr, k1, k2 = capi.joint_grid_cells(two["seen"][r]["grid"])
        mine = np.isin(cr, pick)
        ocr, ok1, ok2 = capi.joint_grid_cells(osess.seen[r]["grid"])
        assert mine.sum() > 0 and np.array_equal(cr[mine], pick[ocr])
        assert np.array_equal(k1[mine], ok1) and np.array_equal(k2[mine], ok2)
        for k in ("cell_score", "cell_wscore"):
            assert len(two["seen"][r]["cells"][k]) == len(cr)
            assert_equal_rows(two["seen"][r]["cells"][k][mine], osess.seen[r]["cells"][k],
                              f"config 3, two calls, round {r + 2}", k, cr[mine])


def test_config3_forms_of_the_rounds_agree(capi, config3_run):
    """Device-routed round 3 == two grid calls == a session that sweeps round 3 again == two read groups in host threads,
    and a second pass on the same resident session: both size dicts of all 5000 reads."""
    w = config3_run
    base = w["routed"]["sizes"]
    assert w["routed"]["refined"]
    assert w["two_calls"]["sizes"] == base
    assert w["second_pass"] == base
    with J.GridSession(w["region"], w["fq"], flags=capi.F_JOINT_NO_KEEP) as sess:
        assert sizes(both_rounds(w, sess)) == base
    with J.GridSession(w["region"], w["fq"], parts=2) as sess:
        assert len(sess.subs) == 2
        got = sizes(both_rounds(w, sess))
        assert got == base and list(got[0]) == list(base[0])


def test_config3_properties(capi, config3_run):
    w = config3_run
    j, routed, two = w["j"], w["routed"], w["two_calls"]
    n = len(j["reads"])
    # every round scored the cells of its grid; the device-routed run both rounds' cells
    counts = []
    for seen in two["seen"]:
        counts.append(len(capi.joint_grid_cells(seen["grid"])[0]))
        assert seen["stats"]["n_alignments"] == counts[-1] == len(seen["cells"]["cell_score"])
    assert routed["seen"][0]["stats"]["n_alignments"] == sum(counts)
    out = routed["seen"][0]["out"]
    for k in PER_READ_2D:
        assert len(out[k]) == n
    assert np.array_equal(out["read_strand"], j["strand"])          # round 1's strands are kept
    ok = (out["status"] == capi.READ_OK) & (out["n_ties"] > 0)
    assert (out["status"] <= capi.READ_NO_RECORD).all() and ok.mean() > 0.98
    names = [f"r{i}" for i in np.nonzero(ok)[0]]
    assert list(routed["sizes"][0]) == names and list(routed["sizes"][1]) == names
    k1 = out["sum_k1"][ok] / out["n_ties"][ok]
    k2 = out["sum_k2"][ok] / out["n_ties"][ok]
    assert np.array_equal(k1, np.array([routed["sizes"][0][x] for x in names]))
    # estimates inside the read's round-1 ranges [lo, hi)
    assert (k1 >= j["range1"][ok, 0]).all() and (k1 <= j["range1"][ok, 1] - 1).all()
    assert (k2 >= j["range2"][ok, 0]).all() and (k2 <= j["range2"][ok, 1] - 1).all()
    assert np.mean(np.abs(k1 - j["truth"][ok, 0]) <= 1) >= 0.8 and np.mean(np.abs(k2 - j["truth"][ok, 1]) <= 1) >= 0.8
    qlen = np.fromiter(map(len, j["reads"]), np.int64, n)
    for seen in two["seen"]:
        cr = capi.joint_grid_cells(seen["grid"])[0]
        assert (seen["cells"]["cell_score"] <= 2 * qlen[cr]).all()
        best = np.full(n, np.iinfo(np.int32).min, np.int64)
        np.maximum.at(best, cr, seen["cells"]["cell_wscore"])
        has = np.zeros(n, bool); has[cr] = True
        scored = has & (np.asarray(seen["out"]["status"]) == capi.READ_OK)
        assert np.array_equal(best[scored], np.asarray(seen["out"]["best_wscore"])[scored])
