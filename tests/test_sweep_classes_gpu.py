"""Every rows-per-lane class of NRA_R_LIST through every form of the 1D and 2D sweep kernels, at the class's borders, with
and without N, bit for bit against the oracle (integer DP: nothing here has a tolerance).  The batches and forms are those
of tests/sweep_class_cases.py; tests/test_sweep_classes_cpu.py proves from the plans that each (form, class, N) runs as
one bucket of exactly that class and form, so a mismatch here names the instantiation that is wrong."""
import numpy as np
import pytest

import sweep_class_cases as S

pytestmark = pytest.mark.gpu

KEYS_1D = ("best_score", "sum_k", "n_ties", "status", "cand_score")
KEYS_2D = ("read_strand", "cell_score", "cell_wscore", "best_wscore", "sum_k1", "sum_k2", "n_ties", "status")
FORMS_1D, FORMS_2D = S.forms_1d(), S.forms_2d()


def _same(g, o, keys, what, sel=None):
    for k in keys:
        a, b = np.asarray(g[k]), np.asarray(o[k])
        if sel is not None and len(b) == len(sel):
            a, b = a[sel], b[sel]
        assert np.array_equal(a, b), (what, k, np.nonzero(a != b)[0][:8].tolist(), a[:12].tolist(), b[:12].tolist())


@pytest.mark.parametrize("R", S.r_list())
def test_1d_sweeps_of_one_class_in_all_forms(capi, oracle, monkeypatch, R):
    for unit in (64, 32):
        if unit == 32 and R > S.RING32_MAX_R:
            continue                                   # no half-wave kernel (test_sweep_classes_cpu states the census)
        for with_n in (False, True):
            d = S.batch_1d(R, unit, with_n)
            # one oracle run per batch, with the extents of every candidate; the ties are the candidates of a read's best score
            o = oracle.round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=oracle.default_scoring(**d["sc"]),
                                 flags=capi.F_ALL_EXTENTS)
            owner = np.repeat(np.arange(len(d["reads"])), d["kmax"] - d["kmin"] + 1)
            ties = (o["cand_score"] >= 0) & (o["cand_score"] == o["best_score"][owner])
            assert ties.any() and (o["cand_tstart"][ties] >= 0).all()
            for name, f in FORMS_1D.items():
                if f["unit"] != unit:
                    continue
                what = (name, R, "N" if with_n else "-")
                for k in S.KNOBS:
                    monkeypatch.delenv(k, raising=False)
                for k, v in S.env_of(f, R).items():
                    monkeypatch.setenv(k, v)
                with capi.Batch.create_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=capi.default_scoring(**d["sc"]),
                                          flags=f["flags"]) as b:
                    b.run(); b.sync()
                    g = b.fetch()
                    if f["ring_form"]:                 # the quanta keep wave state between parts: a second run, the same bits
                        b.run(); b.sync()
                        again = b.fetch()
                        _same(again, g, list(g), what + ("second run",))
                _same(g, o, KEYS_1D, what)
                if f["extents"]:
                    sel = ties if f["extents"] == "ties" else slice(None)
                    assert np.array_equal(g["cand_tstart"][sel], o["cand_tstart"][sel]), what
                    assert np.array_equal(g["cand_tend"][sel], o["cand_tend"][sel]), what
    for k in S.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("R", S.r_list())
def test_2d_sweeps_of_one_class_in_all_forms(capi, oracle, R):
    for with_n in (False, True):
        j = S.batch_2d(R, with_n)
        n = len(j["reads"])
        cells, coarse, bounds, (s1, s2) = S.grids_2d(j)
        cr, k1, k2 = capi.joint_grid_cells(cells)
        osc, gsc = oracle.default_scoring(**j["sc"]), capi.default_scoring(**j["sc"])
        has = np.zeros(n, bool); has[cr] = True
        assert has.all()
        want = {True: oracle.joint_2d(j["region"], j["reads"], cr, k1, k2, read_strand=j["strand"], sc=osc),
                False: oracle.joint_2d(j["region"], j["reads"], cr, k1, k2, sc=osc)}
        for name, f in FORMS_2D.items():
            what = (name, R, "N" if with_n else "-")
            st = j["strand"] if f["given"] else None
            with capi.Batch.create_2d_reads(j["region"], j["reads"], sc=gsc, flags=f["flags"]) as b:
                if f["refine"]:
                    # the refinement behind the coarse grid against the oracle on the finer grid that the oracle's own
                    # coarse sizes route (max(size - s, lo) <= k < min(size + s, hi), as nra_batch2d_refine does)
                    ccr, ck1, ck2 = capi.joint_grid_cells(coarse)
                    oc = oracle.joint_2d(j["region"], j["reads"], ccr, ck1, ck2, read_strand=st, sc=osc)
                    ok = (oc["status"] == 0) & (oc["n_ties"] > 0)
                    nt = np.maximum(oc["n_ties"], 1).astype(np.float64)
                    z1, z2 = oc["sum_k1"] / nt, oc["sum_k2"] / nt
                    lo1, hi1, lo2, hi2 = bounds
                    fb = [np.where(ok, v, 0.0) for v in (np.maximum(z1 - s1, lo1), np.minimum(z1 + s1, hi1),
                                                          np.maximum(z2 - s2, lo2), np.minimum(z2 + s2, hi2))]
                    fine = capi.Grid(cells.axes[0], fb[0], fb[1], cells.axes[1], fb[2], fb[3])
                    fcr, fk1, fk2 = capi.joint_grid_cells(fine)
                    of = oracle.joint_2d(j["region"], j["reads"], fcr, fk1, fk2, read_strand=st, sc=osc)
                    hasf = np.zeros(n, bool); hasf[fcr] = True
                    assert hasf.sum() >= 3
                    assert b.set_grid(coarse, st) == len(ccr)
                    b.run()
                    assert b.refine(s1, s2, lo1, hi1, lo2, hi2), what
                    b.sync()
                    g = b.fetch()
                    _same(g, of, ("best_wscore", "sum_k1", "sum_k2", "n_ties", "status"), what, hasf)
                    assert (g["status"][~hasf] == 2).all(), what
                    cap = 4 * s1 * s2
                    cs, cw = g["cell_score"].reshape(n, cap), g["cell_wscore"].reshape(n, cap)
                    for r in np.nonzero(hasf)[0]:
                        mine = np.nonzero(fcr == r)[0]
                        assert np.array_equal(cs[r, :len(mine)], of["cell_score"][mine]), what + (int(r),)
                        assert np.array_equal(cw[r, :len(mine)], of["cell_wscore"][mine]), what + (int(r),)
                        assert (cs[r, len(mine):] == -1).all(), what
                    # ... and the coarse grid itself, run again from the states it kept
                    b.run(); b.sync()
                    _same(b.fetch(), oc, KEYS_2D, what + ("coarse",))
                    continue
                if f["grid"]:
                    assert b.set_grid(cells, st) == len(cr)
                else:
                    b.set_cells(cr, k1, k2, st)
                b.run(); b.sync()
                _same(b.fetch(), want[f["given"]], KEYS_2D, what)
