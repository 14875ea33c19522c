"""The censored allele fit on the GPU: k_censored_fit (nra_censored_fit) against the numpy restatement on the fit panel
(N at the lane and register-class borders, m from 1 to N, orders 1..4, open 0 and 1, three starts), the streaming form
against the register form bit for bit, fits permuted in the batch and alone, bounds 45 sd either side of every mean,
k_censored_resp (nra_censored_posteriors), the argument errors, and the BAM command end to end.
Continuous outputs (ll, w, nu): the largest relative difference from the restatement measured on the fit panel on one
MI355X is recorded in DESIGN.md section 26; TOLERANCE is 100 times it, capped at 1e-6."""
import sys

import numpy as np
import pytest

import censored_ref as REF
import censored_cases as K

pytestmark = pytest.mark.gpu

MEASURED = 6.425e-12                           # largest relative difference on the fit panel, one MI355X
TOLERANCE = min(100 * MEASURED, 1e-6)
FIT_KEYS = ("values", "prob_off", "prob_n", "prob_n_exact", "prob_tau", "fit_problem", "fit_n", "fit_open", "starts")


def _rel(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


@pytest.fixture(scope="module")
def panel():
    fp = K.fit_panel()
    return fp, REF.censored_fit(**fp)


@pytest.fixture(scope="module")
def on_device(capi, panel):
    return capi.censored_fit(**panel[0])


def _same_bits(a, b, fits_a, fits_b):
    """Fit fits_a[i] of result a and fit fits_b[i] of result b are the same bits."""
    for fa, fb in zip(fits_a, fits_b):
        assert a["ll"][fa].tobytes() == b["ll"][fb].tobytes(), (fa, fb)
        assert (a["n_iter"][fa], a["converged"][fa]) == (b["n_iter"][fb], b["converged"][fb]), (fa, fb)
        for key, off in (("nu", "nu_off"), ("w", "w_off")):
            assert a[key][a[off][fa]:a[off][fa + 1]].tobytes() == b[key][b[off][fb]:b[off][fb + 1]].tobytes(), (key, fa, fb)


def _subset(fp, fits):
    """The arguments of the fits `fits` (in that order) of the panel, all problems kept."""
    nu_off = np.concatenate([[0], np.cumsum(fp["fit_n"])])
    out = {k: fp[k] for k in FIT_KEYS[:5]}
    out["fit_problem"], out["fit_n"], out["fit_open"] = (fp[k][fits] for k in ("fit_problem", "fit_n", "fit_open"))
    out["starts"] = np.concatenate([fp["starts"][nu_off[f]:nu_off[f + 1]] for f in fits])
    return out


def test_device_equals_restatement(panel, on_device):
    fp, ref = panel
    got = on_device
    nf = len(fp["fit_n"])
    assert np.array_equal(got["nu_off"], ref["nu_off"]) and np.array_equal(got["w_off"], ref["w_off"])
    assert np.array_equal(got["converged"], ref["converged"])
    other = np.flatnonzero(got["n_iter"] != ref["n_iter"])
    capped = np.flatnonzero(ref["converged"] == 0)
    print(f"censored fit panel: {nf} fits, {len(capped)} at the 500-step cap, {len(other)} differ in n_iter")
    assert len(other) <= nf // 100, (other, got["n_iter"][other], ref["n_iter"][other])
    assert (ref["n_iter"][capped] == 500).all() and (got["n_iter"][capped] == 500).all()
    worst = _rel(got["ll"], ref["ll"])
    for f in range(nf):
        if ref["converged"][f] and got["n_iter"][f] == ref["n_iter"][f]:
            for key, off in (("nu", "nu_off"), ("w", "w_off")):
                sl = slice(ref[off][f], ref[off][f + 1])
                worst = max(worst, _rel(got[key][sl], ref[key][sl]))
    print(f"censored fit panel: largest relative difference of ll, w, nu: {worst:.3e}")
    assert np.isfinite(got["ll"]).all() and np.isfinite(got["w"]).all() and np.isfinite(got["nu"]).all()
    assert worst <= TOLERANCE, worst


def test_streamed_equals_register_path_bit_for_bit(capi, panel, on_device):
    fp, _ = panel
    small = np.flatnonzero(fp["prob_n"][fp["fit_problem"]] <= 512)
    assert 0 < len(small) < len(fp["fit_n"])
    streamed = capi.censored_fit(**_subset(fp, small), flags=capi.CENS_F_STREAM)
    _same_bits(on_device, streamed, small, range(len(small)))


def test_a_fit_does_not_depend_on_its_place_in_the_batch(capi, panel, on_device):
    fp, _ = panel
    perm = np.random.default_rng(3).permutation(len(fp["fit_n"]))
    _same_bits(on_device, capi.censored_fit(**_subset(fp, perm)), perm, range(len(perm)))
    for f in (0, int(np.flatnonzero(fp["prob_n"][fp["fit_problem"]] == 513)[0]), len(fp["fit_n"]) - 1):
        _same_bits(on_device, capi.censored_fit(**_subset(fp, [f])), [f], [0])


def test_bounds_45_sd_either_side_of_every_mean(capi):
    tau, nu = 0.07, [3.0, 4.0, 5.5]
    y = [3.0, 3.05, 4.0, 5.5, 5.45] + [nu[0] - 45 * tau, nu[-1] + 45 * tau, 4.2]
    prob = dict(values=y, prob_off=[0], prob_n=[len(y)], prob_n_exact=[5], prob_tau=[tau])
    for o in (0, 1):
        fit = dict(fit_problem=[0], fit_n=[3], fit_open=[o], starts=nu, max_iter=1)
        got, ref = capi.censored_fit(**prob, **fit), REF.censored_fit(**prob, **fit)
        assert np.isfinite(got["ll"]).all() and _rel(got["ll"], ref["ll"]) <= TOLERANCE
        w = [0.2, 0.3, 0.5] if o == 0 else [0.2, 0.3, 0.4, 0.1]
        model = dict(model_n=[3], model_open=[o], w=w, nu=nu)
        rg, rr = capi.censored_posteriors(**prob, **model)[0], REF.censored_posteriors(**prob, **model)[0]
        assert np.isfinite(rg).all() and np.abs(rg - rr).max() <= 1e-9, np.abs(rg - rr).max()
        assert np.abs(rg.sum(axis=1) - 1.0).max() <= 1e-12
        assert np.abs(rg[5, :3] - w[:3] / np.sum(w)).max() < 1e-12          # a bound far below says nothing
        if o:
            assert rg[6, 3] > 1 - 1e-12                                      # a bound far above every mean: the open allele


def test_posteriors(capi, panel, on_device):
    fp, _ = panel
    first = {}
    for f, p in enumerate(fp["fit_problem"]):
        first.setdefault(int(p), f)
    fits = [first[p] for p in range(len(fp["prob_n"]))]
    n, o = fp["fit_n"][fits], fp["fit_open"][fits]
    w = np.concatenate([on_device["w"][on_device["w_off"][f]:on_device["w_off"][f + 1]] for f in fits])
    nu = np.concatenate([on_device["nu"][on_device["nu_off"][f]:on_device["nu_off"][f + 1]] for f in fits])
    args = dict(values=fp["values"], prob_off=fp["prob_off"], prob_n=fp["prob_n"], prob_n_exact=fp["prob_n_exact"],
                prob_tau=fp["prob_tau"], model_n=n, model_open=o, w=w, nu=nu)
    got, ref = capi.censored_posteriors(**args), REF.censored_posteriors(**args)
    assert o.any() and not o.all()
    for p, (g, r) in enumerate(zip(got, ref)):
        m = int(fp["prob_n_exact"][p])
        assert g.shape == r.shape == (fp["prob_n"][p], n[p] + o[p])
        assert np.abs(g.sum(axis=1) - 1.0).max() <= 1e-12 and (g >= 0).all()
        if o[p]:
            assert (g[:m, -1] == 0).all()
        assert np.abs(g - r).max() <= 1e-9, (p, np.abs(g - r).max())


def test_argument_errors_come_before_the_device(capi):
    from test_censored_cpu import fit_argument_errors
    assert len(list(fit_argument_errors(capi, device=99))) == 27
    good = dict(values=[1.0, 2.0, 3.0], prob_off=[0], prob_n=[3], prob_n_exact=[2], prob_tau=[0.1])
    with pytest.raises(capi.NraError) as e:                  # good arguments: the device index is looked at last
        capi.censored_fit(**good, fit_problem=[0], fit_n=[1], fit_open=[1], starts=[1.5], device=99)
    assert e.value.code == -1 and "device index" in str(e.value)
    with pytest.raises(capi.NraError) as e:
        capi.censored_posteriors(**good, model_n=[1], model_open=[1], w=[0.5, 0.5], nu=[1.5], device=99)
    assert e.value.code == -1 and "device index" in str(e.value)
    out = capi.censored_fit(**good, fit_problem=[], fit_n=[], fit_open=[], starts=[])
    assert len(out["ll"]) == 0 and len(out["w"]) == 0
    # N = 1: one exact value, one component; the mean is the value, the weight 1
    out = capi.censored_fit([2.5], [0], [1], [1], [0.07], [0], [1], [0], [9.0])
    assert abs(out["nu"][0] - 2.5) < 1e-12 and abs(out["w"][0] - 1) < 1e-12 and out["converged"][0] == 1


def test_bam_command_on_the_gpu_equals_the_restatement_as_engine(capi, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from test_partial_cpu import partial_panel
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, partial_reads=True, censored_fit=True)
    dev = pipeline.quantify_from_bam(*args, str(tmp_path / "dev"), **common)
    ref = pipeline.quantify_from_bam(*args, str(tmp_path / "ref"), censored_engine=REF, **common)
    capsys.readouterr()
    rows = {}
    for name in ("dev", "ref"):
        rows[name] = [l.split("\t") for l in (tmp_path / f"{name}.NanoRepeat_censored.tsv").read_text().split("\n") if l]
    discrete = (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12)
    assert len(rows["dev"]) == 4
    for a, b in zip(rows["dev"], rows["ref"]):
        assert [a[i] for i in discrete] == [b[i] for i in discrete]
    assert rows["dev"][1][7:9] == ["1", "1"] and int(rows["dev"][1][11]) >= 260       # the allele no read spans
    assert rows["dev"][2][7:9] == ["2", "0"] and rows["dev"][2][11] == "-"              # 6 and 17 units, both spanned
    assert [round(float(s)) for s in rows["dev"][2][9].split(",")] == [6, 17]
    for a, b in zip(dev[:2], ref[:2]):
        fa, fb = a.censored_fit, b.censored_fit
        assert (fa.n, fa.open, fa.open_min_size(), fa.problem.cens_bounds) == (fb.n, fb.open, fb.open_min_size(),
                                                                            fb.problem.cens_bounds)
        assert sorted(fa.bics) == sorted(fb.bics)
        assert _rel(fa.ll, fb.ll) <= TOLERANCE and _rel(fa.nu, fb.nu) <= TOLERANCE and _rel(fa.w, fb.w) <= TOLERANCE
        assert np.array_equal(fa.resp_exact.argmax(axis=1), fb.resp_exact.argmax(axis=1))
        assert np.abs(fa.resp_cens - fb.resp_cens).max() <= 1e-6
        assert [r[:2] + r[5:6] + r[7:] for r in fa.allele_rows()] == [r[:2] + r[5:6] + r[7:] for r in fb.allele_rows()]
