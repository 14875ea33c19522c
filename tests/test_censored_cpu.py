"""The censored allele fit without a GPU: the restatement's erfcx, EM that never loses likelihood, the five scenarios and
the four-class panel of DESIGN.md section 26 through the product's host code (starts, BIC rule) with the restatement as
engine, the BAM command with stand-in engines (every earlier output byte-identical), and the C ABI's declarations and
argument checks."""
import math
import os
import sys

import numpy as np
import pytest

from nanorepeat_amd import censored, round3 as R3
import censored_ref as REF
import censored_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- the restatement's special functions
def test_erfcx_continued_fraction_and_branches():
    for u in (1e-3, 0.5, 1.0, 3.0, 4.999, 5.0):
        assert REF.erfcx(u) == math.exp(u * u) * math.erfc(u)
    # the two forms meet at the border, and the large-u form follows the asymptotic series 1 / (u sqrt(pi)) (1 - 1 / (2 u^2))
    hi, lo = REF.erfcx(5.0 + 1e-9), REF.erfcx(5.0)
    assert abs(hi - (lo + 1e-9 * (10.0 * lo - 2.0 / math.sqrt(math.pi)))) <= 1e-13 * lo      # erfcx' = 2 u erfcx - 2 / sqrt(pi)
    for u in (30.0, 45.0, 1e3):
        want = 1.0 / (u * math.sqrt(math.pi)) * (1.0 - 0.5 / (u * u) + 0.75 / u ** 4)
        assert abs(REF.erfcx(u) - want) <= 4.0 / u ** 6 * want
    # logS and lambda are finite 45 sd either side, continuous at z = 0, and the array form is the scalar form
    z = np.array([-45.0, -8.0, -1e-9, 0.0, 1e-9, 3.0, 7.0, 7.2, 45.0])
    ls, lam = REF.log_s_lambda(z)
    assert np.isfinite(ls).all() and np.isfinite(lam).all() and (np.diff(ls) <= 0).all() and (np.diff(lam) >= 0).all()
    assert ls[3] == math.log(0.5) and abs(lam[3] - REF.SQRT_2_PI) < 1e-15 and abs(ls[0]) < 1e-300
    assert abs(lam[-1] - 45.0) < 0.03                     # lambda(z) -> z + 1 / z
    for i, v in enumerate(z):
        u = v * REF.SQRT1_2
        if u > 0:
            assert abs(ls[i] - (math.log(0.5 * REF.erfcx(u)) - u * u)) <= 1e-15 * abs(ls[i])
            assert abs(lam[i] - REF.SQRT_2_PI / REF.erfcx(u)) <= 1e-15 * lam[i]


def test_erfcx_equals_scipy_where_scipy_is_installed():
    try:
        from scipy.special import erfcx
    except ImportError:
        return                                            # nothing to compare with: the checks above stand alone
    u = np.concatenate([np.linspace(1e-6, 5.0, 400), np.linspace(5.0, 60.0, 400), [100.0, 1e3, 1e4]])
    got = np.array([REF.erfcx(float(v)) for v in u])
    want = erfcx(u)
    # exp(u^2) erfc(u) carries the rounding of u^2 through exp: a relative 25 eps at u = 5
    assert (np.abs(got - want) <= 1e-13 * want).all(), float(np.max(np.abs(got / want - 1)))
    assert (np.abs(REF._erfcx_array(u, np.array([math.erfc(v) for v in u])) - got) <= 1e-15 * got).all()


# ---------------------------------------------------------------------------- EM
@pytest.fixture(scope="module")
def fit_panel_ref():
    fp = K.fit_panel()
    traces = []
    return fp, REF.censored_fit(**fp, traces=traces), traces


def test_lb_never_decreases_and_the_panel_keeps_its_distance_from_the_tolerance(fit_panel_ref):
    fp, out, traces = fit_panel_ref
    assert len(traces) == len(fp["fit_n"]) > 100
    for f, tr in enumerate(traces):
        assert len(tr) == out["n_iter"][f]
        assert all(b >= a - 1e-12 for a, b in zip(tr[:-1], tr[1:])), f
    # what the GPU test relies on: no fit decides its last step within 1e-3 (relative) of the tolerance
    assert K.margin_ok(traces)
    assert set(fp["prob_n"].tolist()) == set(K.FIT_SIZES)
    used = {(int(n), int(o)) for n, o in zip(fp["fit_n"], fp["fit_open"])}
    assert used == {(n, o) for n in range(1, 5) for o in (0, 1)}
    assert 0 < int((out["converged"] == 0).sum()) < len(traces) // 3
    for f in range(len(traces)):
        w = out["w"][out["w_off"][f]:out["w_off"][f + 1]]
        assert abs(w.sum() - 1.0) < 1e-12 and (w > 0).all()


def test_starts_and_model_choice():
    e, c = [1.0, 2.0, 3.0, 4.0], [0.5, 9.0]
    assert censored.start_means(e, c, 2) == [[2.0, 4.0], [1.0, 4.0], [3.0, 9.0]]
    assert censored.start_means(e, c, 1) == [[3.0], [3.0], [9.0]]
    assert censored.start_means([5.0], [], 3) == [[5.0] * 3, [5.0] * 3, [5.0] * 3]
    assert censored.quant([1, 2, 3], 2, 3) == 3 and censored.quant([1, 2, 3], 0, 1) == 2
    assert censored.models_of(9, 0) == [(n, 0) for n in range(1, 7)]
    assert censored.models_of(2, 3) == [(1, 0), (1, 1), (2, 0), (2, 1)]
    assert censored.choose_model({(1, 0): 5.0, (1, 1): 5.0 - 2e-9, (2, 0): 7.0}) == (1, 1)
    assert censored.choose_model({(1, 0): 5.0, (1, 1): 5.0 - 5e-10, (2, 0): 5.0}) == (1, 0)     # a tie: fewer parameters
    assert censored.bic_of(-10.0, 2, 1, 100) == 20.0 + 4 * math.log(100)


def test_the_five_scenarios():
    cases = K.scenarios()
    fits = censored.fit_problems([pr for _, pr, _ in cases], engine=REF)
    for (name, pr, want), cf in zip(cases, fits):
        assert (cf.n, cf.open) == want, (name, cf.bics)
        assert cf.resp_exact.shape == (pr.m, cf.n + cf.open) and cf.resp_cens.shape == (pr.q, cf.n + cf.open)
        assert np.allclose(cf.resp_exact.sum(axis=1), 1.0, atol=1e-12) and np.allclose(cf.resp_cens.sum(axis=1), 1.0, atol=1e-12)
        assert cf.sizes() == sorted(cf.sizes())
    minority, unspanned, homo, two, three = fits
    # the long allele's weight is its share of all reads (2 + its bounds that only it explains), not 2 of 32
    pr = cases[0][1]
    share = (2 + sum(c > 30 for c in pr.cens_bounds)) / (pr.m + pr.q)
    assert abs(minority.w[1] - share) < 0.12 and minority.w[1] > 0.3
    assert abs(minority.sizes()[0] - 20) < 1.5 and abs(minority.sizes()[1] - 150) < 12
    rows = minority.allele_rows()
    assert [r[5] for r in rows] == [30, 2] and abs(sum(r[6] for r in rows) - pr.q) < 1e-9
    assert unspanned.open_min_size() == max(cases[1][1].cens_bounds) and unspanned.w[-1] > 0.3
    assert (unspanned.resp_exact[:, -1] == 0).all()
    assert abs(homo.w[0] - 1) < 1e-12
    assert abs(two.sizes()[0] - 20) < 1.5 and abs(two.sizes()[1] - 32) < 2
    assert three.open_min_size() > 300 and abs(three.sizes()[1] - 45) < 3


def test_the_panel_of_four_classes_is_called():
    """4 x 100 regions, read noise 4 %, the bounds with the same noise: at least 95 of each class get their model.
    Measured with this seed: 100, 100, 100, 100."""
    counts = K.call_counts(K.panel(), REF)
    print("censored panel, regions called as planted:", counts)
    for cls in K.PANEL_CLASSES:
        assert counts[cls] >= 95, counts


# ---------------------------------------------------------------------------- regions, files, the command
class _Sized:
    def __init__(self, size):
        self.round3_repeat_size = size


class _Bound:
    def __init__(self, v):
        self.min_repeat_size = self.repeat_units = v


def _region(sizes, partial=(), in_repeat=()):
    rr = R3.RepeatRegion("chr1\t1000\t1030\tCAG")
    rr.read_dict = {f"s{i}": _Sized(x) for i, x in enumerate(sizes)}
    rr.partial_reads = {f"p{i}": _Bound(v) for i, v in enumerate(partial)}
    rr.in_repeat_reads = {f"i{i}": _Bound(v) for i, v in enumerate(in_repeat)}
    rr.no_details, rr.out_prefix = False, None
    return rr


def test_a_region_without_a_spanning_read_gets_its_row():
    calls = []

    class Engine:
        @staticmethod
        def censored_fit(*a, **k):
            calls.append(a)
            return REF.censored_fit(*a, **k)
        censored_posteriors = staticmethod(REF.censored_posteriors)

    bare, none, sized = _region([], [None, 0, 312, 40], [7]), _region([None]), _region([20.0, 21.0, 20.0, None], [None, 0, 5])
    censored.censored_regions([bare, none, sized], "ont", engine=Engine)
    assert len(calls) == 1 and len(calls[0][1]) == 1                 # one call, and only the third region is a problem
    cf = bare.censored_fit
    assert (cf.problem.m, cf.problem.q, cf.n, cf.open, cf.open_min_size()) == (0, 3, 0, 1, 312)
    assert censored.censored_summary_row(bare) == "chr1\t1000\t1030\tCAG\t0\t3\t0\t0\t1\t-\t-\t312\t0\n"
    assert censored.censored_summary_row(none) == "chr1\t1000\t1030\tCAG\t0\t0\t0\t0\t0\t-\t-\t-\t0\n"
    text = censored.censored_fit_text(bare).split("\n")
    assert text[:4] == ["##RepeatRegion=chr1-1000-1030-CAG", "##Tau=0.07", "##Num_Spanning=0", "##Num_Censored=3"]
    assert text[4] == "#Allele\tKind\tSize\tMedian_Spanning_Size\tWeight\tSpanning_Reads\tCensored_Reads\tMin_Size"
    assert text[5] == "1\topen\t-\t-\t-\t0\t3.00\t312"
    reads = censored.censored_reads_text(bare).split("\n")
    assert reads[1] == "#Read_Name\tKind\tMin_Size\tP_Allele1" and reads[2] == "p2\tone_anchor\t312\t1.0000"
    assert reads[4] == "i0\tin_repeat\t7\t1.0000"
    # values that are None or below 1 are dropped; sizes that are None are no exact observation
    cf = sized.censored_fit
    assert (cf.problem.m, cf.problem.cens_bounds, cf.n, cf.open) == (3, [5], 1, 0)
    assert censored.censored_summary_row(sized).split("\t")[4:9] == ["3", "1", "0", "1", "0"]
    assert censored.censored_summary_row(sized).rstrip("\n").split("\t")[-1] == "1"       # the standard call has none
    # the switches choose the kinds; the error rate is tau
    censored.censored_regions([bare], "ont", engine=Engine, use_in_repeat=False, error_rate=0.05)
    assert (bare.censored_fit.problem.q, bare.censored_fit.problem.tau) == (2, 0.05)
    with pytest.raises(ValueError):
        censored.censored_regions([bare], "ont", engine=Engine, error_rate=0.0)
    with pytest.raises(ValueError):
        censored.fit_problems([sized.censored_fit.problem], max_alleles=9, engine=Engine)
    err = []

    class Stream:
        write = staticmethod(err.append)

    assert censored.report_censored_calls([bare, none, sized], stream=Stream) == (1, 1)
    assert "1 region(s) have an open allele" in "".join(err)


def test_bam_command_adds_files_and_changes_none(oracle, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from extend_ref import ref_extend_tracts
    from test_partial_cpu import partial_panel, _tree
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  extension_engine=ref_extend_tracts, partial_reads=True, in_repeat_reads=True)
    with pytest.raises(ValueError, match="partial_reads"):
        pipeline.quantify_from_bam(*args, str(tmp_path / "bad"), censored_fit=True, data_type="ont_q20")
    with pytest.raises(ValueError, match="partial_reads"):
        pipeline.quantify_from_reads(str(tmp_path / "in.fq"), *args[1:], str(tmp_path / "bad"), censored_fit=True)
    with pytest.raises(ValueError, match="censored_max_alleles"):
        pipeline.quantify_from_bam(*args, str(tmp_path / "bad"), censored_fit=True, censored_max_alleles=9, **common)
    pipeline.quantify_from_bam(*args, str(tmp_path / "off"), **common)
    capsys.readouterr()
    regions = pipeline.quantify_from_bam(*args, str(tmp_path / "on"), censored_fit=True, censored_engine=REF, **common)
    err = capsys.readouterr().err
    new = (".censored_fit.tsv", ".censored_reads.tsv")
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(new)} == off and not any(k.endswith(new) for k in off)
    assert sum(k.endswith(new[0]) for k in on) == 2 and sum(k.endswith(new[1]) for k in on) == 2
    tops = {p.name[len("on"):] for p in tmp_path.glob("on.*") if p.is_file()}
    assert tops == {p.name[len("off"):] for p in tmp_path.glob("off.*") if p.is_file()} | {".NanoRepeat_censored.tsv"}
    for name in tops - {".NanoRepeat_censored.tsv"}:
        assert (tmp_path / f"on{name}").read_bytes() == (tmp_path / f"off{name}").read_bytes(), name
    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_censored.tsv").read_text().split("\n") if l]
    assert "\t".join(rows[0]) + "\n" == censored.SUMMARY_HEADER and len(rows) == 4
    # region 0: sixteen reads span the 10-unit allele, sixteen cut reads show up to 269 units of the 400-unit one
    assert rows[1][4:9] == ["16", "16", rows[1][6], "1", "1"] and int(rows[1][11]) >= 260
    assert abs(float(rows[1][9]) - 10) < 1
    # region 1: alleles of 6 and 17 units, both spanned; its four cut reads show 6 units and add no allele
    assert rows[2][4:6] == ["16", "4"] and rows[2][7:9] == ["2", "0"] and rows[2][11] == "-"
    assert [round(float(s)) for s in rows[2][9].split(",")] == [6, 17]
    assert rows[3][4:] == ["0", "0", "0", "0", "0", "-", "-", "-", "0"]            # the region without reads
    fit = [v for k, v in on.items() if k.endswith(new[0]) and "CAG" in k][0].decode().split("\n")
    assert fit[0] == f"##RepeatRegion={regions[0].to_unique_id()}" and fit[1] == "##Tau=0.07"
    assert any(l.startswith("##BIC(n=1,open=1)=") for l in fit)
    body = [l.split("\t") for l in fit if l and not l.startswith("#")]
    assert [b[1] for b in body] == ["closed", "open"] and body[0][5] == "16" and body[1][7] == rows[1][11]
    reads = [v for k, v in on.items() if k.endswith(new[1]) and "CAG" in k][0].decode().split("\n")
    assert reads[1] == "#Read_Name\tKind\tMin_Size\tP_Allele1\tP_Allele2" and len([l for l in reads if l]) == 2 + 16
    notices = [l for l in err.split("\n") if l.startswith("NOTICE: censored fit")]
    assert len(notices) == 1 and "1 region(s) have an open allele" in notices[0]


# ---------------------------------------------------------------------------- C ABI
def test_c_abi_declares_both_symbols_and_checks_arguments_before_the_device(capi):
    header = open(os.path.join(ROOT, "include", "nanorepeat_amd.h")).read()
    for sym in ("nra_censored_fit", "nra_censored_posteriors"):
        assert f"int {sym}(int device" in header and sym in capi.EXPORTS
        getattr(capi.load(), sym)
    assert capi.load().nra_abi_version() == 4
    for name, code in fit_argument_errors(capi, device=0):
        assert code is not None, name
    if capi.load().nra_device_count() <= 0:              # good arguments: the device is looked at last
        for call in (lambda: capi.censored_fit([1.0, 2.0, 3.0], [0], [3], [2], [0.1], [0], [1], [1], [1.5]),
                     lambda: capi.censored_posteriors([1.0, 2.0, 3.0], [0], [3], [2], [0.1], [1], [1], [0.5, 0.5], [1.5])):
            with pytest.raises(capi.NraError) as e:
                call()
            assert e.value.code == -2 and "no HIP device" in str(e.value)


def fit_argument_errors(capi, device):
    """Every argument error of the two entry points, asserted; yields (case, code) for the caller's count."""
    y = [1.0, 2.0, 3.0]
    good = dict(values=y, prob_off=[0], prob_n=[3], prob_n_exact=[2], prob_tau=[0.1], fit_problem=[0], fit_n=[1],
                fit_open=[1], starts=[1.5])
    cases = [("n = 0", dict(fit_n=[0], starts=[]), capi.E_RANGE),
             ("n = 9", dict(fit_n=[9], starts=[1.0] * 9), capi.E_RANGE),
             ("N > 2^20", dict(values=np.zeros((1 << 20) + 1), prob_n=[(1 << 20) + 1]), capi.E_RANGE),
             ("n_exact = 0", dict(prob_n_exact=[0]), -1),
             ("n_exact > N", dict(prob_n_exact=[4]), -1),
             ("a value is nan", dict(values=[1.0, float("nan"), 3.0]), -1),
             ("a value is inf", dict(values=[1.0, 2.0, float("inf")]), -1),
             ("tau = 0", dict(prob_tau=[0.0]), -1),
             ("tau < 0", dict(prob_tau=[-0.1]), -1),
             ("tau is nan", dict(prob_tau=[float("nan")]), -1),
             ("tau is inf", dict(prob_tau=[float("inf")]), -1),
             ("open without a bound", dict(prob_n_exact=[3]), -1),
             ("open = 2", dict(fit_open=[2]), -1),
             ("problem out of range", dict(fit_problem=[1]), -1),
             ("values outside the buffer", dict(prob_off=[1]), -1),
             ("a start is nan", dict(starts=[float("nan")]), -1),
             ("max_iter = 0", dict(max_iter=0), -1),
             ("max_iter = 501", dict(max_iter=501), capi.E_RANGE),
             ("tol < 0", dict(tol=-1.0), -1),
             ("unknown flag", dict(flags=2), -1)]
    for name, change, code in cases:
        with pytest.raises(capi.NraError) as e:
            capi.censored_fit(**{**good, **change}, device=device)
        assert e.value.code == code, (name, str(e.value))
        yield name, code
    model = dict(values=y, prob_off=[0], prob_n=[3], prob_n_exact=[2], prob_tau=[0.1], model_n=[1], model_open=[1],
                 w=[0.5, 0.5], nu=[1.5])
    for name, change, code in (("n = 9", dict(model_n=[9], w=[0.1] * 10, nu=[1.0] * 9), capi.E_RANGE),
                               ("n_exact = 0", dict(prob_n_exact=[0]), -1),
                               ("tau = 0", dict(prob_tau=[0.0]), -1),
                               ("a value is nan", dict(values=[float("nan"), 2.0, 3.0]), -1),
                               ("open without a bound", dict(prob_n_exact=[3]), -1),
                               ("a weight is 0", dict(w=[0.0, 1.0]), -1),
                               ("a mean is inf", dict(nu=[float("inf")]), -1)):
        with pytest.raises(capi.NraError) as e:
            capi.censored_posteriors(**{**model, **change}, device=device)
        assert e.value.code == code, (name, str(e.value))
        yield "posteriors: " + name, code
