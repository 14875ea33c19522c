"""The bootstrap of the censored allele fit without a GPU: the statistics on hand-made replicate
tables, the resampling rows, the kernel's way of taking the starts by position against censored.start_means, the
composed restatement (tests/censored_boot_ref.py) on two scenarios, the files and the BAM command with the restatement
as engine, the ValueErrors, and the argument checks of nra_censored_bootstrap, which come before the device."""
import math
import os
import sys

import numpy as np
import pytest

from nanorepeat_amd import censored, round3 as R3
import censored_boot_ref as BREF
import censored_cases as K
import censored_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fit:
    """What CensoredBootstrap reads of a call."""

    def __init__(self, n, open_):
        self.n, self.open = n, open_


def _table(models):
    """models: [(nu list, w list incl. the open weight)] per replicate, as the engine lays them out -> n, open, nu, w."""
    B = len(models)
    n, o, nu, w = np.zeros(B, int), np.zeros(B, int), np.zeros((B, 8)), np.zeros((B, 9))
    for b, (means, weights) in enumerate(models):
        n[b], o[b] = len(means), len(weights) - len(means)
        nu[b, :len(means)], w[b, :len(weights)] = means, weights
    return n, o, nu, w


# ---------------------------------------------------------------------------- statistics
def test_percentile_indices_at_r_1_2_and_200():
    q = 0.025
    for r, lo, hi in ((1, 0, 0), (2, 0, 1), (200, 4, 195)):
        assert (int(math.floor(q * (r - 1) + 1e-9)), int(math.ceil((1 - q) * (r - 1) - 1e-9))) == (lo, hi)
        v = np.random.default_rng(r).permutation(r).astype(float)
        assert censored.percentile_interval(v, 0.95) == (lo, hi)
    assert censored.percentile_interval([], 0.95) is None
    # through the class: r = 1 and r = 2 replicates with the called closed count
    y20, y30 = math.log(30.0), math.log(40.0)
    n, o, nu, w = _table([([y20], [1.0]), ([y30], [1.0]), ([y20, y30], [0.5, 0.5])])
    one = censored.CensoredBootstrap(1, [3, 3, 3], n, o, nu, w, _Fit(2, 0), 0.95)
    assert one.rows == [("closed", pytest.approx(20.0), pytest.approx(20.0), 0.5, 0.5, 1),
                        ("closed", pytest.approx(30.0), pytest.approx(30.0), 0.5, 0.5, 1)]
    two = censored.CensoredBootstrap(1, [3, 3, 3], n, o, nu, w, _Fit(1, 0), 0.95)
    assert two.rows == [("closed", pytest.approx(20.0), pytest.approx(30.0), 1.0, 1.0, 2)]
    assert (one.model_support, two.model_support, one.open_support) == (1 / 3, 2 / 3, 0.0)
    # r = 200: the interval is v[4] .. v[195] of the sorted sizes
    sizes = np.random.default_rng(0).permutation(200) + 20.0
    n, o, nu, w = _table([([math.log(10.0 + s)], [1.0]) for s in sizes])
    big = censored.CensoredBootstrap(1, [5] * 200, n, o, nu, w, _Fit(1, 0), 0.95)
    assert big.rows[0][1:3] == (pytest.approx(24.0), pytest.approx(215.0)) and big.rows[0][5] == 200


def test_rank_matching_distribution_and_unfitted_replicates():
    a, b, c = math.log(30.0), math.log(60.0), math.log(110.0)
    n, o, nu, w = _table([
        ([b, a], [0.7, 0.3]),                     # means out of order: ranked by size, weights follow
        ([a, b], [0.4, 0.6]),
        ([a, a], [0.2, 0.8]),                     # a tie keeps the engine's order
        ([a, b], [0.25, 0.25, 0.5]),              # (2, 1): counts for the closed alleles, not for the model
        ([c], [0.9, 0.1]),                        # (1, 1)
        ([], []), ([], [])])                      # unfitted
    o[5], o[6] = 1, 0                             # 0+1 and 0+0
    boot = censored.CensoredBootstrap(9, [4, 4, 4, 4, 4, 0, 0], n, o, nu, w, _Fit(2, 0), 0.95)
    assert boot.distribution == "0+0:1,2+0:3,0+1:1,1+1:1,2+1:1"
    assert boot.model_support == 3 / 7 and boot.open_support == 3 / 7
    assert np.array_equal(boot.w[:4, :2], [[0.3, 0.7], [0.4, 0.6], [0.2, 0.8], [0.25, 0.25]])
    assert boot.w.shape == (7, 8) and np.isnan(boot.w[:4, 2:]).all()
    assert np.isnan(boot.nu[4, 1]) and np.isnan(boot.nu[5]).all()
    assert boot.w_open[3] == 0.5 and boot.w_open[4] == 0.1 and np.isnan(boot.w_open[[0, 1, 2, 5, 6]]).all()
    assert [r[5] for r in boot.rows] == [4, 4]                       # the four replicates with two closed alleles
    assert boot.rows[0][1:5] == (pytest.approx(20.0), pytest.approx(20.0), 0.2, 0.4)
    assert boot.rows[1][1:5] == (pytest.approx(20.0), pytest.approx(50.0), 0.25, 0.8)
    called_open = censored.CensoredBootstrap(9, [4, 4, 4, 4, 4, 0, 0], n, o, nu, w, _Fit(2, 1), 0.95)
    assert called_open.rows[2] == ("open", None, None, 0.5, 0.5, 1) and called_open.model_support == 1 / 7
    none_like_it = censored.CensoredBootstrap(9, [4, 4, 4, 4, 4, 0, 0], n, o, nu, w, _Fit(3, 0), 0.95)
    assert none_like_it.rows == [("closed", None, None, None, None, 0)] * 3 and none_like_it.model_support == 0.0


def test_resampling_rows():
    idx, rep_m = censored.resample_rows(5, 3, m=4, n_points=10, n_rep=6)
    want = np.random.default_rng([5, 3, 0x63656E73]).integers(0, 10, size=(6, 10))
    assert idx.dtype == np.int32 and np.array_equal(idx, np.sort(want, axis=1))
    assert np.array_equal(rep_m, (want < 4).sum(axis=1))
    assert not np.array_equal(idx, censored.resample_rows(5, 4, 4, 10, 6)[0])          # the region names the stream
    pr = K.problem([30.0, 20.0, 25.0], [7, 3])
    assert censored.sorted_layout(pr) == [math.log(10.0 + v) for v in (20, 25, 30)] + [math.log(13.0), math.log(17.0)]


def test_starts_by_index_are_start_means():
    """The kernel takes the starts from the two sorted runs by position (a bounded binary search for the merge); that
    is censored.start_means on every replicate shape, ties and empty bound runs included."""
    rng = np.random.default_rng(4)
    checked = 0
    for m, q in [(1, 0), (1, 1), (2, 0), (1, 7), (7, 1), (5, 5), (40, 25), (64, 64), (3, 200), (200, 3), (513, 0)]:
        for trial in range(4):
            pool = rng.integers(0, 6 if trial % 2 else 1000, size=m + q).astype(float) * 0.25      # with many ties
            y = sorted(pool[:m].tolist()) + sorted(pool[m:].tolist())
            for n in range(1, min(8, len(set(y[:m]))) + 1):
                assert BREF.starts_by_index(y, m, n) == censored.start_means(y[:m], y[m:], n), (m, q, n)
                checked += 1
    assert checked > 100
    # the position is the float64 expression of censored.quant, not the exact quotient: (3 + 0.5) / 5 * 90 rounds to
    # 62.99..., so the kernel evaluates the same expression in float64 instead of ((2 k + 1) L) // (2 n) = 63
    assert BREF.quant_pos(3, 5, 90) == 62 == int(math.floor((3 + 0.5) / 5 * 90)) and (7 * 90) // 10 == 63
    y = [float(v) for v in range(90)]
    assert censored.quant(y, 3, 5) == 62.0 and BREF.starts_by_index(y, 90, 5)[0][3] == 62.0


# ---------------------------------------------------------------------------- the restatement on two scenarios
def test_open_support_orders_the_unspanned_and_the_homozygous_scenario():
    """Scenario 2 (an unspanned allele of 800 units, called (1, 1)) against scenario 3 (homozygous with 8 bounds,
    called (1, 0)), B = 16, max_alleles = 3, the composed restatement as engine.  Measured on the CPU (DESIGN.md
    section 27.3): Open_Support 1.0 and 0.0, clearly either side of 0.5, so both sides are asserted too."""
    sc = K.scenarios()
    assert (sc[1][0], sc[2][0]) == ("unspanned_800", "homozygous_with_bounds")
    problems = [sc[1][1], sc[2][1]]
    fits = censored.fit_problems(problems, max_alleles=3, engine=REF)
    assert [(f.n, f.open) for f in fits] == [(1, 1), (1, 0)]
    unspanned, homozygous = censored.bootstrap_problems(problems, fits, 16, 7, 0.95, 3, BREF)
    print("Open_Support:", unspanned.open_support, homozygous.open_support,
          "Model_Support:", unspanned.model_support, homozygous.model_support)
    assert unspanned.open_support > homozygous.open_support
    assert unspanned.open_support > 0.5 and homozygous.open_support < 0.5
    assert unspanned.n_replicates == 16 and len(unspanned.rows) == 2 and len(homozygous.rows) == 1
    lo, hi = unspanned.rows[0][1:3]
    assert lo <= fits[0].sizes()[0] <= hi and 15 < lo and hi < 25


# ---------------------------------------------------------------------------- regions, files, the command
class _Sized:
    def __init__(self, size):
        self.round3_repeat_size = size


class _Bound:
    def __init__(self, v):
        self.min_repeat_size = self.repeat_units = v


def _region(index, sizes, partial=()):
    rr = R3.RepeatRegion("chr1\t1000\t1030\tCAG")
    rr.read_dict = {f"s{i}": _Sized(x) for i, x in enumerate(sizes)}
    rr.partial_reads = {f"p{i}": _Bound(v) for i, v in enumerate(partial)}
    rr.in_repeat_reads = {}
    rr.no_details, rr.out_prefix, rr.index = False, None, index
    return rr


def test_a_region_without_a_spanning_read_gets_its_dash_row_and_one_call_serves_all():
    calls = []

    class Engine:
        censored_fit, censored_posteriors = staticmethod(REF.censored_fit), staticmethod(REF.censored_posteriors)

        @staticmethod
        def censored_bootstrap(*a, **k):
            calls.append((a, k))
            return BREF.censored_bootstrap(*a, **k)

    bare, unfit, sized = _region(0, [], [312, 40]), _region(1, [None]), _region(2, [20.0, 21.0, 20.0, 22.0], [5, 300])
    regions = [bare, unfit, sized]
    censored.censored_regions(regions, "ont", engine=Engine, max_alleles=2)
    del unfit.censored_fit
    censored.bootstrap_regions(regions, 3, 11, 0.9, 2, Engine)
    assert len(calls) == 1                                           # one call, and only the third region is a problem
    args, kw = calls[0]
    assert len(args[1]) == 1 and args[6] == 3 and args[9] == 2 and kw["max_iter"] == 500 and kw["tol"] == 1e-9
    assert args[5][0] == math.log(6) and list(args[0]) == censored.sorted_layout(sized.censored_fit.problem)
    idx, rep_m = censored.resample_rows(11, 2, 4, 6, 3)
    assert np.array_equal(args[7], idx.ravel()) and np.array_equal(np.ravel(args[8]), rep_m)
    assert bare.censored_bootstrap is None and unfit.censored_bootstrap is None
    dash = "chr1\t1000\t1030\tCAG" + "\t-" * 13 + "\n"
    assert censored.censored_bootstrap_rows(bare) == dash and censored.censored_bootstrap_rows(unfit) == dash
    assert censored.BOOT_HEADER.count("\t") == dash.count("\t") == 16
    rows = censored.censored_bootstrap_rows(sized).split("\n")[:-1]
    cf, boot = sized.censored_fit, sized.censored_bootstrap
    assert len(rows) == cf.n + cf.open and boot.n_replicates == 3 and boot.seed == 11
    first = rows[0].split("\t")
    assert first[4:6] == ["1", "closed"] and first[6] == f"{cf.sizes()[0]:.1f}" and first[13] == "3"
    assert first[14] == f"{boot.model_support:.4f}" and first[15] == f"{boot.open_support:.4f}"
    assert sum(int(c) for c in (part.split(":")[1] for part in first[16].split(","))) == 3
    text = censored.censored_bootstrap_text(sized).split("\n")
    assert text[:3] == ["##RepeatRegion=chr1-1000-1030-CAG", "##Seed=11",
                        "#Replicate\tNum_Spanning\tNum_Closed\tOpen\tSizes\tWeights"]
    assert [l.split("\t")[:2] for l in text[3:6]] == [[str(b), str(int(m))] for b, m in enumerate(rep_m)]
    for b, line in enumerate(text[3:6]):
        f = line.split("\t")
        if rep_m[b] == 0:
            assert f[2:] == ["0", "1", "-", "-"]
        else:
            assert len(f[4].split(",")) == int(f[2]) and len(f[5].split(",")) == int(f[2]) + int(f[3])
    err = []

    class Stream:
        write = staticmethod(err.append)

    boot.model_support = 0.25
    assert censored.report_censored_bootstrap(regions, stream=Stream) == 1
    assert "in 1 of 1 region(s) fewer than half of the replicates" in "".join(err)
    with pytest.raises(ValueError):
        censored.bootstrap_problems([cf.problem], [cf], 0, 1, engine=Engine)
    with pytest.raises(ValueError):
        censored.bootstrap_problems([cf.problem], [cf], 4, 1, max_alleles=9, engine=Engine)


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_bam_command_adds_two_files_and_changes_none(oracle, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from extend_ref import ref_extend_tracts
    from test_partial_cpu import partial_panel
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  extension_engine=ref_extend_tracts, partial_reads=True)
    for bad, message in ((dict(censored_bootstrap=4), "censored_fit=True"),
                         (dict(censored_bootstrap=-1, censored_fit=True), "replicates"),
                         (dict(censored_bootstrap=2.5, censored_fit=True), "replicates")):
        with pytest.raises(ValueError, match=message):
            pipeline.quantify_from_bam(*args, str(tmp_path / "bad"), **{**common, **bad})
        with pytest.raises(ValueError, match=message):
            pipeline.quantify_from_reads(str(tmp_path / "in.fq"), *args[1:], str(tmp_path / "bad"), partial_reads=True,
                                         **bad)
    fit = dict(censored_fit=True, censored_engine=BREF, censored_max_alleles=2)
    pipeline.quantify_from_bam(*args, str(tmp_path / "plain"), **common, **fit)
    pipeline.quantify_from_bam(*args, str(tmp_path / "zero"), **common, **fit, censored_bootstrap=0)
    capsys.readouterr()
    regions = pipeline.quantify_from_bam(*args, str(tmp_path / "boot"), **common, **fit, censored_bootstrap=4)
    err = capsys.readouterr().err
    plain, zero, boot = (_tree(tmp_path / f"{name}.details") for name in ("plain", "zero", "boot"))
    assert plain == zero                                             # 0: byte for byte what it was
    new = ".censored_bootstrap.tsv"
    assert {k: v for k, v in boot.items() if not k.endswith(new)} == plain and not any(k.endswith(new) for k in plain)
    assert sum(k.endswith(new) for k in boot) == 2
    tops = {name: {p.name[len(name):] for p in tmp_path.glob(f"{name}.*") if p.is_file()} for name in ("plain", "zero", "boot")}
    assert tops["plain"] == tops["zero"] and tops["boot"] == tops["plain"] | {".NanoRepeat_censored_bootstrap.tsv"}
    for name in tops["plain"]:
        assert (tmp_path / f"boot{name}").read_bytes() == (tmp_path / f"plain{name}").read_bytes() == \
            (tmp_path / f"zero{name}").read_bytes(), name
    rows = [l.split("\t") for l in (tmp_path / "boot.NanoRepeat_censored_bootstrap.tsv").read_text().split("\n") if l]
    assert "\t".join(rows[0]) + "\n" == censored.BOOT_HEADER
    # region 0: a closed 10-unit allele and the open one; region 1: 6 and 17 units; region 2 has no reads
    assert [r[4:6] for r in rows[1:]] == [["1", "closed"], ["2", "open"], ["1", "closed"], ["2", "closed"], ["-", "-"]]
    assert rows[5][4:] == ["-"] * 13 and all(r[13] == "4" for r in rows[1:5])
    assert float(rows[1][8]) <= float(rows[1][6]) <= float(rows[1][9]) or rows[1][12] == "0"
    assert float(rows[1][15]) > 0.5 > float(rows[3][15])             # an open allele where no read spans one
    per = [v for k, v in boot.items() if k.endswith(new) and "CAG" in k][0].decode().split("\n")
    assert per[0] == f"##RepeatRegion={regions[0].to_unique_id()}" and per[1] == "##Seed=1" and len(per) == 3 + 4 + 1
    assert regions[0].censored_bootstrap.n_replicates == 4 and getattr(regions[2], "censored_bootstrap", None) is None
    assert len([l for l in err.split("\n") if l.startswith("NOTICE: censored bootstrap")]) <= 1


# ---------------------------------------------------------------------------- C ABI
def test_c_abi_declares_the_symbol_and_checks_arguments_before_the_device(capi):
    header = open(os.path.join(ROOT, "include", "nanorepeat_amd.h")).read()
    assert "int nra_censored_bootstrap(int device" in header and "nra_censored_bootstrap" in capi.EXPORTS
    capi.load().nra_censored_bootstrap
    assert capi.load().nra_abi_version() == 4
    for name, code in bootstrap_argument_errors(capi, device=0):
        assert code is not None, name
    if capi.load().nra_device_count() <= 0:                  # good arguments: the device is looked at last
        with pytest.raises(capi.NraError) as e:
            capi.censored_bootstrap(**GOOD)
        assert e.value.code == -2 and "no HIP device" in str(e.value)


GOOD = dict(values=[1.0, 2.0, 1.5, 3.0], prob_off=[0], prob_n=[4], prob_n_exact=[2], prob_tau=[0.1],
            prob_ln_n=[math.log(4)], n_rep=2, idx=[0, 1, 2, 3, 2, 2, 3, 3], rep_m=[2, 0], max_alleles=2)


def bootstrap_argument_errors(capi, device):
    """Every argument error of nra_censored_bootstrap, asserted; yields (case, code) for the caller's count."""
    big = (1 << 20) + 1
    cases = [("n_rep = 0", dict(n_rep=0, idx=[], rep_m=[]), -1),
             ("n_rep = 1001", dict(n_rep=1001, idx=[0, 1, 2, 3] * 1001, rep_m=[2] * 1001), capi.E_RANGE),
             ("an index is N", dict(idx=[0, 1, 2, 4, 2, 2, 3, 3]), -1),
             ("an index is negative", dict(idx=[-1, 1, 2, 3, 2, 2, 3, 3]), -1),
             ("a row descends", dict(idx=[0, 1, 3, 2, 2, 2, 3, 3]), -1),
             ("rep_m disagrees", dict(rep_m=[2, 1]), -1),
             ("a value is nan", dict(values=[1.0, float("nan"), 1.5, 3.0]), -1),
             ("a value is inf", dict(values=[1.0, 2.0, 1.5, float("inf")]), -1),
             ("tau is nan", dict(prob_tau=[float("nan")]), -1),
             ("tau = 0", dict(prob_tau=[0.0]), -1),
             ("tau < 0", dict(prob_tau=[-0.1]), -1),
             ("lnN is nan", dict(prob_ln_n=[float("nan")]), -1),
             ("lnN is inf", dict(prob_ln_n=[float("inf")]), -1),
             ("m = 0", dict(prob_n_exact=[0], rep_m=[0, 0]), -1),
             ("m > N", dict(prob_n_exact=[5], rep_m=[4, 4]), -1),
             ("exact values descend", dict(values=[2.0, 1.0, 1.5, 3.0]), -1),
             ("bounds descend", dict(values=[1.0, 2.0, 3.0, 1.5]), -1),
             ("max_iter = 0", dict(max_iter=0), -1),
             ("max_iter = 501", dict(max_iter=501), capi.E_RANGE),
             ("tol < 0", dict(tol=-1.0), -1),
             ("tol is nan", dict(tol=float("nan")), -1),
             ("unknown flag", dict(flags=2), -1),
             ("max_alleles = 0", dict(max_alleles=0), capi.E_RANGE),
             ("max_alleles = 9", dict(max_alleles=9), capi.E_RANGE),
             ("N > 2^20", dict(values=np.zeros(big), prob_n=[big], idx=np.zeros(2 * big, np.int32), rep_m=[big, big]),
              capi.E_RANGE)]
    for name, change, code in cases:
        with pytest.raises(capi.NraError) as e:
            capi.censored_bootstrap(**{**GOOD, **change}, device=device)
        assert e.value.code == code, (name, str(e.value))
        yield name, code
