"""The bootstrap of the censored allele fit on the GPU: k_censored_boot and k_censored_pick (nra_censored_bootstrap)
against the composed device path -- the replicate materialised on the host, its starts from censored.start_means, its
fits from nra_censored_fit, the BIC rule in Python (tests/censored_boot_ref.py over _capi) -- bit for bit: both paths
run one fit body on the same values from the same starts, so no tolerance is involved.  Problems of N at the lane and
register-class borders and one of 3000 values, m from 1 to N, max_alleles 1 and 4; rows: the identity, exact draws only,
bounds only, one exact value repeated, seeded random rows.  Then the invariances (streaming form, problems reversed, a
replicate alone, the launch-group budget forced small), the argument errors, and the BAM command."""
import math
import sys

import numpy as np
import pytest

from nanorepeat_amd import censored
import censored_boot_ref as BREF

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 511, 512, 513)
KEYS = ("status", "model_n", "model_open", "best_start", "n_iter", "ll", "bic", "nu", "w")


def _problem(rng, N, m, tau, n_rep):
    """A problem in sorted layout and its n_rep rows (n_rep = 8: all kinds; fewer: the first kinds)."""
    alleles = [20.0, 55.0, 140.0][:int(rng.integers(2, 4))]
    exact = [max(0.0, round(alleles[int(rng.integers(0, len(alleles)))] * (1 + 0.05 * rng.standard_normal())))
             for _ in range(m)]
    bounds = [max(1, int(rng.random() * (600 if N % 2 else 140))) for _ in range(N - m)]
    ys = sorted(censored.log_size(x) for x in exact) + sorted(censored.log_size(c) for c in bounds)
    random_row = lambda: np.sort(rng.integers(0, N, size=N))
    rows = [np.arange(N),                                                        # the problem itself
            np.sort(rng.integers(0, m, size=N)),                                 # exact draws only: no open model
            np.full(N, int(rng.integers(0, m))),                                 # one exact value: n = 1 only
            np.sort(rng.integers(m, N, size=N)) if N > m else random_row()]      # bounds only: not fitted
    rows += [random_row() for _ in range(n_rep - len(rows))]
    return dict(ys=ys, m=m, tau=tau, rows=np.array(rows[:n_rep], np.int32))


def _args(problems):
    """The arguments of censored_bootstrap for a list of _problem dicts with equally many rows."""
    off = np.concatenate([[0], np.cumsum([len(p["ys"]) for p in problems])]).astype(np.int64)
    n = np.array([len(p["ys"]) for p in problems], np.int32)
    return dict(values=np.concatenate([p["ys"] for p in problems]), prob_off=off[:-1], prob_n=n,
                prob_n_exact=np.array([p["m"] for p in problems], np.int32),
                prob_tau=np.array([p["tau"] for p in problems]), prob_ln_n=np.array([math.log(int(k)) for k in n]),
                n_rep=len(problems[0]["rows"]), idx=np.concatenate([p["rows"].ravel() for p in problems]),
                rep_m=np.array([(p["rows"] < p["m"]).sum(axis=1) for p in problems], np.int32))


def _same_bits(a, b, sel_a=slice(None), sel_b=slice(None)):
    for key in KEYS:
        assert np.ascontiguousarray(a[key][sel_a]).tobytes() == np.ascontiguousarray(b[key][sel_b]).tobytes(), key


@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(27)
    small = [_problem(rng, N, m, (0.07, 0.05, 0.1)[i % 3], 8)
             for N in SIZES for i, m in enumerate(sorted({1, max(1, N // 3), max(1, N - 1), N}))]
    big = [_problem(rng, 3000, 1000, 0.07, 4)]
    return small, big


@pytest.fixture(scope="module")
def on_device(capi, panel):
    """{(which, max_alleles): result} of the entry point, computed once."""
    return {(which, a): capi.censored_bootstrap(**_args(problems), max_alleles=a)
            for which, problems in zip(("small", "big"), panel) for a in (1, 4)}


@pytest.mark.parametrize("max_alleles", (1, 4))
def test_every_replicate_equals_the_composed_device_path_bit_for_bit(capi, panel, on_device, max_alleles):
    for which, problems in zip(("small", "big"), panel):
        args = _args(problems)
        got = on_device[(which, max_alleles)]
        want = BREF.censored_bootstrap(**args, max_alleles=max_alleles, fit_engine=capi)
        _same_bits(got, want)
        # the rows do what they are there for
        rep_m = args["rep_m"]
        assert np.array_equal(got["status"] == capi.CENS_BOOT_NO_EXACT, rep_m == 0)
        assert (got["model_n"][rep_m == 0] == 0).all() and (got["model_open"][rep_m == 0] == 1).all()
        assert (got["model_n"][:, 2] == 1).all() and (got["model_open"][:, 1] == 0).all()
        assert (got["model_n"][rep_m > 0] >= 1).all() and got["model_n"].max() <= max_alleles
        assert np.isfinite(got["ll"]).all() and np.isfinite(got["bic"]).all()
        fitted = got["status"] == capi.CENS_BOOT_FITTED
        assert (got["n_iter"][fitted] >= 1).all() and (got["n_iter"] <= 500).all()
        assert np.abs(got["w"].sum(axis=2)[fitted] - 1.0).max() < 1e-9
        assert (rep_m == 0).any()
        print(f"{which}, max_alleles {max_alleles}: {int(fitted.sum())} fitted replicates, "
              f"{int((got['model_open'][fitted] == 1).sum())} with an open allele, "
              f"{int((got['model_n'] > 1).sum())} with more than one closed allele, "
              f"{int((got['best_start'] > 0).sum())} from a start other than the first")


def test_bits_do_not_move_with_the_form_the_order_the_company_or_the_budget(capi, panel, on_device, monkeypatch):
    small, big = panel
    both = small + [dict(p, rows=np.concatenate([p["rows"], p["rows"]])) for p in big]       # 8 rows everywhere
    base = capi.censored_bootstrap(**_args(both), max_alleles=4)
    _same_bits(base, on_device[("small", 4)], slice(0, len(small)))
    _same_bits(base, on_device[("big", 4)], (slice(len(small), None), slice(0, 4)))
    # the streaming form of every problem
    _same_bits(base, capi.censored_bootstrap(**_args(both), max_alleles=4, flags=capi.CENS_F_STREAM))
    # problems reversed
    _same_bits(base, capi.censored_bootstrap(**_args(both[::-1]), max_alleles=4), slice(None, None, -1))
    # a replicate alone in a call
    for p, b in ((0, 0), (len(small) - 1, 3), (len(small) - 2, 7), (len(both) - 1, 3), (10, 5)):
        alone = capi.censored_bootstrap(**_args([dict(both[p], rows=both[p]["rows"][b:b + 1])]), max_alleles=4)
        _same_bits(base, alone, (slice(p, p + 1), slice(b, b + 1)))
    # launch groups of one problem each, and of a few
    for budget in ("1", str(40 * 8 * 8 * 160)):
        monkeypatch.setenv("NRA_TEST_CENS_BOOT_BYTES", budget)
        _same_bits(base, capi.censored_bootstrap(**_args(both), max_alleles=4))
    monkeypatch.delenv("NRA_TEST_CENS_BOOT_BYTES")


def test_argument_errors_come_before_the_device(capi):
    from test_censored_bootstrap_cpu import GOOD, bootstrap_argument_errors
    assert len(list(bootstrap_argument_errors(capi, device=99))) == 25
    with pytest.raises(capi.NraError) as e:                  # good arguments: the device index is looked at last
        capi.censored_bootstrap(**GOOD, device=99)
    assert e.value.code == -1 and "device index" in str(e.value)
    out = capi.censored_bootstrap(**GOOD)
    assert out["status"].tolist() == [[capi.CENS_BOOT_FITTED, capi.CENS_BOOT_NO_EXACT]]
    assert out["model_n"][0, 0] in (1, 2) and out["model_n"][0, 1] == 0 and out["model_open"][0, 1] == 1
    empty = capi.censored_bootstrap([], [], [], [], [], [], 3, [], [], 2)
    assert empty["status"].shape == (0, 3)


def _tree(root):
    import os
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_bam_command_device_engine_equals_composed_device_path(capi, tmp_path, monkeypatch, capsys):
    from nanorepeat_amd import pipeline
    from test_partial_cpu import partial_panel
    monkeypatch.setitem(sys.modules, "pysam", None)
    partial_panel(tmp_path)
    args = (str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "r.bed"))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, partial_reads=True, censored_fit=True,
                  censored_bootstrap=16)
    with pytest.raises(ValueError, match="censored_fit=True"):
        pipeline.quantify_from_bam(*args, str(tmp_path / "bad"), data_type="ont_q20", censored_bootstrap=16)
    dev = pipeline.quantify_from_bam(*args, str(tmp_path / "dev"), **common)
    pipeline.quantify_from_bam(*args, str(tmp_path / "cmp"), censored_engine=BREF.Composed(capi), **common)
    capsys.readouterr()
    a, b = _tree(tmp_path / "dev.details"), _tree(tmp_path / "cmp.details")
    new = ".censored_bootstrap.tsv"
    assert sum(k.endswith(new) for k in a) == 2 and a == b
    summary = (tmp_path / "dev.NanoRepeat_censored_bootstrap.tsv").read_bytes()
    assert summary == (tmp_path / "cmp.NanoRepeat_censored_bootstrap.tsv").read_bytes()
    rows = [l.split("\t") for l in summary.decode().split("\n") if l]
    assert "\t".join(rows[0]) + "\n" == censored.BOOT_HEADER
    assert [r[4:6] for r in rows[1:]] == [["1", "closed"], ["2", "open"], ["1", "closed"], ["2", "closed"], ["-", "-"]]
    assert all(r[13] == "16" for r in rows[1:5])
    assert float(rows[1][15]) > 0.5 > float(rows[3][15])             # an open allele where no read spans one
    boot = dev[0].censored_bootstrap
    assert boot.n_replicates == 16 and boot.seed == 1 and len(boot.rows) == 2
