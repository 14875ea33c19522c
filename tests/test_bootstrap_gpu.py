"""The bootstrap on the MI355X: nra_mixture_bootstrap (one workgroup runs the whole order search of a replicate) against
the composed path -- every replicate's sample materialised on the host and fitted through mixture.solve with
nra_mixture_fit and the same start rows.  Both run the same fit body on the same points, so every comparison is bit
for bit; nra_mixture_fit against the numpy restatement is bounded by test_mixture_gpu.py."""
import functools
import os

import numpy as np
import pytest

from nanorepeat_amd import mixture, synth
from bootstrap_ref import composed_engine, limit_cases

pytestmark = pytest.mark.gpu

B = 8
MAX_N = 4
FIELDS = ("status", "order", "best_start", "lb", "w", "mu", "var")


def _problem(m, d, seed, max_n=MAX_N, centres=(18.0, 47.0)):
    rng = np.random.default_rng([seed, m, d])
    which = np.arange(m) % len(centres)
    x = np.stack([np.round(np.array(centres)[which] * (1 + 0.4 * a) + rng.standard_normal(m) * 0.8, 1)
                  for a in range(d)], axis=1)
    return mixture.Problem(x, 0.07, 0.15 if d == 1 else 0.1, max_n, seed)


@pytest.fixture(scope="module")
def problems():
    """m = 2, 10, 11, 51, 52 reads: N = 200, 1000, 1100, 5100, 5200 on both sides of both register-class borders."""
    return [_problem(m, d, 300 + 7 * m + d) for d in (1, 2) for m in (2, 10, 11, 51, 52)]


def _indices(ps, n_rep=B):
    return [mixture.resample_indices(p.seed, len(p.x), n_rep) for p in ps]


def _call(capi, ps, idx, n_caps=None, flags=0):
    n_caps = n_caps or [p.max_n for p in ps]
    return mixture._bootstrap_call(ps, n_caps, idx, len(idx[0]), functools.partial(capi.mixture_bootstrap, flags=flags), 0)


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in FIELDS)


@pytest.fixture(scope="module")
def composed(capi, problems):
    """The composed path's answer for every replicate, computed once and left unchanged."""
    return mixture._bootstrap_call(problems, [p.max_n for p in problems], _indices(problems), B,
                                   composed_engine(capi.mixture_fit), 0)


def test_device_search_equals_the_composed_path(capi, problems, composed):
    got = _call(capi, problems, _indices(problems))
    orders = set()
    for p, g, c in zip(problems, got, composed):
        assert (g["status"] == mixture.BOOT_DECIDED).all()
        for k in FIELDS:
            assert g[k].tobytes() == c[k].tobytes(), (len(p.x), p.x.shape[1], k)
        orders.update(int(o) for o in g["order"])
    assert len(orders) >= 2


def test_identity_resample_is_the_main_fit(capi, problems):
    for p in problems:
        mixture.solve([p], capi.mixture_fit)
    got = _call(capi, problems, [np.arange(len(p.x))[None, :] for p in problems])
    for p, g in zip(problems, got):
        n, model = p.answer
        assert int(g["order"][0]) == n
        if n > 1:
            assert int(g["best_start"][0]) == p.best_start[n] and g["lb"][0] == p.best_lb[n]
            assert g["w"][0, :n].tobytes() == model.weights_.tobytes()
            assert g["mu"][0, :n].tobytes() == np.ascontiguousarray(model.means_).tobytes()
            assert g["var"][0, :n].tobytes() == np.ascontiguousarray(model.covariances_).tobytes()


def test_path_and_order_invariance(capi, problems):
    idx = _indices(problems)
    base = _call(capi, problems, idx)
    for flags in (capi.MIX_STREAM, capi.MIX_ONE_CLASS):
        assert all(_same(a, b) for a, b in zip(_call(capi, problems, idx, flags=flags), base)), flags
    rev = _call(capi, problems[::-1], idx[::-1])
    assert all(_same(a, b) for a, b in zip(rev[::-1], base))
    for k in (1, 4, 8):                                           # one replicate of one problem alone in a call
        for b in (0, B - 1):
            alone = _call(capi, [problems[k]], [idx[k][b:b + 1]])[0]
            for f in FIELDS:
                assert alone[f][0].tobytes() == base[k][f][b].tobytes(), (k, b, f)


def test_needs_more_and_the_second_call(capi):
    p = _problem(24, 1, 41, max_n=6, centres=(20.0, 50.0, 90.0))
    idx = _indices([p])
    full = mixture._bootstrap_call([p], [6], idx, B, composed_engine(capi.mixture_fit), 0)[0]
    assert (full["status"] == mixture.BOOT_DECIDED).all() and (full["order"] > 2).any()
    capped = _call(capi, [p], idx, n_caps=[2])[0]
    # with start rows up to order 2 a replicate is decided only by an overlap at order 2: every order >= 2 needs more
    assert np.array_equal(capped["status"] == mixture.BOOT_NEEDS_MORE, full["order"] >= 2)
    assert np.array_equal(capped["status"] == mixture.BOOT_NEEDS_MORE, full["order"] > 2)      # none is exactly 2 here
    assert (capped["order"][capped["status"] == mixture.BOOT_NEEDS_MORE] == 0).all()
    assert _same(_call(capi, [p], idx, n_caps=[6])[0], full)
    # two alleles six units apart: replicates of orders 1, 2 and 3, so one call holds both statuses at either cap
    q = _problem(12, 1, 41, max_n=6, centres=(20.0, 26.0))
    qi = _indices([q])
    qfull = mixture._bootstrap_call([q], [6], qi, B, composed_engine(capi.mixture_fit), 0)[0]
    assert (qfull["status"] == mixture.BOOT_DECIDED).all() and {1, 2} <= set(int(o) for o in qfull["order"])
    for n_cap in (2, 3):
        part = _call(capi, [q], qi, n_caps=[n_cap])[0]
        more = part["status"] == mixture.BOOT_NEEDS_MORE
        assert np.array_equal(more, qfull["order"] >= n_cap) and more.any() and (~more).any(), n_cap
        for b in np.flatnonzero(~more):
            n = int(qfull["order"][b])
            assert all(part[k][b].tobytes() == qfull[k][b].tobytes() for k in ("order", "best_start", "lb"))
            assert all(part[k][b, :n].tobytes() == qfull[k][b, :n].tobytes() for k in ("w", "mu", "var"))
    assert _same(_call(capi, [q], qi, n_caps=[6])[0], qfull)
    # mixture.bootstrap makes both calls: the first with start rows up to the called order + 2 only
    mixture.solve([p], capi.mixture_fit)
    calls = []

    def engine(*args, **kw):
        calls.append(list(args[7]))
        return capi.mixture_bootstrap(*args, **kw)

    low = mixture.Problem(p.x, 0.07, 0.15, 6, p.seed)
    mixture.solve([low], capi.mixture_fit)
    low.answer = (1, low.answer[1])                               # as if one allele had been called: n_cap = 3
    got = mixture.bootstrap([low], B, engine)[0]
    assert calls == [[3], [6]] and _same(got, full)


def test_limits(capi):
    good, cases = limit_cases(capi.boot_start_rows)
    got = capi.mixture_bootstrap(**good)
    assert got["status"].shape == (1, 2) and (got["status"] == mixture.BOOT_NEEDS_MORE).sum() + \
        (got["status"] == mixture.BOOT_DECIDED).sum() == 2
    for change, code in cases:
        with pytest.raises(capi.NraError) as e:
            capi.mixture_bootstrap(**{**good, **change})
        assert e.value.code == code, change


# ---------------------------------------------------------------------------- end to end
def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_fastq_command_device_engine_equals_composed_engine(capi, tmp_path):
    from nanorepeat_amd import pipeline
    p = synth.panel(12, anchor_len=1000, reads_per_region=24, edge_overlaps=(300, 1000), n_decoys=24, seed=21)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont", anchor_len=1000, seed=3, mixture="gpu", bootstrap=16)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "gpu"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), bootstrap_engine=composed_engine(capi.mixture_fit),
                                 **common)
    assert (tmp_path / "gpu.NanoRepeat_bootstrap.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_bootstrap.tsv").read_bytes()
    assert (tmp_path / "gpu.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_output.tsv").read_bytes()
    got = _tree(tmp_path / "gpu.details")
    assert got == _tree(tmp_path / "ref.details")
    assert sum(n.endswith(".bootstrap.tsv") for n in got) >= 10
    table = [l.split("\t") for l in (tmp_path / "gpu.NanoRepeat_bootstrap.tsv").read_text().split("\n") if l]
    assert len(table) > 12 and all(len(r) == 13 for r in table) and all(r[10] in ("16", "-") for r in table[1:])


def test_degenerate_regions_come_out_as_on_the_cpu(capi):
    from nanorepeat_amd import pipeline
    from test_bootstrap_cpu import _region
    rr = _region(0, [30.0] * 12)
    pipeline.phase_regions([rr], seed=11, mixture="gpu", bootstrap=B)
    assert (rr.bootstrap.count == 1).all() and (rr.bootstrap.sizes[:, 0] == 30).all()
    assert rr.bootstrap.rows == [(30, 12, 30, 30, B)] and rr.bootstrap.support == 1.0
    rr = _region(0, [20.0] * 10 + [60.0] * 10)
    pipeline.phase_regions([rr], "hifi", seed=12, mixture="gpu", bootstrap=B)
    assert [a.repeat_size1 for a in rr.results.quantified_allele_list] == [20, 60]
    assert rr.bootstrap.rows == [(20, 10, 20, 20, B), (60, 10, 60, 60, B)] and rr.bootstrap.support == 1.0
