"""Data of the censored-fit tests: the five scenarios and the four-class panel of DESIGN.md section 26 as
censored.Problem objects, and the fit panel on which the device is compared with the restatement."""
import math

import numpy as np

from nanorepeat_amd import censored

TAU = 0.07               # data_type_error_rate of every data type
NOISE = 0.04             # the true read noise of the scenarios and the panel


def _reads(rng, allele, count, noise):
    """Sizes of `count` spanning reads of an allele: sd noise (10 + allele), rounded to whole units, not below 0."""
    x = allele + rng.standard_normal(count) * noise * (10.0 + allele)
    return [float(max(0.0, round(v))) for v in x]


def _bounds(rng, allele, count, noise=0.0):
    """What `count` reads that end inside an allele show: floor(U * allele), the allele itself read with `noise`."""
    out = []
    for _ in range(count):
        seen = allele + (rng.standard_normal() * noise * (10.0 + allele) if noise else 0.0)
        out.append(int(math.floor(rng.random() * seen)))
    return [c for c in out if c >= 1]


def problem(exact, bounds, tau=TAU):
    return censored.Problem([f"s{i}" for i in range(len(exact))], exact, [f"c{i}" for i in range(len(bounds))], bounds,
                            ["one_anchor"] * len(bounds), tau)


def scenarios(seed=11):
    """[(name, Problem, expected (n, o))]: the five scenarios, read noise 4 %, bounds floor(U * allele)."""
    rng = np.random.default_rng(seed)
    short = _reads(rng, 20, 30, NOISE)
    return [
        ("minority_spanned", problem(short + _reads(rng, 150, 2, NOISE), _bounds(rng, 150, 25)), (2, 0)),
        ("unspanned_800", problem(short, _bounds(rng, 800, 25)), (1, 1)),
        ("homozygous_with_bounds", problem(short, _bounds(rng, 20, 8)), (1, 0)),
        ("two_alleles_no_bounds", problem(_reads(rng, 20, 15, NOISE) + _reads(rng, 32, 15, NOISE), []), (2, 0)),
        ("two_spanned_one_unspanned", problem(_reads(rng, 20, 15, NOISE) + _reads(rng, 45, 15, NOISE),
                                              _bounds(rng, 600, 25)), (2, 1)),
    ]


PANEL_CLASSES = ("homozygous_with_bounds", "unspanned_long", "long_spanned_by_two", "two_spanned")
PANEL_EXPECTED = {"homozygous_with_bounds": (1, 0), "unspanned_long": (1, 1), "long_spanned_by_two": (2, 0),
                  "two_spanned": (2, 0)}


def panel(seed=2026, per_class=100, noise=NOISE):
    """[(class, Problem)]: per_class regions of each class; the bounds carry the reads' noise."""
    rng = np.random.default_rng(seed)
    out = []
    for cls in PANEL_CLASSES:
        for _ in range(per_class):
            a = int(rng.integers(10, 61))
            n_short = int(rng.integers(20, 41))
            if cls == "homozygous_with_bounds":
                exact, bounds = _reads(rng, a, n_short, noise), _bounds(rng, a, int(rng.integers(6, 16)), noise)
            elif cls == "unspanned_long":
                long_ = int(rng.integers(300, 1001))
                exact = _reads(rng, a, n_short, noise)
                bounds = _bounds(rng, long_, int(rng.integers(15, 31)), noise) + _bounds(rng, a, int(rng.integers(0, 6)), noise)
            elif cls == "long_spanned_by_two":
                long_ = int(rng.integers(150, 1001))
                exact = _reads(rng, a, n_short, noise) + _reads(rng, long_, 2, noise)
                bounds = _bounds(rng, long_, int(rng.integers(15, 31)), noise)
            else:
                b = int(round(a * rng.uniform(1.6, 3.0))) + 8
                exact = _reads(rng, a, n_short // 2 + 3, noise) + _reads(rng, b, n_short // 2 + 3, noise)
                bounds = _bounds(rng, a, int(rng.integers(0, 6)), noise) + _bounds(rng, b, int(rng.integers(0, 8)), noise)
            out.append((cls, problem(exact, bounds)))
    return out


def call_counts(cases, engine, **kw):
    """{class: regions called as expected} of a panel."""
    fits = censored.fit_problems([pr for _, pr in cases], engine=engine, **kw)
    counts = {c: 0 for c in PANEL_CLASSES}
    for (cls, _), cf in zip(cases, fits):
        counts[cls] += (cf.n, cf.open) == PANEL_EXPECTED[cls]
    return counts


# ------------------------------------------------------------------ the fit panel (device against restatement)
FIT_SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 3000)       # lane and register-class borders
FIT_SEED = 1


def fit_panel(seed=FIT_SEED):
    """Problems and fits as the arguments of censored_fit: for every N of FIT_SIZES, problems with m from 1 to N exact
    values of two or three alleles and bounds of the longest one; on every problem orders 1..4, open 0 and 1 (where it
    has a bound), three starts.  A problem takes a share of these fits, a large one a smaller share: the restatement
    calls math.erfc per bound, component and iteration."""
    rng = np.random.default_rng(seed)
    values, off, n_pts, n_exact, taus = [], [], [], [], []
    fit_problem, fit_n, fit_open, starts = [], [], [], []
    for N in FIT_SIZES:
        for m in sorted({1, max(1, N // 3), max(1, N - 1), N}):
            alleles = [20.0, 55.0, 140.0][:int(rng.integers(2, 4))]
            exact = [max(0.0, round(alleles[int(rng.integers(0, len(alleles)))] * (1 + 0.05 * rng.standard_normal())))
                     for _ in range(m)]
            top = 600 if N <= 65 and len(off) % 4 == 1 else 140          # some problems have bounds beyond every allele
            bounds = [max(1, int(rng.random() * top)) for _ in range(N - m)]
            y = [censored.log_size(x) for x in exact] + [censored.log_size(c) for c in bounds]
            p = len(off)
            off.append(len(values)); values += y
            n_pts.append(N); n_exact.append(m); taus.append((0.07, 0.05, 0.1)[p % 3])
            combos = [(n, o, t) for n in range(1, 5) for o in ((0, 1) if N > m else (0,)) for t in range(3)]
            share = 6 if N > 65 else 3                         # every order, switch and start, spread over the problems
            combos = [c for i, c in enumerate(combos) if (i + p) % share == 0]
            for n, o, t in combos:
                fit_problem.append(p); fit_n.append(n); fit_open.append(o)
                starts += censored.start_means(y[:m], y[m:], n)[t]
    return dict(values=np.array(values), prob_off=np.array(off, np.int64), prob_n=np.array(n_pts, np.int32),
                prob_n_exact=np.array(n_exact, np.int32), prob_tau=np.array(taus),
                fit_problem=np.array(fit_problem, np.int32), fit_n=np.array(fit_n, np.int32),
                fit_open=np.array(fit_open, np.int32), starts=np.array(starts))


def margin_ok(traces, tol=1e-9, rel=1e-3):
    """No fit's last |lb - lb of the E-step before| lies within `rel` (relative) of tol: the device, whose lb differs in
    the last bits, takes the same decision at that E-step."""
    return all(len(tr) < 2 or abs(abs(tr[-1] - tr[-2]) - tol) > rel * tol for tr in traces)
