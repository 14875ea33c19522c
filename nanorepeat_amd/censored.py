"""Censored allele fit (no counterpart in the reference): the sizes of the spanning reads and the
lower bounds of the reads that end inside the repeat in one mixture likelihood.

A one-anchor read (partial.py, `Min_Repeat_Size`) or an in-repeat read (`Repeat_Units`) shows at least so many units: a
right-censored observation of the allele it came from.  Per region, in the variance-stabilised domain y = ln(10 + size)
where the project's error model sd = e (10 + size) is a constant tau = e:

* exact observations: the round-3 size of every spanning read that has one (no outlier cut);
* censored observations: every bound >= 1;
* a model (n, o): n closed components N(nu_k, tau^2), and with o = 1 one open component that explains bounds only -- an
  allele no read spans (a closed component without an exact read has no finite maximum-likelihood mean).

Every (n, o) with n = 1 .. min(max_alleles, distinct exact values) and o in {0, 1} (o = 0 alone without bounds) is fitted
by EM from three starts (`start_means`), all fits of all regions in one `nra_censored_fit` call; the best start per model
is the largest ll (ties: the lowest start), the model the smallest BIC = -2 ll + (2 n + o - 1) ln N (within 1e-9: fewer
parameters, then o = 0); one `nra_censored_posteriors` call then gives every read's posterior per allele.  A region
without a spanning read is not fitted: 0 closed alleles, and an open one when it has a bound.

`censored_regions` fills `region.censored_fit`; `write_censored_fit`, `write_censored_reads` and
`write_censored_summary` write `<region>.censored_fit.tsv`, `<region>.censored_reads.tsv` and
`<out_prefix>.NanoRepeat_censored.tsv`; `report_censored_calls` prints one NOTICE.

`censored_bootstrap=B` resamples every region's reads B times, spanning reads and bounds jointly,
and runs the whole model search of every replicate in one `nra_censored_bootstrap` call: `bootstrap_problems` builds
the sorted layouts and the index rows and computes, in numpy over a region's replicates, how often the called model
comes back (`Model_Support`), how often an open allele does (`Open_Support`) and the percentile interval of every
called allele's size and weight; `write_censored_bootstrap` and `write_censored_bootstrap_summary` write
`<region>.censored_bootstrap.tsv` and `<out_prefix>.NanoRepeat_censored_bootstrap.tsv`.  Nothing is thresholded.
"""
import math
import sys

import numpy as np

MAX_ALLELES = 6          # censored_max_alleles
MAX_ITER = 500
TOL = 1e-9
BIC_TIE = 1e-9


def log_size(x):
    """The variance-stabilised domain: sd e (10 + x) of a size x becomes a constant sd e."""
    return math.log(10.0 + x)


def quant(a, k, n):
    """Element floor((k + 0.5) / n * L), at most L - 1, of the sorted array a of length L."""
    return a[min(len(a) - 1, int(math.floor((k + 0.5) / n * len(a))))]


def start_means(exact, censored, n):
    """The three starts of order n, pure functions of the data: quantiles of the exact values; quantiles of all values;
    n - 1 quantiles of the exact values and the largest value of all."""
    e = sorted(exact)
    pooled = sorted(list(exact) + list(censored))
    return [[quant(e, k, n) for k in range(n)],
            [quant(pooled, k, n) for k in range(n)],
            [quant(e, k, n - 1) for k in range(n - 1)] + [pooled[-1]]]


def models_of(n_distinct, q, max_alleles=MAX_ALLELES):
    """The (n, o) fitted for a region with n_distinct distinct exact values and q bounds."""
    return [(n, o) for n in range(1, min(max_alleles, n_distinct) + 1) for o in ((0, 1) if q else (0,))]


def bic_of(ll, n, o, n_points):
    return -2.0 * ll + (2 * n + o - 1) * math.log(n_points)


def choose_model(bics):
    """bics: {(n, o): BIC} -> the (n, o) of the smallest BIC; within 1e-9 fewer parameters win, then o = 0."""
    lowest = min(bics.values())
    return min((no for no, b in bics.items() if b <= lowest + BIC_TIE), key=lambda no: (2 * no[0] + no[1], no[1]))


class Problem:
    """What one region hands to the fit: names and values of its exact and censored observations."""

    def __init__(self, exact_names, exact_sizes, cens_names, cens_bounds, cens_kinds, tau):
        self.exact_names, self.exact_sizes = list(exact_names), [float(x) for x in exact_sizes]
        self.cens_names, self.cens_bounds, self.cens_kinds = list(cens_names), [int(c) for c in cens_bounds], list(cens_kinds)
        self.tau = float(tau)
        self.y = [log_size(x) for x in self.exact_sizes] + [log_size(c) for c in self.cens_bounds]

    @property
    def m(self):
        return len(self.exact_sizes)

    @property
    def q(self):
        return len(self.cens_bounds)


class CensoredFit:
    """The call of one region: n closed alleles sorted by size and `open`; per allele its weight; the posteriors of the
    exact reads [m, n + open] and of the censored reads [q, n + open] (the open column last); the BIC of every model."""

    def __init__(self, problem):
        self.problem = problem
        self.n, self.open = 0, int(problem.m == 0 and problem.q > 0)
        self.nu, self.w, self.bics, self.ll = [], [], {}, None
        self.resp_exact = np.zeros((problem.m, 0))
        self.resp_cens = np.zeros((problem.q, 0))

    def sizes(self):
        return [math.exp(v) - 10.0 for v in self.nu]

    def open_min_size(self):
        """The largest bound among the reads whose open posterior is > 0.5 (every bound when nothing was fitted)."""
        if not self.open:
            return None
        if self.problem.m == 0:
            return max(self.problem.cens_bounds)
        mine = [c for c, r in zip(self.problem.cens_bounds, self.resp_cens[:, -1]) if r > 0.5]
        return max(mine) if mine else None

    def allele_rows(self):
        """(allele id, kind, size, median spanning size, weight, spanning reads, censored reads, min size) per allele."""
        rows = []
        pr = self.problem
        label = self.resp_exact.argmax(axis=1) if self.n and pr.m else np.zeros(0, int)
        for k in range(self.n):
            mine = [x for x, l in zip(pr.exact_sizes, label) if l == k]
            rows.append((k + 1, "closed", self.sizes()[k], float(np.median(mine)) if mine else None, self.w[k], len(mine),
                         float(self.resp_cens[:, k].sum()) if pr.q else 0.0, None))
        if self.open:
            fitted = pr.m > 0
            rows.append((self.n + 1, "open", None, None, self.w[-1] if fitted else None, 0,
                         float(self.resp_cens[:, -1].sum()) if fitted else float(pr.q), self.open_min_size()))
        return rows


def region_problem(region, tau, use_partial=True, use_in_repeat=True):
    exact = [(name, r.round3_repeat_size) for name, r in region.read_dict.items() if r.round3_repeat_size is not None]
    cens = []
    if use_partial:
        cens += [(name, pr.min_repeat_size, "one_anchor")
                 for name, pr in (getattr(region, "partial_reads", None) or {}).items()]
    if use_in_repeat:
        cens += [(name, ir.repeat_units, "in_repeat")
                 for name, ir in (getattr(region, "in_repeat_reads", None) or {}).items()]
    cens = [c for c in cens if c[1] is not None and c[1] >= 1]
    return Problem([n for n, _ in exact], [x for _, x in exact], [c[0] for c in cens], [c[1] for c in cens],
                   [c[2] for c in cens], tau)


def fit_problems(problems, max_alleles=MAX_ALLELES, engine=None, device=0):
    """The calls of `problems` (Problem objects): one engine.censored_fit call for every fit of every problem with an
    exact value, the BIC rule, one engine.censored_posteriors call.  `engine`: an object with censored_fit and
    censored_posteriors (default _capi; tests pass the restatement).  Returns one CensoredFit per problem."""
    if engine is None:
        from . import _capi
        engine = _capi
    if not 1 <= max_alleles <= 8:
        raise ValueError(f"censored_max_alleles must be in 1..8, not {max_alleles!r}")
    fits = [CensoredFit(pr) for pr in problems]
    live = [i for i, pr in enumerate(problems) if pr.m > 0]
    if not live:
        return fits
    values, off, n_pts, n_exact, taus = [], [], [], [], []
    fit_problem, fit_n, fit_open, starts, owner = [], [], [], [], []
    for p, i in enumerate(live):
        pr = problems[i]
        off.append(len(values)); values += pr.y
        n_pts.append(pr.m + pr.q); n_exact.append(pr.m); taus.append(pr.tau)
        for n, o in models_of(len(set(pr.exact_sizes)), pr.q, max_alleles):
            for t, st in enumerate(start_means(pr.y[:pr.m], pr.y[pr.m:], n)):
                fit_problem.append(p); fit_n.append(n); fit_open.append(o); starts += st
                owner.append((n, o, t))
    out = engine.censored_fit(np.array(values), np.array(off, np.int64), np.array(n_pts, np.int32),
                              np.array(n_exact, np.int32), np.array(taus), np.array(fit_problem, np.int32),
                              np.array(fit_n, np.int32), np.array(fit_open, np.int32), np.array(starts),
                              max_iter=MAX_ITER, tol=TOL, device=device)
    best_of = [dict() for _ in live]                     # (n, o) -> the fit with the largest ll, ties to the lowest t
    for f, (n, o, t) in enumerate(owner):
        cur = best_of[fit_problem[f]].get((n, o))
        if cur is None or out["ll"][f] > out["ll"][cur]:
            best_of[fit_problem[f]][(n, o)] = f
    model_n, model_open, w, nu, order_of = [], [], [], [], []
    for p, i in enumerate(live):
        cf, pr = fits[i], problems[i]
        cf.bics = {no: bic_of(float(out["ll"][f]), no[0], no[1], pr.m + pr.q) for no, f in best_of[p].items()}
        n, o = choose_model(cf.bics)
        f = best_of[p][(n, o)]
        f_nu = out["nu"][out["nu_off"][f]:out["nu_off"][f] + n]
        f_w = out["w"][out["w_off"][f]:out["w_off"][f] + n + o]
        order = sorted(range(n), key=lambda k: (f_nu[k], k))              # closed alleles by size
        cf.n, cf.open, cf.ll = n, o, float(out["ll"][f])
        cf.nu = [float(f_nu[k]) for k in order]
        cf.w = [float(f_w[k]) for k in order] + ([float(f_w[n])] if o else [])
        model_n.append(n); model_open.append(o); w += cf.w; nu += cf.nu
    resp = engine.censored_posteriors(np.array(values), np.array(off, np.int64), np.array(n_pts, np.int32),
                                      np.array(n_exact, np.int32), np.array(taus), np.array(model_n, np.int32),
                                      np.array(model_open, np.int32), np.array(w), np.array(nu), device=device)
    for p, i in enumerate(live):
        m = problems[i].m
        fits[i].resp_exact, fits[i].resp_cens = np.asarray(resp[p][:m]), np.asarray(resp[p][m:])
    return fits


def censored_regions(repeat_regions, data_type="ont", error_rate=None, max_alleles=MAX_ALLELES, use_partial=True,
                     use_in_repeat=True, engine=None, device=0):
    """Sets `region.censored_fit` (a CensoredFit) for every region and returns the regions.  error_rate: tau (None: the
    data type's error rate, as the phasing step uses it)."""
    from . import phasing
    tau = phasing.data_type_error_rate(data_type) if error_rate is None else float(error_rate)
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"censored_error_rate must be finite and > 0, not {error_rate!r}")
    problems = [region_problem(region, tau, use_partial, use_in_repeat) for region in repeat_regions]
    for region, cf in zip(repeat_regions, fit_problems(problems, max_alleles, engine, device)):
        region.censored_fit = cf
    return repeat_regions


def _f(v, fmt):
    return "-" if v is None else format(v, fmt)


def censored_fit_text(region):
    cf = region.censored_fit
    pr = cf.problem
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Tau={pr.tau:g}\n", f"##Num_Spanning={pr.m}\n",
             f"##Num_Censored={pr.q}\n"]
    lines += [f"##BIC(n={n},open={o})={b:.6f}\n" for (n, o), b in sorted(cf.bics.items())]
    lines.append("#Allele\tKind\tSize\tMedian_Spanning_Size\tWeight\tSpanning_Reads\tCensored_Reads\tMin_Size\n")
    for a, kind, size, med, w, ns, nc, min_size in cf.allele_rows():
        lines.append(f"{a}\t{kind}\t{_f(size, '.1f')}\t{_f(med, '.1f')}\t{_f(w, '.4f')}\t{ns}\t{nc:.2f}\t"
                     f"{_f(min_size, 'd')}\n")
    return "".join(lines)


def censored_reads_text(region):
    cf = region.censored_fit
    pr = cf.problem
    nc = cf.n + cf.open
    names = [f"P_Allele{k + 1}" for k in range(nc)]
    lines = [f"##RepeatRegion={region.to_unique_id()}\n",
             "\t".join(["#Read_Name", "Kind", "Min_Size"] + names) + "\n"]
    for i in sorted(range(pr.q), key=lambda i: (-pr.cens_bounds[i], pr.cens_names[i])):
        post = cf.resp_cens[i] if pr.m else ([1.0] if cf.open else [])
        lines.append("\t".join([pr.cens_names[i], pr.cens_kinds[i], str(pr.cens_bounds[i])] +
                               [f"{float(r):.4f}" for r in post]) + "\n")
    return "".join(lines)


def write_censored_fit(region):
    """`<region out_prefix>.censored_fit.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix or getattr(region, "censored_fit", None) is None:
        return None
    path = f"{region.out_prefix}.censored_fit.tsv"
    with open(path, "w") as f:
        f.write(censored_fit_text(region))
    return path


def write_censored_reads(region):
    """`<region out_prefix>.censored_reads.tsv` (not with no_details)."""
    if region.no_details or not region.out_prefix or getattr(region, "censored_fit", None) is None:
        return None
    path = f"{region.out_prefix}.censored_reads.tsv"
    with open(path, "w") as f:
        f.write(censored_reads_text(region))
    return path


SUMMARY_HEADER = ("#Chrom\tStart\tEnd\tMotif\tNum_Spanning\tNum_Censored\tNum_Alleles_Standard\tNum_Closed\tOpen\tSizes\t"
                  "Weights\tOpen_Min_Size\tDiffers\n")


def _standard_alleles(region):
    from . import phasing
    return len(phasing.results_of(region).quantified_allele_list)


def censored_summary_row(region):
    head = f"{region.chrom}\t{max(0, region.start_pos)}\t{region.end_pos}\t{region.repeat_unit_seq}\t"
    cf = getattr(region, "censored_fit", None)
    std = _standard_alleles(region)
    if cf is None:
        return head + f"0\t0\t{std}\t0\t0\t-\t-\t-\t{int(std != 0)}\n"
    sizes = ",".join(f"{s:.1f}" for s in cf.sizes()) or "-"
    weights = ",".join(f"{w:.4f}" for w in cf.w) or "-"
    return head + (f"{cf.problem.m}\t{cf.problem.q}\t{std}\t{cf.n}\t{cf.open}\t{sizes}\t{weights}\t"
                   f"{_f(cf.open_min_size(), 'd')}\t{int(cf.n != std)}\n")


def write_censored_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_censored.tsv`: one row per BED region, in BED order."""
    path = f"{out_prefix}.NanoRepeat_censored.tsv"
    with open(path, "w") as f:
        f.write(SUMMARY_HEADER)
        f.write("".join(censored_summary_row(region) for region in regions))
    return path


def report_censored_calls(regions, stream=None):
    """One NOTICE counting the regions with an open allele and the regions whose number of closed alleles differs from
    the standard call.  Returns (regions with an open allele, regions that differ)."""
    stream = stream or sys.stderr
    fits = [(r, r.censored_fit) for r in regions if getattr(r, "censored_fit", None) is not None]
    n_open = sum(cf.open for _, cf in fits)
    n_diff = sum(cf.n != _standard_alleles(r) for r, cf in fits)
    if n_open or n_diff:
        print(f"NOTICE: censored fit: {n_open} region(s) have an open allele (an allele no read spans); in {n_diff} "
              "region(s) the number of closed alleles differs from the standard call", file=stream)
    return n_open, n_diff


# ---------------------------------------------------------------------------- bootstrap
BOOT_SALT = 0x63656E73                # "cens": keeps these draws apart from every other stream of (seed, region)
BOOT_FITTED, BOOT_NO_EXACT = 0, 1     # NRA_CENS_BOOT_FITTED, NRA_CENS_BOOT_NO_EXACT


def sorted_layout(problem):
    """The values of a problem as the bootstrap reads them: the exact ones ascending, then the bounds ascending."""
    return sorted(problem.y[:problem.m]) + sorted(problem.y[problem.m:])


def resample_rows(seed, region_index, m, n_points, n_rep):
    """(idx [n_rep, N] int32, rep_m [n_rep] int32): N draws from all N observations per replicate, every row sorted, so
    that a replicate's first rep_m positions are exact values in order and the others bounds in order."""
    rng = np.random.default_rng([int(seed), int(region_index), BOOT_SALT])
    idx = np.sort(rng.integers(0, n_points, size=(n_rep, n_points)), axis=1).astype(np.int32)
    return idx, (idx < m).sum(axis=1).astype(np.int32)


def percentile_interval(values, confidence):
    """Section 24's nearest-rank interval (bootstrap.percentile_interval) of r values; None for r = 0."""
    from .bootstrap import percentile_interval as interval
    return interval(values, confidence)


class CensoredBootstrap:
    """The bootstrap of one region against its call `fit` (a CensoredFit with m >= 1).  Per replicate: `num_spanning`,
    `n`, `open`, and `nu`, `w` [B, n] of its closed alleles by size (ties by index, as fit_problems ranks them; padded
    with nan) and `w_open` (nan without one, and for a replicate that was not fitted).  Against the call: `model_support`, `open_support`, `distribution`, and
    `rows`: per called allele (kind, size CI low, size CI high, weight low, weight high, replicates used)."""

    def __init__(self, seed, num_spanning, n, open_, nu, w, fit, confidence):
        self.seed = seed
        self.num_spanning, self.n, self.open = (np.asarray(v, np.int64) for v in (num_spanning, n, open_))
        B = self.n_replicates = len(self.n)
        nu, w = np.asarray(nu, np.float64).reshape(B, -1), np.asarray(w, np.float64).reshape(B, -1)
        C = nu.shape[1]
        closed = np.arange(C)[None, :] < self.n[:, None]
        order = np.argsort(np.where(closed, nu, np.inf), axis=1, kind="stable")
        self.nu = np.where(closed, np.take_along_axis(nu, order, axis=1), np.nan)
        self.w = np.where(closed, np.take_along_axis(w[:, :C], order, axis=1), np.nan)
        at_n = np.take_along_axis(w, np.minimum(self.n, w.shape[1] - 1)[:, None], axis=1)[:, 0]
        self.w_open = np.where((self.open == 1) & (self.n > 0), at_n, np.nan)
        same_n = self.n == fit.n
        same = same_n & (self.open == fit.open)
        self.model_support = float(same.sum()) / B
        self.open_support = float((self.open == 1).sum()) / B
        models, tally = np.unique(np.stack([self.open, self.n], axis=1), axis=0, return_counts=True)
        self.distribution = ",".join(f"{int(n_)}+{int(o)}:{int(c)}" for (o, n_), c in zip(models, tally))
        self.rows = []
        for k in range(fit.n):
            size = percentile_interval(np.exp(self.nu[same_n, k]) - 10.0, confidence)
            weight = percentile_interval(self.w[same_n, k], confidence)
            self.rows.append(("closed",) + (size or (None, None)) + (weight or (None, None)) + (int(same_n.sum()),))
        if fit.open:
            weight = percentile_interval(self.w_open[same], confidence)
            self.rows.append(("open", None, None) + (weight or (None, None)) + (int(same.sum()),))


def bootstrap_problems(problems, fits, n_rep, seed, confidence=0.95, max_alleles=MAX_ALLELES, engine=None, device=0,
                       indices=None):
    """One CensoredBootstrap per problem (None where it has no exact value): the sorted layouts, index rows, rep_m and
    lnN of all problems with m >= 1, one engine.censored_bootstrap call, the statistics in numpy over the replicates of
    a region.  `fits`: fit_problems' result; `indices`: every problem's region index (default: its place in the list),
    which with `seed` names its random stream; `engine`: an object with censored_bootstrap (default _capi)."""
    if engine is None:
        from . import _capi
        engine = _capi
    if not 1 <= max_alleles <= 8:
        raise ValueError(f"censored_max_alleles must be in 1..8, not {max_alleles!r}")
    if n_rep < 1 or int(n_rep) != n_rep:
        raise ValueError(f"censored_bootstrap must be a number of replicates >= 1 here, not {n_rep!r}")
    n_rep = int(n_rep)
    indices = list(range(len(problems))) if indices is None else list(indices)
    out = [None] * len(problems)
    live = [i for i, pr in enumerate(problems) if pr.m > 0]
    if not live:
        return out
    values, off, rows, rep_m = [], [], [], []
    for i in live:
        pr = problems[i]
        off.append(len(values)); values += sorted_layout(pr)
        idx, m_b = resample_rows(seed, indices[i], pr.m, pr.m + pr.q, n_rep)
        rows.append(idx.ravel()); rep_m.append(m_b)
    n_pts = [problems[i].m + problems[i].q for i in live]
    rep = engine.censored_bootstrap(np.array(values), np.array(off, np.int64), np.array(n_pts, np.int32),
                                    np.array([problems[i].m for i in live], np.int32),
                                    np.array([problems[i].tau for i in live]), np.array([math.log(n) for n in n_pts]),
                                    n_rep, np.concatenate(rows), np.stack(rep_m), max_alleles, max_iter=MAX_ITER, tol=TOL,
                                    device=device)
    for p, i in enumerate(live):
        out[i] = CensoredBootstrap(seed, rep_m[p], rep["model_n"][p], rep["model_open"][p], rep["nu"][p], rep["w"][p],
                                   fits[i], confidence)
    return out


def bootstrap_regions(repeat_regions, n_rep, seed, confidence=0.95, max_alleles=MAX_ALLELES, engine=None, device=0):
    """Sets `region.censored_bootstrap` (a CensoredBootstrap, or None without a fit or a spanning read) for every region
    that censored_regions has been through."""
    with_fit = [r for r in repeat_regions if getattr(r, "censored_fit", None) is not None]
    boots = bootstrap_problems([r.censored_fit.problem for r in with_fit], [r.censored_fit for r in with_fit], n_rep,
                               seed, confidence, max_alleles, engine, device, [r.index for r in with_fit])
    for region in repeat_regions:
        region.censored_bootstrap = None
    for region, boot in zip(with_fit, boots):
        region.censored_bootstrap = boot
    return repeat_regions


def censored_bootstrap_text(region):
    boot = region.censored_bootstrap
    lines = [f"##RepeatRegion={region.to_unique_id()}\n", f"##Seed={boot.seed}\n",
             "#Replicate\tNum_Spanning\tNum_Closed\tOpen\tSizes\tWeights\n"]
    for b in range(boot.n_replicates):
        n, o = int(boot.n[b]), int(boot.open[b])
        sizes = ",".join(f"{math.exp(v) - 10.0:.1f}" for v in boot.nu[b, :n]) or "-"
        weights = ",".join([f"{v:.4f}" for v in boot.w[b, :n]] + ([f"{boot.w_open[b]:.4f}"] if n and o else [])) or "-"
        lines.append(f"{b}\t{int(boot.num_spanning[b])}\t{n}\t{o}\t{sizes}\t{weights}\n")
    return "".join(lines)


def write_censored_bootstrap(region):
    """`<region out_prefix>.censored_bootstrap.tsv`: the model of every replicate (not with no_details)."""
    if region.no_details or not region.out_prefix or getattr(region, "censored_bootstrap", None) is None:
        return None
    path = f"{region.out_prefix}.censored_bootstrap.tsv"
    with open(path, "w") as f:
        f.write(censored_bootstrap_text(region))
    return path


BOOT_HEADER = ("#Chrom\tStart\tEnd\tMotif\tAllele\tKind\tSize\tWeight\tCI_Low\tCI_High\tWeight_Low\tWeight_High\t"
               "Replicates_Used\tNum_Replicates\tModel_Support\tOpen_Support\tModel_Distribution\n")
BOOT_FIELDS = 17


def censored_bootstrap_rows(region):
    head = f"{region.chrom}\t{max(0, region.start_pos)}\t{region.end_pos}\t{region.repeat_unit_seq}"
    boot = getattr(region, "censored_bootstrap", None)
    if boot is None:
        return head + "\t-" * (BOOT_FIELDS - 4) + "\n"
    cf = region.censored_fit
    out = []
    for a, (kind, lo, hi, w_lo, w_hi, used) in enumerate(boot.rows):
        size = cf.sizes()[a] if kind == "closed" else None
        out.append(f"{head}\t{a + 1}\t{kind}\t{_f(size, '.1f')}\t{cf.w[a]:.4f}\t{_f(lo, '.1f')}\t{_f(hi, '.1f')}\t"
                   f"{_f(w_lo, '.4f')}\t{_f(w_hi, '.4f')}\t{used}\t{boot.n_replicates}\t{boot.model_support:.4f}\t"
                   f"{boot.open_support:.4f}\t{boot.distribution}\n")
    return "".join(out)


def write_censored_bootstrap_summary(regions, out_prefix):
    """`<out_prefix>.NanoRepeat_censored_bootstrap.tsv`: one row per (region, called allele), in BED order; a region
    without a fit gets one row of `-`."""
    path = f"{out_prefix}.NanoRepeat_censored_bootstrap.tsv"
    with open(path, "w") as f:
        f.write(BOOT_HEADER)
        f.write("".join(censored_bootstrap_rows(region) for region in regions))
    return path


def report_censored_bootstrap(regions, stream=None):
    """One NOTICE counting the regions whose called model has less than half of the replicates.  Returns the count."""
    stream = stream or sys.stderr
    boots = [b for b in (getattr(r, "censored_bootstrap", None) for r in regions) if b is not None]
    weak = sum(b.model_support < 0.5 for b in boots)
    if weak:
        print(f"NOTICE: censored bootstrap: in {weak} of {len(boots)} region(s) fewer than half of the replicates give the "
              "called model", file=stream)
    return weak
