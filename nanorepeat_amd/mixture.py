"""The mixture fits of step 4 on the GPU (`mixture="gpu"`): the reference's procedure
(phasing.py) with its optimiser replaced.  scikit-learn's k-means-initialised, randomly restarted EM becomes a fully
specified EM whose starts are a pure function of the seed, and the fits of every region run in one call of
`nra_mixture_fit` per window of model orders.  What stays the reference's: the outlier cut, the simulated sample, the
model order by the overlap rule, the classification of the real sizes, confidences, noisy-allele removal and every
file -- `phasing.phase` runs them unchanged with a `Fitter` in place of `phasing.auto_gmm`.

Host side of the contract:
* sample of a problem with kept sizes x (m reads x d axes), error rate e, seed s:
  z = default_rng(s).standard_normal(100 m d), X[c m d + i] = x_flat[i] + z[c m d + i] e (10 + x_flat[i]), N = 100 m
  rows (the copy-major order of phasing.simulate_reads);
* start t (0 <= t < 10) of order n: the rows default_rng([s, n, t]).choice(N, size=n, replace=False);
* the best fit of order n is the start with the largest lb (ties: the lowest t); order 1 is the closed form;
* orders as in phasing.auto_gmm: stop at the first n with two components whose central intervals
  mu +- z_o max(1, sd) overlap on every axis; the answer is the fit of order n - 1 already made.
The joint mode's restart on the surviving reads (restart r >= 1) draws its sample from default_rng([s, r]) and its
starts from default_rng([s, n, t, r]).  Neither scikit-learn nor scipy is imported here."""
import math
import statistics

import numpy as np

from . import phasing

N_STARTS = 10
WINDOW = 2                 # model orders fitted per call for every problem that has not stopped
ENGINES = ("sklearn", "gpu")


def check_engine_name(mixture):
    if mixture not in ENGINES:
        raise ValueError(f"mixture must be one of {ENGINES}, not {mixture!r}")


def fresh_seed():
    """What `seed=None` becomes, once per command."""
    return int(np.random.SeedSequence().entropy % (1 << 62))


def _key(seed, restart, *more):
    key = [int(seed)] + [int(v) for v in more]
    return key + [int(restart)] if restart else key


def noise(n_values, seed, restart=0):
    """The noise of a problem whose kept sizes are n_values numbers (m d): one standard normal per value of its sample."""
    rng = np.random.default_rng(_key(seed, restart) if restart else int(seed))
    return rng.standard_normal(phasing.SIM_COPIES * n_values)


def sample(x, error_rate, seed, restart=0, z=None):
    """x: the kept sizes [m, d] -> the simulated sample [100 m, d] (z: its noise, when the caller has drawn it)."""
    x = np.ascontiguousarray(x, np.float64)
    flat = x.ravel()
    if z is None:
        z = noise(flat.size, seed, restart)
    tiled = np.tile(flat, phasing.SIM_COPIES)
    return (tiled + z * error_rate * (10 + tiled)).reshape(-1, x.shape[1])


def start_rows(seed, n, t, N, restart=0):
    return np.random.default_rng(_key(seed, restart, n, t)).choice(N, size=n, replace=False).astype(np.int32)


class FittedMixture:
    """What phasing.create_allele_list needs of a fitted mixture, in numpy."""

    def __init__(self, weights, means, covariances):
        self.weights_ = np.asarray(weights, np.float64)
        self.means_ = np.asarray(means, np.float64)
        self.covariances_ = np.asarray(covariances, np.float64)
        self.n_components = len(self.weights_)

    def _log_joint(self, X):
        X = np.asarray(X, np.float64)
        d = X.shape[1]
        a = np.log(self.weights_) - 0.5 * (d * math.log(2 * math.pi) + np.log(self.covariances_).sum(axis=1))
        e = X[:, None, :] - self.means_[None, :, :]
        return a[None, :] - 0.5 * (e * e / self.covariances_[None, :, :]).sum(axis=2)

    def predict_proba(self, X):
        lj = self._log_joint(X)
        m = lj.max(axis=1, keepdims=True)
        p = np.exp(lj - m)
        return p / p.sum(axis=1, keepdims=True)

    def predict(self, X):
        return self._log_joint(X).argmax(axis=1)


def one_component(X):
    """Order 1 in closed form: the M-step on responsibilities of 1."""
    nk = len(X) + 10 * np.finfo(np.float64).eps
    mu = X.sum(axis=0) / nk
    var = (X * X).sum(axis=0) / nk - mu * mu + 1e-6
    return FittedMixture([nk / len(X)], [mu], [var])


def overlap_z(overlap):
    """The half width, in standard deviations, of the central interval that leaves `overlap` outside on each side."""
    return statistics.NormalDist().inv_cdf(1.0 - overlap)


def components_overlap(model, overlap, z=None):
    """phasing.auto_gmm's stop test on a fitted mixture (z: overlap_z(overlap), when the caller has it)."""
    if z is None:
        z = overlap_z(overlap)
    n, d = model.means_.shape
    iv = [[(model.means_[c][a] - z * max(1.0, math.sqrt(model.covariances_[c][a])),
            model.means_[c][a] + z * max(1.0, math.sqrt(model.covariances_[c][a]))) for a in range(d)] for c in range(n)]
    return any(all(phasing.interval_has_overlap(iv[i][a], iv[j][a]) for a in range(d))
               for i in range(n) for j in range(i + 1, n))


class Problem:
    """One sample and the orders fitted to it so far."""

    def __init__(self, x, error_rate, max_mutual_overlap, max_num_components, seed, restart=0):
        self.x = np.ascontiguousarray(x, np.float64)
        self.seed, self.restart = seed, restart
        self.overlap, self.max_n = max_mutual_overlap, max_num_components
        self.error_rate, self.z_o = error_rate, overlap_z(max_mutual_overlap)
        self.z = noise(self.x.size, seed, restart)             # kept for the bootstrap, which leaves it in place
        self.X = sample(self.x, error_rate, seed, restart, self.z)
        self.first_n = 2 if self.x.shape[1] == 1 else 1
        self.models = {}                   # order -> FittedMixture of its best start
        self.best_start = {}
        self.best_lb = {}
        self.next_n = self.first_n
        self.answer = None                 # (order, model) once decided

    def _model(self, n):
        if n not in self.models:
            assert n == 1
            self.models[1] = one_component(self.X)
        return self.models[n]

    def starts(self, n, t):
        """The start rows of start t of order n."""
        return start_rows(self.seed, n, t, len(self.X), self.restart)

    def wanted(self, window):
        """The orders of the next call: up to `window` of them that need the device."""
        out = []
        n = self.next_n
        while n <= self.max_n and len(out) < window:
            if n > 1:
                out.append(n)
            n += 1
        return out

    def advance(self):
        """Apply the order rule to the orders fitted so far."""
        while self.answer is None:
            n = self.next_n
            if n > self.max_n:
                self.answer = (self.max_n, self._model(self.max_n))
            elif n > 1 and n not in self.models:
                return
            elif components_overlap(self._model(n), self.overlap, self.z_o):
                self.answer = (n - 1, self._model(n - 1))
            else:
                self.next_n = n + 1


def solve(problems, engine=None, device=0, window=None):
    """Fit every problem until its order is decided: one engine call per window of orders (WINDOW by default)."""
    window = window or WINDOW
    if engine is None:
        from . import _capi
        engine = _capi.mixture_fit
    for p in problems:
        p.advance()
    while True:
        active = [p for p in problems if p.answer is None]
        if not active:
            return
        prob_off, prob_n, prob_d, fit_problem, fit_n, starts, owner = [], [], [], [], [], [], []
        off = 0
        for i, p in enumerate(active):
            N, d = p.X.shape
            prob_off.append(off); prob_n.append(N); prob_d.append(d)
            off += N * d
            for n in p.wanted(window):
                for t in range(N_STARTS):
                    fit_problem.append(i); fit_n.append(n); owner.append((p, n, t))
                    starts.append(p.starts(n, t))
        samples = np.concatenate([p.X.ravel() for p in active])
        got = engine(samples, prob_off, prob_n, prob_d, fit_problem, fit_n, np.concatenate(starts), device=device)
        lb, o = got["lb"], got["off"]
        for f in range(0, len(owner), N_STARTS):
            p, n, _ = owner[f]
            best = f + int(np.argmax(lb[f:f + N_STARTS]))          # argmax keeps the lowest start on a tie
            d = p.X.shape[1]
            sl = slice(int(o[best]), int(o[best + 1]))
            p.models[n] = FittedMixture(got["w"][sl], got["mu"][sl, :d], got["var"][sl, :d])
            p.best_start[n] = best - f
            p.best_lb[n] = float(lb[best])
        for p in active:
            p.advance()


BOOT_KEY = 0x626F6F74      # "boot": the second word of the key of a problem's resampling generator
BOOT_DECIDED, BOOT_NEEDS_MORE = 0, 1
BOOT_EXTRA_ORDERS = 2      # the first call hands over start rows up to the called order + 2


def resample_indices(seed, m, B):
    """The reads of the B replicates of a problem of m kept reads: [B, m] indices into them."""
    return np.random.default_rng([int(seed), BOOT_KEY]).integers(0, m, size=(B, m))


def _bootstrap_call(problems, n_caps, idx, B, engine, device):
    starts = []
    for p, n_cap in zip(problems, n_caps):
        starts += [p.starts(n, t) for n in range(max(p.first_n, 2), n_cap + 1) for t in range(N_STARTS)]
    got = engine(np.concatenate([p.x.ravel() for p in problems]), np.concatenate([p.z for p in problems]),
                 [len(p.x) for p in problems], [p.x.shape[1] for p in problems], [p.error_rate for p in problems],
                 [p.z_o for p in problems], [p.first_n for p in problems], n_caps, [p.max_n for p in problems],
                 np.concatenate(starts) if starts else np.zeros(0, np.int32), B,
                 np.concatenate([i.ravel() for i in idx]).astype(np.int32), device=device)
    out = []
    for k, (p, n_cap) in enumerate(zip(problems, n_caps)):
        d = p.x.shape[1]
        sl = slice(int(got["off"][k]), int(got["off"][k + 1]))
        out.append(dict(status=got["status"][k].copy(), order=got["order"][k].copy(),
                        best_start=got["best_start"][k].copy(), lb=got["lb"][k].copy(),
                        w=got["w"][sl].reshape(B, n_cap), mu=got["mu"][sl, :d].reshape(B, n_cap, d),
                        var=got["var"][sl, :d].reshape(B, n_cap, d), idx=idx[k]))
    return out


def bootstrap(problems, B, engine=None, device=0):
    """The order search of B bootstrap replicates of every solved problem: one engine call with
    start rows up to the called order + 2, and one more, with every order up to max_n, for the problems that had a
    replicate left undecided by that cap.  -> per problem dict(status, order, best_start, lb [B]; w [B, n_cap]; mu, var
    [B, n_cap, d]: the model of replicate b in its first order[b] components; idx [B, m]: its reads)."""
    if engine is None:
        from . import _capi
        engine = _capi.mixture_bootstrap
    if not problems:
        return []
    if any(p.answer is None for p in problems):
        raise ValueError("bootstrap needs solved problems")
    idx = [resample_indices(p.seed, len(p.x), B) for p in problems]
    out = _bootstrap_call(problems, [min(p.max_n, p.answer[0] + BOOT_EXTRA_ORDERS) for p in problems], idx, B, engine,
                          device)
    again = [k for k, r in enumerate(out) if (r["status"] == BOOT_NEEDS_MORE).any()]
    if again:
        more = _bootstrap_call([problems[k] for k in again], [problems[k].max_n for k in again],
                               [idx[k] for k in again], B, engine, device)
        for k, r in zip(again, more):
            out[k] = r
    return out


class Fitter:
    """The `fitter` of phasing.phase: -> (order, fitted mixture) for the kept sizes of a region.  `prefetched` holds a
    problem solved ahead in a batch with other regions'; anything else (the joint mode's restart) is solved here."""

    def __init__(self, engine=None, device=0, prefetched=None):
        self.engine, self.device, self.prefetched = engine, device, prefetched

    def __call__(self, real, error_rate, max_mutual_overlap, max_num_components, seed, restart):
        p = self.prefetched
        if p is None or restart != p.restart or not np.array_equal(p.x, real):
            p = Problem(real, error_rate, max_mutual_overlap, max_num_components, seed, restart)
            solve([p], self.engine, self.device)
        return p.answer


def phase_jobs(jobs, device=0, engine=None, problems_out=None):
    """jobs: ("1d" | "2d", args) as pipeline.phase_regions builds them -> what phasing.run_job returns for each, with
    the first fit of every job made in one batch.  A job's seed must be an int (see fresh_seed).  `problems_out`: a
    list that receives every job's solved Problem (None for a job with too few reads), for the bootstrap."""
    problems = []
    for kind, args in jobs:
        count_dict, ploidy, error_rate, overlap, max_n, _, seed = args
        dimension = 1 if kind == "1d" else 2
        too_few = len(count_dict) < 2 if dimension == 1 else (len(count_dict) < ploidy or len(count_dict) == 1)
        if too_few or ploidy < 1:
            problems.append(None)
            continue
        _, flat = phasing.remove_outlier_reads(count_dict, dimension)
        problems.append(Problem(np.array(flat, np.float64).reshape(-1, dimension), error_rate, overlap, max_n, seed))
    solve([p for p in problems if p is not None], engine, device)
    if problems_out is not None:
        problems_out.extend(problems)
    out = []
    for (kind, args), p in zip(jobs, problems):
        fitter = Fitter(engine, device, p)
        out.append(phasing.phase_1d_job(args, fitter) if kind == "1d" else phasing.phase_2d_job(args, fitter))
    return out
