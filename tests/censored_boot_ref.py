"""Restatement of the censored bootstrap (include/nanorepeat_amd.h) by composition: every
replicate is materialised on the host, its models come from censored.models_of, its starts from censored.start_means,
its fits from one `censored_fit` call of a fit engine (tests/censored_ref.py by default; the GPU tests pass _capi, which
makes this the composed device path), and its model from censored.bic_of and censored.choose_model.
`censored_bootstrap` has the signature of _capi.censored_bootstrap, and the module also carries censored_fit and
censored_posteriors, so it stands in as `censored_engine` of the commands.  `starts_by_index` restates how the kernel
takes the three starts from the two sorted runs by position."""
import math

import numpy as np

from nanorepeat_amd import censored
import censored_ref as REF

censored_fit = REF.censored_fit
censored_posteriors = REF.censored_posteriors
FITTED, NO_EXACT = 0, 1


def censored_bootstrap(values, prob_off, prob_n, prob_n_exact, prob_tau, prob_ln_n, n_rep, idx, rep_m, max_alleles,
                       max_iter=500, tol=1e-9, flags=0, device=0, fit_engine=REF):
    """As _capi.censored_bootstrap.  prob_ln_n is not read: bic_of takes math.log(N) itself, which is what the contract
    has the caller pass."""
    y = np.asarray(values, np.float64)
    n_rep, P = int(n_rep), len(prob_n)
    idx = np.asarray(idx, np.int64).ravel()
    rep_m = np.asarray(rep_m, np.int64).reshape(P, n_rep)
    shape = (P, n_rep)
    out = dict(status=np.zeros(shape, np.int32), model_n=np.zeros(shape, np.int32), model_open=np.zeros(shape, np.int32),
               best_start=np.zeros(shape, np.int32), n_iter=np.zeros(shape, np.int32), ll=np.zeros(shape),
               bic=np.zeros(shape), nu=np.zeros(shape + (8,)), w=np.zeros(shape + (9,)))
    rep_values, rep_off, rep_n, rep_exact, rep_tau = [], [], [], [], []
    fit_problem, fit_n, fit_open, starts, owner = [], [], [], [], []
    row0 = 0
    for p in range(P):
        N = int(prob_n[p])
        ys = y[prob_off[p]:prob_off[p] + N]
        for b in range(n_rep):
            row = idx[row0 + b * N:row0 + (b + 1) * N]
            m_b = int(rep_m[p, b])
            assert (np.diff(row) >= 0).all() and m_b == int((row < prob_n_exact[p]).sum())
            if m_b == 0:
                out["status"][p, b], out["model_open"][p, b] = NO_EXACT, int(N > 0)
                continue
            yb = ys[row].tolist()
            k = len(rep_off)
            rep_off.append(len(rep_values)); rep_values += yb
            rep_n.append(N); rep_exact.append(m_b); rep_tau.append(float(prob_tau[p]))
            for n, o in censored.models_of(len(set(yb[:m_b])), N - m_b, max_alleles):
                for t, st in enumerate(censored.start_means(yb[:m_b], yb[m_b:], n)):
                    fit_problem.append(k); fit_n.append(n); fit_open.append(o); starts += st
                    owner.append((p, b, n, o, t))
        row0 += n_rep * N
    if not owner:
        return out
    got = fit_engine.censored_fit(np.array(rep_values), np.array(rep_off, np.int64), np.array(rep_n, np.int32),
                                  np.array(rep_exact, np.int32), np.array(rep_tau), np.array(fit_problem, np.int32),
                                  np.array(fit_n, np.int32), np.array(fit_open, np.int32), np.array(starts),
                                  max_iter=max_iter, tol=tol, device=device)
    best = {}                                    # (p, b) -> {(n, o): fit}: the largest ll, ties to the lowest start
    for f, (p, b, n, o, t) in enumerate(owner):
        of = best.setdefault((p, b), {})
        if (n, o) not in of or got["ll"][f] > got["ll"][of[(n, o)]]:
            of[(n, o)] = f
    for (p, b), of in best.items():
        bics = {no: censored.bic_of(float(got["ll"][f]), no[0], no[1], int(prob_n[p])) for no, f in of.items()}
        n, o = censored.choose_model(bics)
        f = of[(n, o)]
        out["status"][p, b], out["model_n"][p, b], out["model_open"][p, b] = FITTED, n, o
        out["best_start"][p, b], out["n_iter"][p, b] = owner[f][4], got["n_iter"][f]
        out["ll"][p, b], out["bic"][p, b] = got["ll"][f], bics[(n, o)]
        out["nu"][p, b, :n] = got["nu"][got["nu_off"][f]:got["nu_off"][f] + n]
        out["w"][p, b, :n + o] = got["w"][got["w_off"][f]:got["w_off"][f] + n + o]
    return out


class Composed:
    """The composed path over a fit engine, as a `censored_engine`: Composed(_capi) is the composed device path."""

    def __init__(self, fit_engine):
        self.fit_engine = fit_engine
        self.censored_fit, self.censored_posteriors = fit_engine.censored_fit, fit_engine.censored_posteriors

    def censored_bootstrap(self, *args, **kw):
        return censored_bootstrap(*args, fit_engine=self.fit_engine, **kw)


# ---------------------------------------------------------------------------- the starts as the kernel takes them
def quant_pos(k, n, L):
    """censored.quant's position: the float64 expression of the contract."""
    return min(L - 1, int(math.floor((k + 0.5) / n * L)))


def merged(y, m, q, k):
    """Value k of the merge of the sorted runs y[:m] and y[m:m + q]: the kernel's bounded binary search."""
    lo, hi = max(0, k - q), min(k, m)
    steps = 0
    while lo < hi:
        steps += 1
        assert steps <= 21
        mid = (lo + hi) >> 1
        assert 0 <= mid < m and 0 <= k - mid - 1 < q
        if y[mid] < y[m + (k - mid - 1)]:
            lo = mid + 1
        else:
            hi = mid
    j = k - lo
    if lo >= m:
        return y[m + j]
    if j >= q:
        return y[lo]
    return min(y[lo], y[m + j])


def starts_by_index(y, m, n):
    """The three starts of order n of a replicate y (m exact values ascending, then its bounds ascending)."""
    N, q = len(y), len(y) - m
    top = max(y[m - 1], y[N - 1]) if q else y[m - 1]
    return [[y[quant_pos(k, n, m)] for k in range(n)],
            [merged(y, m, q, quant_pos(k, n, N)) for k in range(n)],
            [y[quant_pos(k, n - 1, m)] for k in range(n - 1)] + [top]]
