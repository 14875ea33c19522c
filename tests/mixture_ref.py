"""The mixture-fit contract of include/nanorepeat_amd.h (nra_mixture_fit) and DESIGN.md section 17 restated in plain
numpy float64: what the GPU kernel is tested against, and the stand-in for it (`mixture_engine`) in the CPU tests.
Written from the contract, not from the kernel: sums are numpy's, in numpy's order."""
import numpy as np

LLOYD_STEPS = 10
MAX_ITER = 100
TOL = 1e-3
REG_COVAR = 1e-6
EPS10 = 10 * np.finfo(np.float64).eps
LOG_2PI = float(np.log(2 * np.pi))


def labels_of(X, mu):
    """Nearest mean by squared distance summed over the axes; argmin takes the lowest component on a tie."""
    d2 = np.zeros((len(X), len(mu)))
    for a in range(X.shape[1]):
        e = X[:, a:a + 1] - mu[None, :, a]
        d2 = d2 + e * e
    return np.argmin(d2, axis=1)


def m_step(X, r):
    nk = r.sum(axis=0) + EPS10
    mu = (r.T @ X) / nk[:, None]
    var = (r.T @ (X * X)) / nk[:, None] - mu * mu + REG_COVAR
    return nk / len(X), mu, var


def log_joint(X, w, mu, var):
    """log p(x, c), [N, n]."""
    a = np.log(w) - 0.5 * (X.shape[1] * LOG_2PI + np.log(var).sum(axis=1))
    q = np.zeros((len(X), len(w)))
    for ax in range(X.shape[1]):
        e = X[:, ax:ax + 1] - mu[None, :, ax]
        q = q + e * e * (1.0 / var[None, :, ax])
    return a[None, :] - 0.5 * q


def log_sum_exp(lj):
    m = lj.max(axis=1)
    return m + np.log(np.exp(lj - m[:, None]).sum(axis=1))


def fit_one(X, start_rows, detail=False):
    """One fit -> dict(lb, w, mu, var, n_iter, converged); with detail also `margin`, the distance of the last
    step's |lb - lb_prev| from the tolerance (how close the stop test came to going the other way)."""
    X = np.asarray(X, np.float64)
    n = len(start_rows)
    mu = X[np.asarray(start_rows, np.int64)].copy()
    lab = labels_of(X, mu)
    for _ in range(LLOYD_STEPS):
        for c in range(n):
            mine = X[lab == c]
            if len(mine):
                mu[c] = mine.sum(axis=0) / len(mine)
        new = labels_of(X, mu)
        same = np.array_equal(new, lab)
        lab = new
        if same:
            break
    r = np.zeros((len(X), n))
    r[np.arange(len(X)), lab] = 1.0
    w, mu, var = m_step(X, r)
    lb_prev, converged, margin = -np.inf, 0, np.inf
    for it in range(1, MAX_ITER + 1):
        lj = log_joint(X, w, mu, var)
        lse = log_sum_exp(lj)
        lb = float(lse.sum() / len(X))
        w, mu, var = m_step(X, np.exp(lj - lse[:, None]))
        n_iter = it
        change = abs(lb - lb_prev)
        margin = min(margin, abs(change - TOL))     # an earlier step that nearly stopped is a knife edge too
        if change < TOL:
            converged = 1
            break
        lb_prev = lb
    out = dict(lb=lb, w=w, mu=mu, var=var, n_iter=n_iter, converged=converged)
    if detail:
        out["margin"] = margin
    return out


def ref_mixture_fit(samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts, flags=0, device=0, detail=False):
    """The signature and the result of _capi.mixture_fit."""
    x = np.ascontiguousarray(samples, np.float64).ravel()
    nf = len(fit_n)
    off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.asarray(fit_n, np.int64), out=off[1:])
    t = int(off[-1])
    starts = np.asarray(starts, np.int64)
    out = dict(lb=np.zeros(nf), n_iter=np.zeros(nf, np.int32), converged=np.zeros(nf, np.int32), off=off,
               w=np.zeros(t), mu=np.zeros((t, 2)), var=np.zeros((t, 2)))
    if detail:
        out["margin"] = np.zeros(nf)
    for f in range(nf):
        p = int(fit_problem[f])
        N, d = int(prob_n[p]), int(prob_d[p])
        X = x[int(prob_off[p]):int(prob_off[p]) + N * d].reshape(N, d)
        got = fit_one(X, starts[off[f]:off[f + 1]], detail)
        o = slice(int(off[f]), int(off[f + 1]))
        out["lb"][f], out["n_iter"][f], out["converged"][f] = got["lb"], got["n_iter"], got["converged"]
        out["w"][o] = got["w"]
        out["mu"][o, :d] = got["mu"]
        out["var"][o, :d] = got["var"]
        if detail:
            out["margin"][f] = got["margin"]
    return out
