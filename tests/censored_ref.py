"""Restatement of the censored allele fit (include/nanorepeat_amd.h) in numpy and the standard
library: `censored_fit` and `censored_posteriors` have the signatures of the _capi functions of these names, so this
module stands in for _capi as `censored_engine`.  erfc is math.erfc; erfcx(u) = exp(u^2) erfc(u) up to u = 5 and a
continued fraction of fixed length above."""
import math

import numpy as np

SQRT1_2 = 0.7071067811865476
SQRT_2_PI = 0.7978845608028654
TEN_EPS = 10.0 * 2.220446049250313e-16
CF_TERMS = 18           # at u = 5 sixteen terms already agree with double precision (2 ulp); the error falls with u


def erfcx(u):
    """exp(u^2) erfc(u) for u > 0 (a float)."""
    if u <= 5.0:
        return math.exp(u * u) * math.erfc(u)
    t = u
    for k in range(CF_TERMS, 0, -1):                 # sqrt(pi) erfcx(u) = 1 / (u + (1/2) / (u + (2/2) / (u + (3/2) / ...
        t = u + 0.5 * k / t
    return 1.0 / (math.sqrt(math.pi) * t)


def _erfcx_array(u, erfc_u):
    """erfcx of the entries of u that are > 0 (the others: any finite value)."""
    out = np.exp(np.clip(u, 0.0, 5.0) ** 2) * erfc_u
    big = u > 5.0
    if big.any():
        t = u[big]
        v = t
        for k in range(CF_TERMS, 0, -1):
            v = t + 0.5 * k / v
        out[big] = 1.0 / (math.sqrt(math.pi) * v)
    return out


def log_s_lambda(z):
    """logS(z) and the inverse Mills ratio lambda(z) of an array z, by the two-branch form of the contract."""
    u = z * SQRT1_2
    e = np.array([math.erfc(v) for v in u.ravel().tolist()]).reshape(u.shape)
    neg = u <= 0.0
    ex = _erfcx_array(u, e)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ls = np.where(neg, np.log(0.5 * np.where(neg, e, 1.0)), np.log(0.5 * ex) - u * u)
        lam = np.where(neg, (SQRT_2_PI * np.exp(-(u * u))) / np.where(neg, e, 1.0), SQRT_2_PI / ex)
    return ls, lam


def e_step(ye, yc, tau, nu, w, open_):
    """log p of every value and the posteriors: (lse_exact [m], lse_cens [q], r_exact [m, n + open], r_cens [q, n + open],
    t [q, n] = nu + tau lambda).  w: n + open weights, the open one last."""
    n = len(nu)
    lw = np.log(w)
    hl = 0.5 * math.log(2.0 * math.pi * (tau * tau))
    i2 = 1.0 / (2.0 * (tau * tau))
    d = ye[:, None] - nu[None, :]
    lpe = (lw[None, :n] - hl) - (d * d) * i2
    me = lpe.max(axis=1)
    lse_e = me + np.log(np.exp(lpe - me[:, None]).sum(axis=1))
    re = np.exp(lpe - lse_e[:, None])
    if open_:
        re = np.concatenate([re, np.zeros((len(ye), 1))], axis=1)
    if len(yc) == 0:
        return lse_e, np.zeros(0), re, np.zeros((0, n + open_)), np.zeros((0, n))
    z = (yc[:, None] - nu[None, :]) * (1.0 / tau)
    ls, lam = log_s_lambda(z)
    lpc = lw[None, :n] + ls
    if open_:
        lpc = np.concatenate([lpc, np.full((len(yc), 1), lw[n])], axis=1)
    mc = lpc.max(axis=1)
    lse_c = mc + np.log(np.exp(lpc - mc[:, None]).sum(axis=1))
    rc = np.exp(lpc - lse_c[:, None])
    return lse_e, lse_c, re, rc, nu[None, :] + tau * lam


def fit_one(y, n_exact, tau, n, open_, nu0, max_iter=500, tol=1e-9, trace=None):
    """One fit -> (ll, w [n + open], nu [n], n_iter, converged).  `trace`: a list that receives lb of every E-step."""
    y = np.asarray(y, np.float64)
    ye, yc = y[:n_exact], y[n_exact:]
    N = len(y)
    nu = np.array(nu0, np.float64)
    w = np.full(n + open_, 1.0 / (n + open_))
    lb, lb_prev, n_iter, converged = 0.0, -math.inf, 0, 0
    for it in range(1, max_iter + 1):
        lse_e, lse_c, re, rc, t = e_step(ye, yc, tau, nu, w, open_)
        lb = (lse_e.sum() + lse_c.sum()) / N
        if trace is not None:
            trace.append(lb)
        sr = re.sum(axis=0) + rc.sum(axis=0)
        sy = (re[:, :n] * ye[:, None]).sum(axis=0) + (rc[:, :n] * t).sum(axis=0)
        nk = sr + TEN_EPS
        w = nk / N
        nu = np.where(sr[:n] > 1e-12, sy / nk[:n], nu)
        n_iter = it
        if abs(lb - lb_prev) < tol:
            converged = 1
            break
        lb_prev = lb
    return lb * N, w, nu, n_iter, converged


def censored_fit(values, prob_off, prob_n, prob_n_exact, prob_tau, fit_problem, fit_n, fit_open, starts, max_iter=500,
                 tol=1e-9, flags=0, device=0, traces=None):
    """As _capi.censored_fit.  `traces`: a list that receives the lb trace of every fit."""
    y = np.asarray(values, np.float64)
    nf = len(fit_n)
    nu_off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.asarray(fit_n, np.int64), out=nu_off[1:])
    w_off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.asarray(fit_n, np.int64) + np.asarray(fit_open, np.int64), out=w_off[1:])
    out = dict(ll=np.zeros(nf), n_iter=np.zeros(nf, np.int32), converged=np.zeros(nf, np.int32), nu_off=nu_off,
               w_off=w_off, nu=np.zeros(int(nu_off[-1])), w=np.zeros(int(w_off[-1])))
    starts = np.asarray(starts, np.float64)
    for f in range(nf):
        p, n, o = int(fit_problem[f]), int(fit_n[f]), int(fit_open[f])
        trace = [] if traces is not None else None
        ll, w, nu, it, conv = fit_one(y[prob_off[p]:prob_off[p] + prob_n[p]], int(prob_n_exact[p]), float(prob_tau[p]),
                                      n, o, starts[nu_off[f]:nu_off[f + 1]], max_iter, tol, trace)
        out["ll"][f], out["n_iter"][f], out["converged"][f] = ll, it, conv
        out["nu"][nu_off[f]:nu_off[f + 1]] = nu
        out["w"][w_off[f]:w_off[f + 1]] = w
        if traces is not None:
            traces.append(trace)
    return out


def censored_posteriors(values, prob_off, prob_n, prob_n_exact, prob_tau, model_n, model_open, w, nu, device=0):
    """As _capi.censored_posteriors."""
    y = np.asarray(values, np.float64)
    w, nu = np.asarray(w, np.float64), np.asarray(nu, np.float64)
    out, o_w, o_nu = [], 0, 0
    for p in range(len(prob_n)):
        n, o, m = int(model_n[p]), int(model_open[p]), int(prob_n_exact[p])
        yp = y[prob_off[p]:prob_off[p] + prob_n[p]]
        _, _, re, rc, _ = e_step(yp[:m], yp[m:], float(prob_tau[p]), nu[o_nu:o_nu + n], w[o_w:o_w + n + o], o)
        out.append(np.concatenate([re, rc], axis=0))
        o_w += n + o
        o_nu += n
    return out
