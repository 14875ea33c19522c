"""The bootstrap contract of include/nanorepeat_amd.h (nra_mixture_bootstrap) and DESIGN.md section 24 restated through
what the project already has: `composed_engine(fit)` has the signature and the result of _capi.mixture_bootstrap, but
materialises every replicate's sample in numpy and runs mixture.solve on it with `fit` (mixture_ref.ref_mixture_fit on
the CPU, _capi.mixture_fit on the GPU); `alleles_of_replicate` turns one replicate's answer into its alleles through
phasing.create_allele_list and remove_noisy_alleles.

The contract.  A problem: m reads kept after the outlier cut (x [m, d]), error rate e, seed s, its noise
z = default_rng(s).standard_normal(100 m d) and its start rows start_rows(s, n, t, 100 m).
* resampling: idx = default_rng([s, 0x626F6F74]).integers(0, m, size=(B, m)); the outlier cut is not repeated;
* sample of replicate b, row j (0 <= j < 100 m), axis a:
  X_b[j][a] = x[idx[b][j mod m]][a] + (z[j d + a] e) (10 + x[idx[b][j mod m]][a]), float64, in this order: the noise
  belongs to the position, and idx[b] = arange(m) gives the problem's own sample;
* order search: mixture.Problem.advance with the problem's own start rows -- orders from first_n (2 for d = 1, 1 for
  d = 2), ten starts each, the best the largest lb (a tie to the lowest start), stop at the first order with two
  components whose intervals mu +- z_o max(1, sd) overlap on every axis (the answer is the order before), at most
  max_n; order 1 has no parameters;
* order cap: with start rows up to n_cap < max_n only, a replicate not decided by then is NEEDS_MORE."""
import numpy as np

from nanorepeat_amd import mixture, phasing

STARTS = mixture.N_STARTS
COPIES = phasing.SIM_COPIES


def replicate_sample(x, z, e, idx_b):
    """X_b by the formula above: x [m, d], z [100 m d], idx_b [m] -> [100 m, d]."""
    x = np.asarray(x, np.float64)
    m, d = x.shape
    rows = np.arange(COPIES * m)
    src = x[np.asarray(idx_b)[rows % m]]                         # [100 m, d]
    return src + (np.asarray(z).reshape(-1, d) * e) * (10 + src)


class _Replicate(mixture.Problem):
    """A mixture.Problem whose sample, start rows and interval factor are handed over."""

    def __init__(self, X, z_o, first_n, max_n, rows):
        self.x, self.X = X, X
        self.seed = self.restart = 0
        self.overlap, self.z_o, self.max_n, self.first_n = None, z_o, max_n, first_n
        self.rows = rows                                          # (order, start) -> rows
        self.models, self.best_start, self.best_lb = {}, {}, {}
        self.next_n, self.answer = first_n, None

    def starts(self, n, t):
        return self.rows[(n, t)]


def composed_engine(fit):
    """-> engine(...) with the signature and the result of _capi.mixture_bootstrap."""

    def engine(x, z, prob_m, prob_d, prob_e, prob_zo, prob_first_n, prob_n_cap, prob_max_n, starts, n_rep, idx, flags=0,
               device=0):
        x, z = np.asarray(x, np.float64).ravel(), np.asarray(z, np.float64).ravel()
        starts, idx = np.asarray(starts, np.int32).ravel(), np.asarray(idx).ravel()
        P, B = len(prob_m), int(n_rep)
        off = np.zeros(P + 1, np.int64)
        np.cumsum(B * np.asarray(prob_n_cap, np.int64), out=off[1:])
        out = dict(status=np.zeros((P, B), np.int32), order=np.zeros((P, B), np.int32),
                   best_start=np.zeros((P, B), np.int32), lb=np.zeros((P, B)), off=off, w=np.zeros(int(off[-1])),
                   mu=np.zeros((int(off[-1]), 2)), var=np.zeros((int(off[-1]), 2)))
        xo = zo = so = io = 0
        reps = []
        for p in range(P):
            m, d, n_cap = int(prob_m[p]), int(prob_d[p]), int(prob_n_cap[p])
            xp, zp = x[xo:xo + m * d].reshape(m, d), z[zo:zo + COPIES * m * d]
            xo, zo = xo + m * d, zo + COPIES * m * d
            rows = {}
            for n in range(max(int(prob_first_n[p]), 2), n_cap + 1):
                for t in range(STARTS):
                    rows[(n, t)] = starts[so:so + n]
                    so += n
            for b in range(B):
                X = replicate_sample(xp, zp, float(prob_e[p]), idx[io:io + m])
                io += m
                reps.append((p, b, _Replicate(X, float(prob_zo[p]), int(prob_first_n[p]), n_cap, rows)))
        mixture.solve([r for _, _, r in reps], fit, device)
        for p, b, r in reps:
            n, model = r.answer
            n_cap, d = int(prob_n_cap[p]), int(prob_d[p])
            if n_cap < int(prob_max_n[p]) and n >= n_cap:         # the cap, not the rule, ended the search
                out["status"][p, b] = mixture.BOOT_NEEDS_MORE
                out["best_start"][p, b] = -1
                continue
            out["order"][p, b] = n
            out["best_start"][p, b] = r.best_start.get(n, -1)
            if n > 1:
                o = int(off[p]) + b * n_cap
                out["lb"][p, b] = r.best_lb[n]
                out["w"][o:o + n] = model.weights_
                out["mu"][o:o + n, :d] = model.means_
                out["var"][o:o + n, :d] = model.covariances_
        return out

    return engine


def alleles_of_replicate(x, idx_b, order, w, mu, var, ploidy, remove_noisy_reads):
    """The alleles of one decided replicate of a 1D problem, per phasing: sizes in the order of the component means."""
    x = np.asarray(x, np.float64).reshape(-1)
    real = x[np.asarray(idx_b)].reshape(-1, 1)
    names = [f"r{j}" for j in range(len(real))]
    counts = {name: float(v) for name, v in zip(names, real[:, 0])}
    if order <= 1:
        model = mixture.one_component(real)
    else:
        model = mixture.FittedMixture(w[:order], np.asarray(mu[:order]).reshape(order, 1),
                                      np.asarray(var[:order]).reshape(order, 1))
    alleles = phasing.create_allele_list(max(order, 1), model, names, real, counts)
    if remove_noisy_reads and len(alleles) > ploidy:
        alleles, _ = phasing.remove_noisy_alleles(alleles, ploidy)
    alleles.sort(key=lambda a: a.gmm_mean1)
    return [a.repeat1_median_size for a in alleles]


def limit_cases(boot_start_rows):
    """(good, [(change, code)]): keyword arguments of _capi.mixture_bootstrap that pass, and changes to them that must be
    refused with NRA_E_ARG (-1) or NRA_E_RANGE (-3) before the device is touched."""
    good = dict(x=np.array([20.0, 21.0, 40.0]), z=np.zeros(300), prob_m=[3], prob_d=[1], prob_e=[0.07], prob_zo=[1.0],
                prob_first_n=[2], prob_n_cap=[2], prob_max_n=[4], starts=np.arange(20) % 300, n_rep=2,
                idx=[0, 1, 2, 2, 2, 0])
    m = (1 << 22) // 100 + 1                                      # N = 100 m > 2^22
    cases = [(dict(n_rep=0, idx=[]), -1), (dict(n_rep=-1, idx=[]), -1), (dict(n_rep=1001, idx=[0] * 3003), -3),
             (dict(idx=[0, 1, 2, 3, 2, 0]), -1), (dict(idx=[0, 1, 2, -1, 2, 0]), -1),
             (dict(x=np.array([20.0, np.nan, 40.0])), -1), (dict(z=np.where(np.arange(300) == 299, np.inf, 0.0)), -1),
             (dict(prob_e=[np.nan]), -1), (dict(prob_zo=[np.inf]), -1),
             (dict(prob_d=[3], x=np.zeros(9), z=np.zeros(900)), -1), (dict(prob_d=[0], x=np.zeros(0), z=np.zeros(0)), -1),
             (dict(prob_n_cap=[33], prob_max_n=[40], starts=np.zeros(boot_start_rows(2, 33), np.int32)), -3),
             (dict(prob_n_cap=[5], starts=np.zeros(boot_start_rows(2, 5), np.int32)), -1),     # n_cap > max_n
             (dict(starts=np.where(np.arange(20) == 19, 300, 0)), -1), (dict(flags=4), -1),
             (dict(prob_first_n=[0]), -1), (dict(prob_first_n=[3], starts=np.zeros(0, np.int32)), -1),
             (dict(prob_first_n=[5], prob_n_cap=[3], prob_max_n=[3], starts=np.zeros(0, np.int32)), -1),
             (dict(x=np.ones(m), z=np.zeros(100 * m), prob_m=[m], n_rep=1, idx=np.zeros(m, np.int32)), -3)]
    return good, cases
