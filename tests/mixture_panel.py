"""Seeded synthetic regions for the mixture tests: read sizes of one- and two-allele regions as round 3 reports them
(one decimal), 1D and 2D.  Shared by the CPU and the GPU tests so that both see the same problems."""
import numpy as np

PANEL_SEED = 2024
EDGE_GAPS = (0, 1, 2, 3)


def _sizes(rng, allele, n):
    sd = 0.015 * allele + 0.4
    return np.maximum(0.0, np.round(allele + rng.standard_normal(n) * sd, 1))


def region_1d(rng, i):
    """{read: size}, (allele 1, allele 2).  Every eighth region sits on an edge gap (0..3 units: one allele, or a coin
    flip), every tenth has few reads (down to 2 in all)."""
    a1 = int(rng.integers(8, 121))
    gap = EDGE_GAPS[(i // 8) % 4] if i % 8 == 0 else int(rng.integers(0, 41))
    if i % 10 == 9:
        n1, n2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    else:
        n1, n2 = int(rng.integers(8, 41)), int(rng.integers(8, 41))
    sizes = np.concatenate([_sizes(rng, a1, n1), _sizes(rng, a1 + gap, n2)])
    return {f"r{i}_{j}": float(v) for j, v in enumerate(sizes)}, (a1, a1 + gap)


def region_2d(rng, i):
    a = (int(rng.integers(8, 80)), int(rng.integers(5, 30)))
    gap = (int(rng.integers(0, 41)), int(rng.integers(0, 9)))
    n1, n2 = int(rng.integers(8, 41)), int(rng.integers(8, 41))
    x = np.concatenate([_sizes(rng, a[0], n1), _sizes(rng, a[0] + gap[0], n2)])
    y = np.concatenate([_sizes(rng, a[1], n1), _sizes(rng, a[1] + gap[1], n2)])
    return {f"j{i}_{j}": (float(u), float(v)) for j, (u, v) in enumerate(zip(x, y))}, (a, gap)


def panel(n_1d, n_2d, seed=PANEL_SEED):
    """-> [("1d" | "2d", count_dict, truth)]"""
    rng = np.random.default_rng(seed)
    out = [("1d",) + region_1d(rng, i) for i in range(n_1d)]
    out += [("2d",) + region_2d(rng, i) for i in range(n_2d)]
    return out


def jobs_of(regions, seed, ploidy=2, max_num_components=22):
    """The job tuples pipeline.phase_regions / quantify_joint build: region i uses seed + i."""
    return [(kind, (counts, ploidy, 0.07 if kind == "1d" else 0.1, 0.15 if kind == "1d" else 0.1, max_num_components,
                    False, seed + i)) for i, (kind, counts, _) in enumerate(regions)]


def medians(result):
    """The list of allele median sizes of a phase_1d_job / phase_2d_job result (None: too few reads)."""
    if result is None:
        return None
    return [(a.repeat1_median_size, a.repeat2_median_size) for a in result[0]]


def fit_problems(n_problems, seed=PANEL_SEED, n_lo=200, n_hi=4000):
    """Problems for the fit-by-fit comparison, drawn from the panel's regions: the simulated sample of a region cut or
    repeated to N rows (N from n_lo to n_hi), 1D and 2D alternating three to one, orders 2..6, all ten starts.
    -> (samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts)"""
    from nanorepeat_amd import mixture
    rng = np.random.default_rng([seed, 1])
    regions = panel(n_problems, n_problems, seed)
    one, two = regions[:n_problems], regions[n_problems:]
    xs, prob_off, prob_n, prob_d, fit_problem, fit_n, starts = [], [], [], [], [], [], []
    off = 0
    for p in range(n_problems):
        kind, counts, _ = (two if p % 4 == 3 else one)[p]
        d = 1 if kind == "1d" else 2
        x = np.array(list(counts.values()), np.float64).reshape(-1, d)
        X = mixture.sample(x, 0.07, seed + p)
        N = int(rng.integers(n_lo, n_hi + 1))
        X = np.resize(X, (N, d)) if N > len(X) else X[rng.permutation(len(X))[:N]]
        xs.append(np.ascontiguousarray(X).ravel())
        prob_off.append(off); prob_n.append(N); prob_d.append(d)
        off += N * d
        n = 2 + p % 5
        for t in range(mixture.N_STARTS):
            fit_problem.append(p); fit_n.append(n)
            starts.append(mixture.start_rows(seed + p, n, t, N))
    return (np.concatenate(xs), np.array(prob_off, np.int64), np.array(prob_n, np.int32), np.array(prob_d, np.int32),
            np.array(fit_problem, np.int32), np.array(fit_n, np.int32), np.concatenate(starts))
