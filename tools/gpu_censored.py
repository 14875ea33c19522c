"""Measures the censored allele fit (nra_censored_fit) on the 1000-region panel of section 13, with
bounds added, on one GPU, and writes one JSON file.

The panel is synth.panel(--regions, anchor_len=1000, reads_per_region=46, ...) as in tools/gpu_mixture.py.  One run of
pipeline.quantify_from_reads gives the regions with their round-3 sizes.  Bounds are added per region from a seeded
generator: 5 to 25 reads that end inside one of the region's planted alleles show floor(U * units) of it, and every
fourth region gets an allele of 300 to 1000 units that no read spans, seen by 15 to 30 such reads.  censored.fit_problems
then runs --reps times on these problems; the nra_censored_fit call is timed from host buffers to host results, and so
is the whole step (starts, both calls, the BIC rule).  The yardstick is the tests' restatement (tests/censored_ref.py)
of the same nra_censored_fit call on --ref-regions of the problems, in 16 fresh worker processes that never open the
GPU, scaled to all regions.  The four-class panel of the tests (tests/censored_cases.py) is called on the device at a
read noise of 4 % and of tau.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_censored.py --reps 1 --ref-regions 0 --no-classes`.

  python tools/gpu_censored.py --out censored.json [--regions 1000] [--reps 3] [--ref-regions 64]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def ref_fit_one_problem(job):
    """Worker: every fit of one problem through the restatement.  Imports nothing that opens the GPU."""
    import censored_ref
    from nanorepeat_amd import censored
    exact, bounds, tau = job
    pr = censored.Problem([str(i) for i in range(len(exact))], exact, [str(i) for i in range(len(bounds))], bounds,
                          ["one_anchor"] * len(bounds), tau)
    t0 = time.perf_counter()
    cf = censored.fit_problems([pr], engine=censored_ref)[0]
    return time.perf_counter() - t0, cf.n, cf.open


def add_bounds(regions, truth, seed=5):
    """[(exact sizes, bounds, unspanned units or None)] per region with a sized read."""
    rng = np.random.default_rng(seed)
    planted = {}
    for g, k in truth.values():
        planted.setdefault(g, set()).add(k)
    out = []
    for region in regions:
        exact = [float(r.round3_repeat_size) for r in region.read_dict.values() if r.round3_repeat_size is not None]
        alleles = sorted(planted.get(region.index, ()))
        if not exact or not alleles:
            continue
        bounds = [int(math.floor(rng.random() * alleles[int(rng.integers(0, len(alleles)))]))
                  for _ in range(int(rng.integers(5, 26)))]
        long_ = None
        if len(out) % 4 == 0:
            long_ = int(rng.integers(300, 1001))
            bounds += [int(math.floor(rng.random() * long_)) for _ in range(int(rng.integers(15, 31)))]
        out.append((exact, [c for c in bounds if c >= 1], long_))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-regions", type=int, default=64)
    ap.add_argument("--no-classes", action="store_true")
    a = ap.parse_args()
    from nanorepeat_amd import _capi, censored, phasing, pipeline, synth
    tau = phasing.data_type_error_rate("ont")
    with tempfile.TemporaryDirectory() as tmp:
        p = synth.panel(a.regions, anchor_len=1000, reads_per_region=46, edge_overlaps=(150, 300),
                        n_decoys=a.regions, shared=min(40, a.regions), seed=33)
        ref, bed, reads = synth.write_panel(p, tmp)
        regions = pipeline.quantify_from_reads(reads, ref, bed, os.path.join(tmp, "run"), seed=1, mixture="gpu")
    cases = add_bounds(regions, p["truth"])
    problems = [censored.Problem([str(i) for i in range(len(e))], e, [str(i) for i in range(len(b))], b,
                                 ["one_anchor"] * len(b), tau) for e, b, _ in cases]
    row = dict(regions=len(problems), exact_values=sum(pr.m for pr in problems), bounds=sum(pr.q for pr in problems),
               regions_with_unspanned_allele=sum(c[2] is not None for c in cases), runs=[])
    spent = {}

    class Engine:
        @staticmethod
        def censored_fit(*args, **kw):
            t0 = time.perf_counter()
            out = _capi.censored_fit(*args, **kw)
            spent["call"], spent["fits"] = time.perf_counter() - t0, len(out["ll"])
            spent["capped"] = int((out["converged"] == 0).sum())
            spent["e_steps"] = int(out["n_iter"].sum())
            return out

        @staticmethod
        def censored_posteriors(*args, **kw):
            t0 = time.perf_counter()
            out = _capi.censored_posteriors(*args, **kw)
            spent["posteriors"] = time.perf_counter() - t0
            return out

    fits = None
    for rep in range(a.reps):
        t0 = time.perf_counter()
        fits = censored.fit_problems(problems, engine=Engine)
        run = dict(path="device", rep=rep, step_s=time.perf_counter() - t0, fit_call_s=spent["call"],
                   posteriors_call_s=spent["posteriors"], fits=spent["fits"], fits_at_the_cap=spent["capped"],
                   e_steps=spent["e_steps"])
        print(json.dumps(run), flush=True)
        row["runs"].append(run)
    want_open = [int(c[2] is not None) for c in cases]
    row["open_called_as_planted"] = sum(cf.open == w for cf, w in zip(fits, want_open))
    row["closed_alleles_called"] = {str(k): int(v) for k, v in zip(*np.unique([cf.n for cf in fits], return_counts=True))}
    if a.ref_regions:
        import multiprocessing
        some = list(range(0, len(cases), max(1, len(cases) // a.ref_regions)))[:a.ref_regions]
        jobs = [(cases[i][0], cases[i][1], tau) for i in some]
        with multiprocessing.get_context("spawn").Pool(16) as pool:
            pool.map(ref_fit_one_problem, jobs[:16])                   # the workers have imported numpy
            t0 = time.perf_counter()
            got = pool.map(ref_fit_one_problem, jobs, chunksize=1)
            wall = time.perf_counter() - t0
        run = dict(path="restatement, 16 processes", regions=len(some), wall_s=wall,
                   scaled_to_all_regions_s=wall * len(cases) / len(some),
                   cpu_s_per_region=sum(g[0] for g in got) / len(got),
                   same_model_as_device=sum((g[1], g[2]) == (fits[i].n, fits[i].open) for g, i in zip(got, some)))
        run["ratio_restatement_over_device_step"] = run["scaled_to_all_regions_s"] / min(r["step_s"] for r in row["runs"])
        print(json.dumps(run), flush=True)
        row["runs"].append(run)
    if not a.no_classes:
        import censored_cases
        for name, noise in (("read_noise_0.04", censored_cases.NOISE), ("read_noise_tau", censored_cases.TAU)):
            t0 = time.perf_counter()
            counts = censored_cases.call_counts(censored_cases.panel(noise=noise), _capi)
            row["classes_" + name] = dict(counts=counts, seconds=time.perf_counter() - t0)
            print(json.dumps({name: counts}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
