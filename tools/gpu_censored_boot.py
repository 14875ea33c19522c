"""Measures the bootstrap of the censored allele fit (nra_censored_bootstrap) on the 1000-region
panel of section 26.4 on one GPU and writes one JSON file.

The panel and its bounds are those of tools/gpu_censored.py (synth.panel, one quantify_from_reads run, add_bounds).
censored.fit_problems gives the calls; the layouts, index rows and lnN of --replicates replicates per region are built
once (timed as host preparation), then the nra_censored_bootstrap call is timed --reps times from host buffers to host
results, and once more with every problem streaming its values.  The yardstick is the composed device path of the
tests (tests/censored_boot_ref.py over _capi: replicates materialised on the host, starts in Python, one
nra_censored_fit call, the BIC rule in Python) on --yardstick-regions regions, alternating with the entry point on the
same regions in this process, two repetitions, scaled to all regions.  Reported without a pass mark: how often the
interval of a called closed allele holds the planted size nearest to the call, and the Open_Support of the regions
with and without a planted unspanned allele.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_censored_boot.py --reps 1 --yardstick-regions 0`.

  python tools/gpu_censored_boot.py --out boot.json [--regions 1000] [--replicates 200] [--reps 3]
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
sys.path.append(os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def boot_args(problems, indices, n_rep, seed):
    """The arguments of censored_bootstrap for problems with an exact value, as censored.bootstrap_problems builds them."""
    from nanorepeat_amd import censored
    values, off, rows, rep_m = [], [], [], []
    for pr, i in zip(problems, indices):
        off.append(len(values)); values += censored.sorted_layout(pr)
        idx, m_b = censored.resample_rows(seed, i, pr.m, pr.m + pr.q, n_rep)
        rows.append(idx.ravel()); rep_m.append(m_b)
    n_pts = [pr.m + pr.q for pr in problems]
    return dict(values=np.array(values), prob_off=np.array(off, np.int64), prob_n=np.array(n_pts, np.int32),
                prob_n_exact=np.array([pr.m for pr in problems], np.int32), prob_tau=np.array([pr.tau for pr in problems]),
                prob_ln_n=np.array([math.log(n) for n in n_pts]), n_rep=n_rep, idx=np.concatenate(rows),
                rep_m=np.stack(rep_m), max_alleles=censored.MAX_ALLELES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick-regions", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    from nanorepeat_amd import _capi, censored, phasing, pipeline, synth
    import censored_boot_ref
    from gpu_censored import add_bounds
    tau = phasing.data_type_error_rate("ont")
    with tempfile.TemporaryDirectory() as tmp:
        p = synth.panel(a.regions, anchor_len=1000, reads_per_region=46, edge_overlaps=(150, 300),
                        n_decoys=a.regions, shared=min(40, a.regions), seed=33)
        ref, bed, reads = synth.write_panel(p, tmp)
        regions = pipeline.quantify_from_reads(reads, ref, bed, os.path.join(tmp, "run"), seed=1, mixture="gpu")
    cases = add_bounds(regions, p["truth"])
    planted = {}
    for g, k in p["truth"].values():
        planted.setdefault(g, set()).add(k)
    planted_of = [sorted(planted[r.index]) for r in regions
                  if any(x.round3_repeat_size is not None for x in r.read_dict.values()) and planted.get(r.index)]
    assert len(planted_of) == len(cases)
    problems = [censored.Problem([str(i) for i in range(len(e))], e, [str(i) for i in range(len(b))], b,
                                 ["one_anchor"] * len(b), tau) for e, b, _ in cases]
    fits = censored.fit_problems(problems)
    B = a.replicates
    t0 = time.perf_counter()
    args = boot_args(problems, range(len(problems)), B, a.seed)
    row = dict(regions=len(problems), replicates=B, exact_values=sum(pr.m for pr in problems),
               bounds=sum(pr.q for pr in problems), regions_with_unspanned_allele=sum(c[2] is not None for c in cases),
               host_preparation_s=time.perf_counter() - t0, index_entries=int(len(args["idx"])), runs=[])
    rep = None
    for flags, name in [(0, "device")] * a.reps + [(_capi.CENS_F_STREAM, "device, every problem streaming")]:
        t0 = time.perf_counter()
        rep = _capi.censored_bootstrap(**args, flags=flags)
        run = dict(path=name, call_s=time.perf_counter() - t0)
        print(json.dumps(run), flush=True)
        row["runs"].append(run)
    fitted = rep["status"] == _capi.CENS_BOOT_FITTED
    row["replicates_fitted"] = int(fitted.sum())
    row["replicates_at_the_cap"] = int((rep["n_iter"][fitted] == censored.MAX_ITER).sum())
    row["e_steps_of_the_chosen_fits"] = int(rep["n_iter"].sum())
    # the statistics, as the product computes them
    t0 = time.perf_counter()
    boots = [censored.CensoredBootstrap(a.seed, args["rep_m"][i], rep["model_n"][i], rep["model_open"][i], rep["nu"][i],
                                        rep["w"][i], fits[i], 0.95) for i in range(len(problems))]
    row["statistics_s"] = time.perf_counter() - t0
    held = total = 0
    for cf, boot, alleles in zip(fits, boots, planted_of):
        for size, (_, lo, hi, _, _, used) in zip(cf.sizes(), boot.rows):
            if used:
                truth = min(alleles, key=lambda v: abs(v - size))
                total += 1
                held += int(lo <= truth <= hi)
    row["closed_alleles_with_an_interval"], row["intervals_that_hold_the_planted_size"] = total, held
    with_long = np.array([c[2] is not None for c in cases])
    support = np.array([b.open_support for b in boots])
    model = np.array([b.model_support for b in boots])
    row["open_support_with_unspanned_allele"] = dict(mean=float(support[with_long].mean()),
                                                     min=float(support[with_long].min()))
    row["open_support_without_unspanned_allele"] = dict(mean=float(support[~with_long].mean()),
                                                        max=float(support[~with_long].max()))
    row["model_support"] = dict(mean=float(model.mean()), regions_below_half=int((model < 0.5).sum()))
    if a.yardstick_regions:
        some = list(range(0, len(problems), max(1, len(problems) // a.yardstick_regions)))[:a.yardstick_regions]
        part = boot_args([problems[i] for i in some], some, B, a.seed)
        composed = device = None
        for r in range(2):
            t0 = time.perf_counter()
            composed = censored_boot_ref.censored_bootstrap(**part, fit_engine=_capi)
            t1 = time.perf_counter()
            device = _capi.censored_bootstrap(**part)
            t2 = time.perf_counter()
            run = dict(path="composed device path against the entry point", rep=r, regions=len(some),
                       composed_s=t1 - t0, entry_point_s=t2 - t1,
                       composed_scaled_to_all_regions_s=(t1 - t0) * len(problems) / len(some))
            print(json.dumps(run), flush=True)
            row["runs"].append(run)
        row["yardstick_same_bits"] = all(composed[k].tobytes() == device[k].tobytes() for k in device)
        best = min(r["composed_scaled_to_all_regions_s"] for r in row["runs"] if "composed_s" in r)
        row["ratio_composed_over_entry_point"] = best / min(r["call_s"] for r in row["runs"] if r.get("path") == "device")
    print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
