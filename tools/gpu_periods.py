"""Measures the tandem period call (nra_tract_periods) next to the tandem motif call and round 3 on
the same reads, on one GPU; writes one JSON file.  The method is tools/gpu_motifs.py's.

For config 2 (10 k reads, TATTG) and config 4 (--regions x --reads-per-region, 3-6 bp motifs) the tracts are the reads'
cores without their 100-base flanks.  Per config: the wall time of one nra_tract_periods call over all tracts (best of
--reps, after one warm-up call), of one nra_tract_motifs call and of one nra_round3_1d call over the cores.  Kernel
times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_periods.py --reps 1`
(k_tract_periods against k_tract_motifs and round 3's kernels).

  python tools/gpu_periods.py --out periods.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanorepeat_amd import _capi, synth  # noqa: E402

FLANK = 100


def best_of(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def measure(name, d, reps):
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    _capi.tract_periods(tracts)                                   # warm-up (module load, first allocations)
    t_period = best_of(lambda: _capi.tract_periods(tracts), reps)
    _capi.tract_motifs(tracts)
    t_motif = best_of(lambda: _capi.tract_motifs(tracts), reps)
    call, _ = _capi.prepared_round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d["read_region"])
    call()
    t_r3 = best_of(call, reps)
    bases = int(sum(len(t) for t in tracts))
    row = dict(config=name, reads=len(tracts), tract_bases=bases, period_call_s=t_period, motif_call_s=t_motif,
               round3_call_s=t_r3, period_over_round3=t_period / t_r3, period_over_motif=t_period / t_motif)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for c in a.configs.split(","):
        if c == "2":
            rows.append(measure("config2", synth.config2(), a.reps))
        elif c == "4":
            rows.append(measure("config4", synth.config4(a.regions, a.reads_per_region), a.reps))
        else:
            raise SystemExit(f"unknown config {c}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(calls=rows), f, indent=1)


if __name__ == "__main__":
    main()
