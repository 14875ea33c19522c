"""Measures the allele consensus call (nra_tract_consensus) next to round 3 on the same reads, on
one GPU, and writes one JSON file.

For config 2 (10 k reads, TATTG, two alleles) and config 4 (--regions x --reads-per-region, 3-6 bp motifs, two alleles
per region) the tracts are the reads' cores without their 100-base flanks, grouped by their true allele.  Per config:
the wall time of one nra_tract_consensus call from host buffers to host results (best of --reps, after one warm-up
call) and of one nra_round3_1d call over the cores (best of --reps), the call's counters (alignments and tract rows
per band class, rounds, launches, widenings) and the share of rows per class.  Kernel times come from a separate run
under `rocprofv3 --kernel-trace --stats -- python tools/gpu_consensus.py --reps 1` (k_cons_align<C>, k_cons_build
against round 3's kernels).

  python tools/gpu_consensus.py --out consensus.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

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


def groups_of(d):
    rr = d["read_region"] if d["read_region"] is not None else np.zeros(len(d["reads"]), np.int32)
    kt = np.asarray(d["k_true"])
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    by = {}
    for i, (g, k) in enumerate(zip(rr.tolist(), kt.tolist())):
        by.setdefault((g, k), []).append(tracts[i])
    return [by[key] for key in sorted(by)]


def measure(name, d, reps, with_round3):
    groups = groups_of(d)
    out = _capi.tract_consensus(groups)                            # warm-up (module load, first allocations)
    t_cons = best_of(lambda: _capi.tract_consensus(groups), reps)
    st = out["stats"]
    rows = [st[f"rows_{w}"] for w in (64, 128, 256, 512, 1024)]
    row = dict(config=name, groups=len(groups), tracts=int(sum(len(g) for g in groups)),
               tract_bases=int(sum(len(t) for g in groups for t in g)), consensus_call_s=t_cons, stats=st,
               row_share={str(w): r / max(1, sum(rows)) for w, r in zip((64, 128, 256, 512, 1024), rows)},
               band_cells=int(sum(r * w for w, r in zip((64, 128, 256, 512, 1024), rows))),
               rounds_max=int(out["n_rounds"].max()), converged=int(out["converged"].sum()),
               left_out=int(out["left_out"].sum()))
    if with_round3:
        call, _ = _capi.prepared_round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d["read_region"])
        call()
        row["round3_call_s"] = best_of(call, reps)
        row["consensus_over_round3"] = t_cons / row["round3_call_s"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-round3", action="store_true")
    a = ap.parse_args()
    rows = []
    for c in a.configs.split(","):
        if c == "2":
            rows.append(measure("config2", synth.config2(), a.reps, not a.no_round3))
        elif c == "4":
            rows.append(measure("config4", synth.config4(a.regions, a.reads_per_region), a.reps, not a.no_round3))
        else:
            raise SystemExit(f"unknown config {c}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
