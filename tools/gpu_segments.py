"""Measures the motif-run call (nra_tract_segments) next to the repeat structure call
(nra_read_structure) and round 3 on the same reads, on one GPU, and writes one JSON file.

For config 2 (10 k reads, TATTG) and config 4 (--regions x --reads-per-region, 3-6 bp motifs) the tracts are the reads'
cores without their 100-base flanks; the motif set of a region is its BED motif plus one variant of the same period
(the last base changed).  Per config: the wall time of one nra_tract_segments call over all tracts from host buffers to
host results (best of --reps, after one warm-up call), of one nra_read_structure call with the BED motif alone and of
one nra_round3_1d call over the cores, plus the tracts' bases and the state-cell updates (bases x states of the set).
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_segments.py --reps 1`
(k_segment<SC> against k_structure<P> and round 3's kernels).

  python tools/gpu_segments.py --out segments.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanorepeat_amd import _capi, segments, synth  # noqa: E402

FLANK = 100


def best_of(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def variant(u):
    """The motif with its last base changed."""
    return u[:-1] + "ACGT"[("ACGT".index(u[-1]) + 1) % 4]


def measure(name, d, reps, switch_cost):
    motifs = [u for _, u, _ in d["regions"]]
    sets = [[u, variant(u)] for u in motifs]
    rr = d["read_region"] if d["read_region"] is not None else np.zeros(len(d["reads"]), np.int32)
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    _capi.tract_segments(sets, tracts, rr, switch_cost)           # warm-up (module load, first allocations)
    t_seg = best_of(lambda: _capi.tract_segments(sets, tracts, rr, switch_cost), reps)
    _capi.read_structure(motifs, tracts, rr)
    t_struct = best_of(lambda: _capi.read_structure(motifs, tracts, rr), reps)
    call, _ = _capi.prepared_round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d["read_region"])
    call()
    t_r3 = best_of(call, reps)
    bases = int(sum(len(t) for t in tracts))
    cells = int(sum(len(t) * 2 * len(motifs[int(g)]) for t, g in zip(tracts, rr)))
    row = dict(config=name, reads=len(tracts), tract_bases=bases, state_cells=cells, phase_cells=cells // 2,
               switch_cost=switch_cost, segments_call_s=t_seg, structure_call_s=t_struct, round3_call_s=t_r3,
               segments_over_structure=t_seg / t_struct, segments_over_round3=t_seg / t_r3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--switch-cost", type=int, default=segments.DEFAULT_SWITCH_COST)
    a = ap.parse_args()
    rows = []
    for c in a.configs.split(","):
        if c == "2":
            rows.append(measure("config2", synth.config2(), a.reps, a.switch_cost))
        elif c == "4":
            rows.append(measure("config4", synth.config4(a.regions, a.reads_per_region), a.reps, a.switch_cost))
        else:
            raise SystemExit(f"unknown config {c}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
