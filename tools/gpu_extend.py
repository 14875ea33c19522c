"""Measures the anchored extension call (nra_extend_tracts) next to the repeat structure call on the
same tracts, on one GPU, and writes one JSON file.

For config 2 (10 k reads, TATTG) and config 4 (--regions x --reads-per-region, 3-6 bp motifs) the tracts are the reads'
cores without their 100-base flanks, as tools/gpu_structure.py takes them.  Per config: the wall time of one
nra_extend_tracts call and of one nra_read_structure call over all tracts, from host buffers to host results (best of
--reps, after one warm-up call each, the two calls alternating), plus the tracts' bases and the phase-cell updates
(bases x motif length).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_extend.py --reps 1 ...` (k_extend<P> against k_structure<P>).

  python tools/gpu_extend.py --out extend.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(name, d, reps):
    motifs = [u for _, u, _ in d["regions"]]
    rr = d["read_region"] if d["read_region"] is not None else np.zeros(len(d["reads"]), np.int32)
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    extend = lambda: _capi.extend_tracts(motifs, tracts, rr)
    structure = lambda: _capi.read_structure(motifs, tracts, rr)
    extend(); structure()                                         # warm-up (module load, first allocations)
    t_ext = t_str = float("inf")
    for _ in range(reps):
        t_ext = min(t_ext, timed(extend))
        t_str = min(t_str, timed(structure))
    bases = int(sum(len(t) for t in tracts))
    cells = int(sum(len(t) * len(motifs[int(g)]) for t, g in zip(tracts, rr)))
    row = dict(config=name, reads=len(tracts), tract_bases=bases, phase_cells=cells, extend_call_s=t_ext,
               structure_call_s=t_str, extend_over_structure=t_ext / t_str)
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
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
