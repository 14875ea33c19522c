"""Measures the allele split call (nra_allele_split) next to the consensus call on the same
groups, on one GPU, and writes one JSON file.

For config 2 (10 k reads, TATTG, two alleles) and config 4 (--regions x --reads-per-region, 3-6 bp motifs, two alleles
per region) the tracts are the reads' cores without their 100-base flanks, grouped by their true allele; the backbone of
a group is its consensus, from the nra_tract_consensus call that is timed beside the split.  Per config: the wall time
of one nra_allele_split call from host buffers to host results (best of --reps, after one warm-up call), of one
nra_tract_consensus call (best of --reps), their ratio, and the split's counters (alignments and tract rows per band
class, launches, widenings, sites, groups split).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_split.py --reps 1` (k_split_align<C>, k_split_count,
k_split_phase against k_cons_align<C>, k_cons_build).

  python tools/gpu_split.py --out split.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nanorepeat_amd import _capi, synth  # noqa: E402
from gpu_consensus import best_of, groups_of  # noqa: E402


def measure(name, d, reps):
    groups = groups_of(d)
    cons = _capi.tract_consensus(groups)                           # warm-up, and the backbones
    bbs = cons["consensus"]
    out = _capi.allele_split(groups, bbs)                          # warm-up
    t_cons = best_of(lambda: _capi.tract_consensus(groups), reps)
    t_split = best_of(lambda: _capi.allele_split(groups, bbs), reps)
    row = dict(config=name, groups=len(groups), tracts=int(sum(len(g) for g in groups)),
               tract_bases=int(sum(len(t) for g in groups for t in g)), split_call_s=t_split, consensus_call_s=t_cons,
               split_over_consensus=t_split / t_cons, consensus_rounds=cons["stats"]["rounds"], stats=out["stats"],
               groups_split=int(out["split"].sum()), sites=int(out["n_sites"].sum()),
               left_out=int(out["left_out"].sum()), iterations_max=int(out["iterations"].max(initial=0)))
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
