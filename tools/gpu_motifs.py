"""Measures the tandem motif call (nra_tract_motifs) next to round 3 on the same reads, on one GPU,
and the re-sizing accuracy on synth.motif_panel; writes one JSON file.

For config 2 (10 k reads, TATTG) and config 4 (--regions x --reads-per-region, 3-6 bp motifs) the tracts are the reads'
cores without their 100-base flanks.  Per config: the wall time of one nra_tract_motifs call over all tracts (best of
--reps, after one warm-up call) and of one nra_round3_1d call over the cores (best of --reps).  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_motifs.py --reps 1 --no-panel`
(k_tract_motifs against round 3's kernels).  The panel: the FASTQ command with discover_motifs=True, then per planted
allele whose class differs from the BED class the median Size_In_Motif of the reads that call it.

  python tools/gpu_motifs.py --out motifs.json [--configs 2,4] [--regions 1000] [--reads-per-region 1000]
"""
import argparse
import json
import os
import sys
import tempfile
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


def measure(name, d, reps):
    tracts = [s[FLANK:max(FLANK, len(s) - FLANK)] for s in d["reads"]]
    _capi.tract_motifs(tracts)                                    # warm-up (module load, first allocations)
    t_motif = best_of(lambda: _capi.tract_motifs(tracts), reps)
    call, _ = _capi.prepared_round3_1d(d["regions"], d["reads"], d["kmin"], d["kmax"], read_region=d["read_region"])
    call()
    t_r3 = best_of(call, reps)
    bases = int(sum(len(t) for t in tracts))
    row = dict(config=name, reads=len(tracts), tract_bases=bases, motif_call_s=t_motif, round3_call_s=t_r3,
               motif_over_round3=t_motif / t_r3)
    print(json.dumps(row), flush=True)
    return row


def panel(seed):
    from nanorepeat_amd import motifs, pipeline
    p = synth.motif_panel(model="hifi", seed=seed)
    with tempfile.TemporaryDirectory() as tmp:
        ref, bed, reads = synth.write_panel(p, tmp)
        regions = pipeline.quantify_from_reads(reads, ref, bed, os.path.join(tmp, "o"), data_type="hifi",
                                               discover_motifs=True, seed=3)
    rows = []
    for g, region in enumerate(regions):
        bed_cls = motifs.bed_class(region.repeat_unit_seq)
        for a, (cls, units) in enumerate(p["planted"][g]):
            names = [n for n, (gg, aa) in p["truth"].items() if gg == g and aa == a]
            rms = [region.read_motifs[n] for n in names if n in region.read_motifs]
            called = [rm for rm in rms if rm.call == cls]
            sizes = [rm.size_in_motif for rm in called if rm.size_in_motif is not None]
            rows.append(dict(region=region.to_unique_id(), allele=a, planted=cls, units=units, reads=len(names),
                             with_core=len(rms), calling_planted=len(called), resized=cls != bed_cls,
                             median_size_in_motif=float(np.median(sizes)) if sizes else None))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-panel", action="store_true")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    rows = []
    for c in a.configs.split(","):
        if c == "2":
            rows.append(measure("config2", synth.config2(), a.reps))
        elif c == "4":
            rows.append(measure("config4", synth.config4(a.regions, a.reads_per_region), a.reps))
        else:
            raise SystemExit(f"unknown config {c}")
    result = dict(calls=rows, panel=None if a.no_panel else panel(a.seed))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
