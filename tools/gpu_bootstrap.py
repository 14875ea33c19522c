"""Measures the bootstrap of the phasing step (nra_mixture_bootstrap) on the 1000-region panel of
section 13, on one GPU, and writes one JSON file.

The panel is synth.panel(--regions, anchor_len=1000, reads_per_region=46, ...) as in tools/gpu_mixture.py.  One run of
pipeline.quantify_from_reads with mixture="gpu" gives the regions with their round-3 sizes.  pipeline.phase_regions then
runs on them with bootstrap=--replicates, --reps times, alternating in this process with the same replicates of
--composed-regions regions through the composed path (every replicate's sample made on the host and fitted through
mixture.solve with nra_mixture_fit; tests/bootstrap_ref.py), whose time is scaled to all regions.  The bootstrap step is
split into: indices and start rows, the nra_mixture_bootstrap calls (host buffers to host results), the alleles of the
replicates and the statistics, and the files.  Coverage, from the last device run: the share of intervals that hold the
planted size and the called size, over the alleles of regions whose called count is the planted one.  The composed
path's engine is the tests' restatement (tests/bootstrap_ref.py), imported only when that path is run.  Kernel times come from a separate run
under `rocprofv3 --kernel-trace --stats -- python tools/gpu_bootstrap.py --reps 1 --composed-regions 0`.

  python tools/gpu_bootstrap.py --out bootstrap.json [--regions 1000] [--replicates 200] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanorepeat_amd import _capi, bootstrap, mixture, pipeline, synth  # noqa: E402
from gpu_mixture import Clock  # noqa: E402


def coverage(regions, truth):
    """The intervals the regions carry against the planted alleles (truth: {read: (region index, units)})."""
    planted = {}
    for g, k in truth.values():
        planted.setdefault(g, set()).add(k)
    n = hold_planted = hold_called = same_count = with_call = 0
    for region in regions:
        boot = getattr(region, "bootstrap", None)
        if boot is None:
            continue
        with_call += 1
        want = sorted(planted.get(region.index, ()))
        if len(want) != len(boot.rows):
            continue
        same_count += 1
        for k, (size, _, lo, hi, _) in zip(want, boot.rows):
            if lo is None:
                continue
            n += 1
            hold_planted += lo <= k <= hi
            hold_called += lo <= size <= hi
    return dict(regions_with_call=with_call, regions_with_planted_count=same_count, intervals=n,
                hold_planted=hold_planted / max(1, n), hold_called=hold_called / max(1, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-regions", type=int, default=20)
    a = ap.parse_args()
    clock = Clock()
    captured = {}
    phase_regions = pipeline.phase_regions

    def capture(regions, *args, **kw):
        captured["regions"], captured["args"] = regions, args
        return phase_regions(regions, *args, **kw)

    calls = []

    def engine(*args, **kw):
        calls.append(len(args[2]) * int(args[10]))
        return _capi.mixture_bootstrap(*args, **kw)

    pipeline.phase_regions = capture
    bootstrap.bootstrap_regions = clock.wrap("bootstrap_regions", bootstrap.bootstrap_regions)
    bootstrap.alleles_of_replicates = clock.wrap("alleles", bootstrap.alleles_of_replicates)
    bootstrap.RegionBootstrap = clock.wrap("statistics", bootstrap.RegionBootstrap)
    bootstrap.write_region_bootstrap = clock.wrap("files", bootstrap.write_region_bootstrap)
    bootstrap.write_bootstrap_summary = clock.wrap("files", bootstrap.write_bootstrap_summary)
    mixture.bootstrap = clock.wrap("mixture_bootstrap", mixture.bootstrap)
    timed_engine = clock.wrap("call", engine)
    with tempfile.TemporaryDirectory() as tmp:
        p = synth.panel(a.regions, anchor_len=1000, reads_per_region=46, edge_overlaps=(150, 300),
                        n_decoys=a.regions, shared=min(40, a.regions), seed=33)
        ref, bed, reads = synth.write_panel(p, tmp)
        pipeline.quantify_from_reads(reads, ref, bed, os.path.join(tmp, "run"), seed=1, mixture="gpu")
        regions, args = captured["regions"], captured["args"]
        row = dict(regions=len(regions), replicates=a.replicates, runs=[])
        for rep in range(a.reps):
            for region in regions:
                region.results = None
            del calls[:]
            clock.take()
            t0 = time.perf_counter()
            phase_regions(regions, *args, mixture="gpu", bootstrap=a.replicates, bootstrap_engine=timed_engine,
                          bootstrap_tsv_file=os.path.join(tmp, "boot.tsv"))
            wall = time.perf_counter() - t0
            t = clock.take()
            step = t["bootstrap_regions"] + t["files"]
            run = dict(path="device", rep=rep, phase_regions_s=wall, bootstrap_step_s=step, calls=len(calls),
                       replicates_run=sum(calls), call_s=t["call"],
                       indices_and_start_rows_s=t["mixture_bootstrap"] - t["call"],
                       alleles_and_statistics_s=t["alleles"] + t["statistics"], files_s=t["files"])
            print(json.dumps(run), flush=True)
            row["runs"].append(run)
            row["coverage"] = coverage(regions, p["truth"])
            if a.composed_regions:
                sys.path.append(os.path.join(ROOT, "tests"))
                from bootstrap_ref import composed_engine
                some = [r for r in regions if getattr(r, "bootstrap", None) is not None][:a.composed_regions]
                scale = sum(getattr(r, "bootstrap", None) is not None for r in regions) / len(some)
                for region in some:
                    region.results = None
                clock.take()
                phase_regions(some, *args, mixture="gpu", bootstrap=a.replicates,
                              bootstrap_engine=composed_engine(_capi.mixture_fit),
                              bootstrap_tsv_file=os.path.join(tmp, "boot_composed.tsv"))
                t = clock.take()
                step_c = (t["bootstrap_regions"] + t["files"]) * scale
                run = dict(path="composed", rep=rep, regions=len(some), scale=scale, bootstrap_step_scaled_s=step_c,
                           ratio_composed_over_device=step_c / step)
                print(json.dumps(run), flush=True)
                row["runs"].append(run)
    print(json.dumps(row["coverage"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
