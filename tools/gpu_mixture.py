"""Measures the phasing step with the GPU mixture engine (nra_mixture_fit) next to the default
engine on the 1000-region panel of section 13, on one GPU, and writes one JSON file.

The panel is synth.panel(--regions, anchor_len=1000, reads_per_region=46, ...) as in tests/test_screen_gpu.py.  One
run of pipeline.quantify_from_reads with mixture="gpu" gives the steps' wall times (screen, anchors, phasing) and the
regions with their round-3 sizes; pipeline.phase_regions then runs on those regions with mixture="gpu" and with the
default engine (its 16 worker processes), alternating, --reps times each.  The GPU path's time is split into: the
samples and start rows, the nra_mixture_fit calls (host buffers to host results), the order rule and the
classification, and the files.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_mixture.py --reps 1 --no-default` (k_mixture<D, KREG>).

  python tools/gpu_mixture.py --out mixture.json [--regions 1000] [--reps 3] [--no-default]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanorepeat_amd import _capi, mixture, pipeline, synth, upstream  # noqa: E402


class Clock:
    """Wall time spent inside wrapped functions, by name."""

    def __init__(self):
        self.t = {}

    def wrap(self, name, fn):
        def inner(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return inner

    def take(self):
        out, self.t = self.t, {}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-default", action="store_true")
    a = ap.parse_args()
    clock = Clock()
    captured = {}
    phase_regions = pipeline.phase_regions

    def capture(regions, *args, **kw):
        captured["regions"], captured["args"] = regions, args
        return phase_regions(regions, *args, **kw)

    fits = []

    def engine(samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts, **kw):
        fits.append(len(fit_n))
        return _capi.mixture_fit(samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts, **kw)

    pipeline.phase_regions = clock.wrap("phasing", capture)
    upstream.find_anchor_locations_in_reads_many = clock.wrap("anchors", upstream.find_anchor_locations_in_reads_many)
    mixture.phase_jobs = clock.wrap("phase_jobs", mixture.phase_jobs)
    mixture.sample = clock.wrap("sample", mixture.sample)
    mixture.start_rows = clock.wrap("start_rows", mixture.start_rows)
    timed_engine = clock.wrap("call", engine)
    with tempfile.TemporaryDirectory() as tmp:
        p = synth.panel(a.regions, anchor_len=1000, reads_per_region=46, edge_overlaps=(150, 300),
                        n_decoys=a.regions, shared=min(40, a.regions), seed=33)
        ref, bed, reads = synth.write_panel(p, tmp)
        t0 = time.perf_counter()
        pipeline.quantify_from_reads(reads, ref, bed, os.path.join(tmp, "run"), seed=1, mixture="gpu",
                                     mixture_engine=timed_engine)
        command = dict(clock.take(), total=time.perf_counter() - t0)
        row = dict(regions=a.regions, reads=len(p["reads"]), command_s=command,
                   phasing_shorter_than_anchors=command["phasing"] < command["anchors"], runs=[])
        print(json.dumps(row), flush=True)
        regions, args = captured["regions"], captured["args"]
        for rep in range(a.reps):
            for name in ("gpu",) if a.no_default else ("gpu", "sklearn"):
                for region in regions:
                    region.results = None
                del fits[:]
                clock.take()
                t0 = time.perf_counter()
                phase_regions(regions, *args, mixture=name, mixture_engine=timed_engine if name == "gpu" else None)
                wall = time.perf_counter() - t0
                t = clock.take()
                run = dict(engine=name, rep=rep, phase_regions_s=wall)
                if name == "gpu":
                    host = t["sample"] + t["start_rows"]
                    run.update(sample_and_start_rows_s=host, calls=len(fits), fits=sum(fits), call_s=t["call"],
                               order_rule_and_classification_s=t["phase_jobs"] - host - t["call"],
                               files_s=wall - t["phase_jobs"])
                print(json.dumps(run), flush=True)
                row["runs"].append(run)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
