"""Measures the placement scan on one GPU and writes one JSON file.

Workload: --ref-bases random reference bases in one contig (default 2^28) and --sides sides of 1000 bases cut from it
through `ont` errors, every second one reverse-complemented.  One call = nra_place_create, nra_place_scan over chunks of
--chunk-bases bases with the k - 1 overlap, nra_place_candidates; for every -k, medians of --reps calls after a warm-up
call.  The kernel time is from HIP events, the upload and reduce times are the host's (nra_place_stats_t).  The same
sides against the first --cpu-bases bases also go through tests/place_ref.py's numpy form once, on the same machine,
for the ratio per target base.

  python tools/gpu_place.py --out profiles/place_scan.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nanorepeat_amd import _capi, place, synth  # noqa: E402


def workload(ref_bases, n_sides, seed=5):
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ref_bases, dtype=np.uint8)].tobytes()
    at = rng.integers(0, ref_bases - 1000, n_sides)
    sides = synth.apply_errors_batch(rng, [ref[a:a + 1000].decode() for a in at], "ont")
    sides = [(synth.revcomp(s) if i % 2 else s)[:place.MAX_SIDE] for i, s in enumerate(sides)]
    return ref, sides, at


def one_call(ref, sides, k, chunk, bin, max_target_occ, min_votes):
    t0 = time.perf_counter()
    h = _capi.place_create(sides, k, place.MAX_OCC)
    try:
        step = chunk - (k - 1)
        for pos0 in range(0, max(1, len(ref) - (k - 1)), step):
            _capi.place_scan(h, 0, pos0, ref[pos0:pos0 + chunk])
        got = _capi.place_candidates(h, bin, max_target_occ, min_votes)
        st = _capi.place_stats(h)
    finally:
        _capi.place_destroy(h)
    return dict(call_ms=(time.perf_counter() - t0) * 1e3, candidates=len(got["query"]), **st), got


def cpu_reference(ref, sides, k, bin, max_target_occ, min_votes):
    import place_ref
    t0 = time.perf_counter()
    got, stats = place_ref.candidates_numpy(sides, [(0, 0, ref.decode())], k, place.MAX_OCC, bin, max_target_occ,
                                            min_votes)
    return dict(bases=len(ref), sides=len(sides), seconds=time.perf_counter() - t0, candidates=len(got),
                n_hits_kept=stats["n_hits_kept"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bases", type=int, default=1 << 28)
    ap.add_argument("--sides", type=int, default=2000)
    ap.add_argument("--chunk-bases", type=int, default=place.CHUNK_BASES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, nargs="*", default=[place.K, 13])
    ap.add_argument("--bin", type=int, default=place.BIN)
    ap.add_argument("--min-votes", type=int, default=place.MIN_VOTES)
    ap.add_argument("--max-target-occ", type=int, default=place.MAX_TARGET_OCC)
    ap.add_argument("--cpu-bases", type=int, default=1 << 22)
    ap.add_argument("--out", default="place_scan.json")
    a = ap.parse_args()
    ref, sides, at = workload(a.ref_bases, a.sides)
    res = dict(args=vars(a), workloads=[],
               screen_context="k_screen_hits reads 39 G bases/s (DESIGN.md section 13): another index and hit rate")
    for k in a.k:
        calls = []
        for rep in range(a.reps + 1):
            c, got = one_call(ref, sides, k, a.chunk_bases, a.bin, a.max_target_occ, a.min_votes)
            if rep:                                   # the first call is the warm-up
                calls.append(c)
        med = {key: float(np.median([c[key] for c in calls])) for key in ("call_ms", "build_ms", "kernel_ms",
                                                                          "upload_ms", "reduce_ms")}
        med.update(kernel_gbases_per_s=a.ref_bases / (med["kernel_ms"] * 1e6),
                   reduce_share=med["reduce_ms"] / med["call_ms"], upload_share=med["upload_ms"] / med["call_ms"],
                   kernel_share=med["kernel_ms"] / med["call_ms"])
        # how many sides have their best candidate where they were cut from
        best = {}
        for q, t, s, b, v in zip(*(got[key].tolist() for key in _capi.PLACE_KEYS)):
            if v > best.get(q, (0,))[0]:
                best[q] = (v, s, b)
        home = sum(1 for q, (v, s, b) in best.items() if s == q % 2 and abs(b * a.bin - int(at[q])) <= 3 * a.bin)
        w = dict(k=k, calls=calls, median=med, sides_placed_where_cut=home)
        print(json.dumps(dict(k=k, **med, sides_placed_where_cut=home, n_hits_kept=calls[-1]["n_hits_kept"])), flush=True)
        if a.cpu_bases:
            cpu = cpu_reference(ref[:a.cpu_bases], sides, k, a.bin, a.max_target_occ, a.min_votes)
            cpu["per_base_over_gpu_call"] = (cpu["seconds"] / cpu["bases"]) / (med["call_ms"] * 1e-3 / a.ref_bases)
            w["cpu_numpy"] = cpu
            print(json.dumps(cpu), flush=True)
        res["workloads"].append(w)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
