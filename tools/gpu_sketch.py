"""Measures the sketch pairs on one GPU and writes one JSON file.

Workloads: n sides of 500 bases in one group, n / 20 loci with 20 copies each through `ont` errors, half of them
reverse-complemented, prepacked.  nra_sketch_pairs runs from host buffers to host results; medians of --reps calls after
a warm-up call, kernel times from HIP events and the host's upload and sort times from nra_sketch_stats_t.  --cpu-sides
sides also go through tests/sketch_ref.py's numpy form once, on the same machine.  --round-trip runs the locus commands
on the test panel with `ont` errors and counts the reads that pass the anchor check against the pseudo-reference.

  python tools/gpu_sketch.py --out sketch.json
"""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nanorepeat_amd import _capi, synth  # noqa: E402


def sides(n, flank=500, copies=20, model="ont", seed=5):
    rng = np.random.default_rng(seed)
    loci = [synth.rand_seq(rng, flank) for _ in range((n + copies - 1) // copies)]
    out = synth.apply_errors_batch(rng, [loci[i // copies] for i in range(n)], model)
    return [synth.revcomp(s) if i % 2 else s for i, s in enumerate(out)]


def bench(n, reps, k, min_shared):
    seqs = sides(n)
    data, off = _capi.pack_reads(seqs)
    grp = np.zeros(n, np.int32)
    lib = _capi.load()
    cap = 64 * n
    arrs = [np.zeros(cap, np.int32) for _ in range(3)]
    size = np.zeros(n, np.int32)
    calls = []
    for rep in range(reps + 1):
        n_pairs, st = C.c_int64(cap), _capi.SketchStats()
        t0 = time.perf_counter()
        rc = lib.nra_sketch_pairs(0, n, data, _capi._ptr(off, C.c_int64), _capi._ptr(grp, C.c_int32), k, min_shared,
                                  C.byref(n_pairs), *(_capi._ptr(a, C.c_int32) for a in arrs),
                                  _capi._ptr(size, C.c_int32), C.byref(st))
        wall = time.perf_counter() - t0
        _capi._check(rc)
        if rep:                                       # the first call is the warm-up
            calls.append(dict(call_ms=wall * 1e3, pairs=int(n_pairs.value), **st.as_dict()))

    def med(key):
        return float(np.median([c[key] for c in calls]))
    m = {key: med(key) for key in ("call_ms", "sketch_ms", "pairs_ms", "upload_ms", "sort_ms")}
    m.update(compared_per_s=calls[-1]["n_compared"] / (m["pairs_ms"] * 1e-3),
             host_share=(m["upload_ms"] + m["sort_ms"]) / m["call_ms"],
             kernel_share=(m["sketch_ms"] + m["pairs_ms"]) / m["call_ms"])
    return dict(sides=n, bases=int(off[-1]), k=k, min_shared=min_shared, calls=calls, median=m), seqs


def cpu_reference(seqs, k, min_shared):
    import sketch_ref
    t0 = time.perf_counter()
    pairs, _, stats = sketch_ref.pairs_numpy(seqs, [0] * len(seqs), k, min_shared)
    return dict(sides=len(seqs), seconds=time.perf_counter() - t0, pairs=len(pairs), n_compared=stats["n_compared"])


def round_trip(model):
    import test_loci_gpu
    with tempfile.TemporaryDirectory() as d:
        p, table, runs, regions = test_loci_gpu.round_trip(pathlib.Path(d), model, model)
    spanning = {x: {n for n, y in p["locus"].items() if y == x} for x in "ABC"}
    cores = {}
    for name, _, _, _, locus, role, _ in runs:
        if role == "core":
            cores.setdefault(locus, set()).add(name)
    out = dict(model=model, loci=[{k: c[k] for k in ("Locus", "Class", "Type", "Spanned", "Min_Copies", "Max_Copies")}
                                  for c in table], regions=[])
    for r in regions:
        mine = cores.get(r.chrom[len("locus_"):], set())
        planted = max(spanning.values(), key=lambda s: len(s & mine))
        alleles = getattr(getattr(r, "results", None), "quantified_allele_list", [])
        out["regions"].append(dict(contig=r.chrom, unit=r.repeat_unit_seq, motif_check=not getattr(r, "ref_has_issue", True),
                                   spanning_reads_planted=len(planted), reads_passing_anchors=len(set(r.read_dict) & planted),
                                   alleles=sorted(int(a.repeat_size1) for a in alleles)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="*", default=[2000, 20000, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=13)
    ap.add_argument("--min-shared", type=int, default=8)
    ap.add_argument("--cpu-sides", type=int, default=2000)
    ap.add_argument("--round-trip", action="store_true")
    ap.add_argument("--out", default="sketch.json")
    a = ap.parse_args()
    res = dict(args=vars(a), workloads=[])
    for n in a.sides:
        w, seqs = bench(n, a.reps, a.k, a.min_shared)
        res["workloads"].append(w)
        print(json.dumps(dict(sides=n, **w["median"])), flush=True)
        if n == a.cpu_sides:
            res["cpu_numpy"] = cpu_reference(seqs, a.k, a.min_shared)
            res["cpu_numpy"]["over_gpu_call"] = res["cpu_numpy"]["seconds"] * 1e3 / w["median"]["call_ms"]
            print(json.dumps(res["cpu_numpy"]), flush=True)
    if a.round_trip:
        res["round_trip"] = [round_trip(m) for m in ("hifi", "ont")]
        print(json.dumps(res["round_trip"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
