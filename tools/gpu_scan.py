"""Measures the repeat scan on one GPU and writes one JSON file.

The chunk is section 13's: the panel's reads repeated up to about 2^28 bases, prepacked.  nra_scan_repeats and
nra_screen_reads_partial run in alternating calls in one process, each from host buffers to host results; medians of
--reps rounds after a warm-up round, kernel times from HIP events (k_scan_repeats from nra_scan_stats_t, k_screen_hits
and k_screen_motifs from nra_screen_stats_t).

  python tools/gpu_scan.py --out scan.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpu_screen  # noqa: E402
from nanorepeat_amd import _capi, screen as nr_screen, synth  # noqa: E402


def bench_scan(p, anchor_len, chunk_bases, reps, k, max_gap, min_span):
    chunk = gpu_screen.panel_chunk(p, chunk_bases)
    data, off = _capi.pack_reads(chunk)
    off_p = _capi._ptr(off, C.c_int64)
    lib = _capi.load()
    motifs = [u for _, _, _, u in p["regions"]]
    scans, partials = [], []
    with nr_screen.Screen(gpu_screen.anchors_of(p, anchor_len), motifs=motifs) as scr:
        cap = 8 * len(chunk) + 1024
        arrs = [np.zeros(cap, np.int32) for _ in range(6)]
        kind = np.zeros(cap, np.uint8)
        ptrs = [_capi._ptr(a, C.c_int32) for a in arrs]
        for rep in range(reps + 1):
            n, st = C.c_int64(cap), _capi.ScanStats()
            t0 = time.perf_counter()
            rc = lib.nra_scan_repeats(0, len(chunk), data, off_p, k, max_gap, min_span, C.byref(n), *ptrs, C.byref(st))
            wall = time.perf_counter() - t0
            _capi._check(rc)
            a = dict(call_ms=wall * 1e3, runs=int(n.value), **st.as_dict())
            n = C.c_int64(cap)
            t0 = time.perf_counter()
            rc = lib.nra_screen_reads_partial(scr._h, len(chunk), data, off_p, 4, 5, C.byref(n), *ptrs[:5],
                                              _capi._ptr(kind, C.c_uint8))
            wall = time.perf_counter() - t0
            _capi._check(rc)
            s = scr.stats()
            b = dict(call_ms=wall * 1e3, hits_kernel_ms=s["kernel_ms"], motif_kernel_ms=s["motif_kernel_ms"],
                     pairs=int(n.value))
            if rep:                                   # the first round is the warm-up
                scans.append(a); partials.append(b)

    def med(rows, key):
        return float(np.median([r[key] for r in rows]))
    bases = int(off[-1])
    scan_ms, motif_ms = med(scans, "kernel_ms"), med(partials, "motif_kernel_ms")
    return dict(reads=len(chunk), bases=bases, k=k, max_gap=max_gap, min_span=min_span, scan_repeats=scans,
                screen_reads_partial=partials,
                median=dict(scan_kernel_ms=scan_ms, motif_kernel_ms=motif_ms, hits_kernel_ms=med(partials, "hits_kernel_ms"),
                            scan_over_motifs=scan_ms / motif_ms, scan_bases_per_s=bases / (scan_ms * 1e-3),
                            segments_per_megabase=scans[-1]["n_segments"] / (bases * 1e-6),
                            scan_call_ms=med(scans, "call_ms"), screen_reads_partial_call_ms=med(partials, "call_ms")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=46)
    ap.add_argument("--anchor-len", type=int, default=1000)
    ap.add_argument("--chunk-bases", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", type=int, default=11)
    ap.add_argument("--max-gap", type=int, default=100)
    ap.add_argument("--min-span", type=int, default=200)
    ap.add_argument("--out", default="scan.json")
    a = ap.parse_args()
    res = dict(args=vars(a))
    t0 = time.perf_counter()
    p = synth.panel(a.regions, anchor_len=a.anchor_len, reads_per_region=a.reads_per_region, edge_overlaps=(150, 300),
                    n_decoys=a.regions, shared=a.regions // 25, seed=33)
    res["panel"] = dict(regions=a.regions, reads=len(p["reads"]), bases=sum(len(s) for _, s in p["reads"]),
                        gen_s=time.perf_counter() - t0)
    res["scan"] = bench_scan(p, a.anchor_len, a.chunk_bases, a.reps, a.k, a.max_gap, a.min_span)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["scan"]["median"]))


if __name__ == "__main__":
    main()
