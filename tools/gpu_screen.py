"""Measures the FASTQ / FASTA command's anchor screen on one GPU and writes one JSON file.

  index   nra_screen_create at --index-regions regions of random 1 kb anchors (host build time)
  screen  nra_screen_reads per chunk of about 2^28 read bases from prepacked host buffers (the panel's reads repeated),
          with the screen kernels' time from HIP events -> read bases/s
  e2e     quantify_from_reads on the --regions panel split into parsing, screen, anchors, rounds 1-2, round 3, phasing;
          recall of the truth reads (offered by the screen / accepted by the anchor check)
  recall  a smaller panel with reads that end inside an anchor: screen=True against screen=False, per anchor overlap

--partial: the motif screen alone, on the same chunk: nra_screen_reads and nra_screen_reads_partial in
alternating calls on one handle, each from host buffers to host results, with k_screen_hits' and k_screen_motifs' time
from HIP events (the partial call runs both kernels on one upload).

--only anchors: the screen and the anchor stage alone on the panel (no other kernels), for a rocprofv3 kernel trace that
compares k_screen_hits with the anchor stage's kernels.

  python tools/gpu_screen.py --out screen.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nanorepeat_amd import _capi, io as nr_io, pipeline, round3, screen as nr_screen, synth, upstream  # noqa: E402


class Timers:
    """Wall time of the pipeline's steps, by wrapping the module functions the command calls."""

    def __init__(self):
        self.t = {}

    def wrap(self, module, name, label):
        fn = getattr(module, name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.t[label] = self.t.get(label, 0.0) + time.perf_counter() - t0
        setattr(module, name, timed)
        return fn

    def wrap_gen(self, module, name, label):
        fn = getattr(module, name)

        def timed(*a, **kw):
            it = fn(*a, **kw)
            while True:
                t0 = time.perf_counter()
                try:
                    item = next(it)
                except StopIteration:
                    self.t[label] = self.t.get(label, 0.0) + time.perf_counter() - t0
                    return
                self.t[label] = self.t.get(label, 0.0) + time.perf_counter() - t0
                yield item
        setattr(module, name, timed)
        return fn


def bench_index(n_regions, anchor_len=1000, seed=1):
    rng = np.random.default_rng(seed)
    anchors = [(synth.rand_seq(rng, anchor_len), synth.rand_seq(rng, anchor_len)) for _ in range(n_regions)]
    t0 = time.perf_counter()
    with nr_screen.Screen(anchors) as scr:
        wall = time.perf_counter() - t0
        st = scr.stats()
    return dict(regions=n_regions, build_ms=st["build_ms"], create_wall_ms=wall * 1e3, keys=st["n_keys"],
                postings=st["n_postings"], index_bytes=st["index_bytes"], masked_periodic=st["n_masked_periodic"],
                masked_max_occ=st["n_masked_max_occ"])


def anchors_of(p, anchor_len):
    return [(p["ref"][c][max(0, st - anchor_len):st], p["ref"][c][en:en + anchor_len]) for c, st, en, _ in p["regions"]]


def bench_screen(p, anchor_len, chunk_bases, reps):
    """nra_screen_reads over one chunk of ~chunk_bases bases, prepacked: the C call alone."""
    seqs = [s for _, s in p["reads"]]
    chunk, size = [], 0
    while size < chunk_bases:                         # the panel's reads, repeated up to chunk_bases
        for s in seqs:
            chunk.append(s)
            size += len(s)
            if size >= chunk_bases:
                break
    data, off = _capi.pack_reads(chunk)
    lib = _capi.load()
    out = []
    with nr_screen.Screen(anchors_of(p, anchor_len)) as scr:
        cap = 4 * len(chunk) + 1024
        arrs = [np.zeros(cap, np.int32) for _ in range(4)]
        for rep in range(reps + 1):
            n = C.c_int64(cap)
            t0 = time.perf_counter()
            rc = lib.nra_screen_reads(scr._h, len(chunk), data, _capi._ptr(off, C.c_int64), 4, C.byref(n),
                                      *(_capi._ptr(a, C.c_int32) for a in arrs))
            wall = time.perf_counter() - t0
            _capi._check(rc)
            st = scr.stats()
            if rep:                                   # the first call is the warm-up
                out.append(dict(call_ms=wall * 1e3, kernel_ms=st["kernel_ms"], pairs=int(n.value)))
    bases = int(off[-1])
    kern = float(np.median([o["kernel_ms"] for o in out]))
    call = float(np.median([o["call_ms"] for o in out]))
    return dict(reads=len(chunk), bases=bases, calls=out, kernel_ms_median=kern, call_ms_median=call,
                kernel_bases_per_s=bases / (kern * 1e-3), call_bases_per_s=bases / (call * 1e-3),
                index=scr_stats_keys(st))


def panel_chunk(p, chunk_bases):
    seqs = [s for _, s in p["reads"]]
    chunk, size = [], 0
    while size < chunk_bases:                         # the panel's reads, repeated up to chunk_bases
        for s in seqs:
            chunk.append(s)
            size += len(s)
            if size >= chunk_bases:
                break
    return chunk


def bench_partial(p, anchor_len, chunk_bases, reps):
    """nra_screen_reads and nra_screen_reads_partial in alternating calls over one prepacked chunk of ~chunk_bases."""
    chunk = panel_chunk(p, chunk_bases)
    data, off = _capi.pack_reads(chunk)
    lib = _capi.load()
    motifs = [u for _, _, _, u in p["regions"]]
    plain, partial = [], []
    with nr_screen.Screen(anchors_of(p, anchor_len), motifs=motifs) as scr:
        cap = 8 * len(chunk) + 1024
        arrs = [np.zeros(cap, np.int32) for _ in range(5)]
        kind = np.zeros(cap, np.uint8)
        ptrs = [_capi._ptr(a, C.c_int32) for a in arrs]
        for rep in range(reps + 1):
            n = C.c_int64(cap)
            t0 = time.perf_counter()
            rc = lib.nra_screen_reads(scr._h, len(chunk), data, _capi._ptr(off, C.c_int64), 4, C.byref(n), *ptrs[:4])
            wall = time.perf_counter() - t0
            _capi._check(rc)
            a = dict(call_ms=wall * 1e3, hits_kernel_ms=scr.stats()["kernel_ms"], pairs=int(n.value))
            n = C.c_int64(cap)
            t0 = time.perf_counter()
            rc = lib.nra_screen_reads_partial(scr._h, len(chunk), data, _capi._ptr(off, C.c_int64), 4, 5, C.byref(n),
                                              *ptrs, _capi._ptr(kind, C.c_uint8))
            wall = time.perf_counter() - t0
            _capi._check(rc)
            st = scr.stats()
            b = dict(call_ms=wall * 1e3, hits_kernel_ms=st["kernel_ms"], motif_kernel_ms=st["motif_kernel_ms"],
                     pairs=int(n.value), kinds=np.bincount(kind[:n.value], minlength=4).tolist())
            if rep:                                   # the first round is the warm-up
                plain.append(a); partial.append(b)
        n_classes = st["n_classes"]

    def med(rows, key):
        return float(np.median([r[key] for r in rows]))
    return dict(reads=len(chunk), bases=int(off[-1]), n_classes=n_classes, screen_reads=plain, screen_reads_partial=partial,
                median=dict(hits_kernel_ms=med(plain, "hits_kernel_ms"), hits_kernel_ms_in_partial=med(partial, "hits_kernel_ms"),
                            motif_kernel_ms=med(partial, "motif_kernel_ms"), screen_reads_call_ms=med(plain, "call_ms"),
                            screen_reads_partial_call_ms=med(partial, "call_ms")))


def scr_stats_keys(st):
    return {k: st[k] for k in ("n_keys", "n_postings", "n_masked_periodic", "n_masked_max_occ", "index_bytes", "build_ms")}


def offered_recall(p, regions):
    """Truth reads that reached their region (offered by the screen / accepted by the anchor check)."""
    n = len(p["truth"])
    found = {(name, region.index) for region in regions for name in region.read_dict}
    accepted = sum((name, g) in found for name, (g, _) in p["truth"].items())
    return dict(truth_reads=n, accepted_by_anchor_check=accepted, recall_vs_truth=accepted / max(n, 1))


def run_e2e(p, anchor_len, work, only_anchors=False):
    ref, bed, reads = synth.write_panel(p, work)
    timers = Timers()
    timers.wrap_gen(nr_io, "iter_reads", "parsing")
    timers.wrap(nr_screen.Screen, "screen_reads", "screen_kernels_call")
    timers.wrap(nr_screen, "reads_by_region", "read_selection")
    timers.wrap(upstream, "find_anchor_locations_in_reads_many", "anchors")
    timers.wrap(upstream, "round1_and_round2_estimation_many", "rounds_1_2")
    timers.wrap(round3, "round3_estimation_regions", "round3")
    timers.wrap(pipeline, "phase_regions", "phasing")
    if only_anchors:
        regions = nr_io.read_repeat_region_file(bed)
        refd = nr_io.fasta_file2dict(ref)
        for i, r in enumerate(regions):
            r.index = i
            nr_io.extract_ref_sequence(refd, r, anchor_len)
        t0 = time.perf_counter()
        found = nr_screen.reads_by_region(reads, regions)
        upstream.find_anchor_locations_in_reads_many(
            "ont", regions, [{n: s for n, (s, _) in f.items()} for f in found])
        total = time.perf_counter() - t0
    else:
        t0 = time.perf_counter()
        regions = pipeline.quantify_from_reads(reads, ref, bed, os.path.join(work, "out"), data_type="ont",
                                               anchor_len=anchor_len, seed=1)
        total = time.perf_counter() - t0
    t = dict(timers.t)
    # reads_by_region = parsing + screen calls + the rest of read selection (create, dict building)
    t["screen"] = t.pop("read_selection", 0.0) - t.get("parsing", 0.0)
    t.pop("screen_kernels_call", None)
    t["total"] = total
    return dict(phase_s=t, **offered_recall(p, regions))


def run_recall(n_regions, anchor_len, work, model, seed):
    overlaps = (150, 300, 600, 1000)
    p = synth.panel(n_regions, anchor_len=anchor_len, reads_per_region=2, edge_overlaps=overlaps, n_decoys=0,
                    model=model, seed=seed)
    ref, bed, reads = synth.write_panel(p, work)
    res = {}
    for mode in (True, False):
        regions = pipeline.quantify_from_reads(reads, ref, bed, os.path.join(work, f"r{int(mode)}"), data_type=model,
                                               anchor_len=anchor_len, seed=1, screen=mode)
        res[mode] = {(name, region.index) for region in regions for name in region.read_dict}
    table = []
    for o in overlaps:
        names = [n for n, ov in p["overlap"].items() if min(ov) == o]
        want = [(n, p["truth"][n][0]) for n in names]
        exh = sum(x in res[False] for x in want)
        scr = sum(x in res[True] for x in want)
        table.append(dict(anchor_overlap=o, reads=len(names), accepted_exhaustive=exh, accepted_screened=scr,
                          recall_vs_exhaustive=scr / max(exh, 1)))
    extra = len(res[True] - res[False])
    return dict(regions=n_regions, model=model, table=table, screened_not_exhaustive=extra,
                identical=res[True] == res[False])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads-per-region", type=int, default=46)
    ap.add_argument("--anchor-len", type=int, default=1000)
    ap.add_argument("--index-regions", default="1000,10000")
    ap.add_argument("--chunk-bases", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--recall-regions", type=int, default=40)
    ap.add_argument("--only", choices=("all", "anchors", "screen"), default="all")
    ap.add_argument("--partial", action="store_true", help="the motif screen against the anchor screen, alone")
    ap.add_argument("--out", default="screen.json")
    a = ap.parse_args()
    res = dict(args=vars(a))
    t0 = time.perf_counter()
    p = synth.panel(a.regions, anchor_len=a.anchor_len, reads_per_region=a.reads_per_region, edge_overlaps=(150, 300),
                    n_decoys=a.regions, shared=a.regions // 25, seed=33)
    res["panel"] = dict(regions=a.regions, reads=len(p["reads"]), bases=sum(len(s) for _, s in p["reads"]),
                        gen_s=time.perf_counter() - t0)
    with tempfile.TemporaryDirectory() as work:
        if a.partial:
            res["partial"] = bench_partial(p, a.anchor_len, a.chunk_bases, a.reps)
        elif a.only == "anchors":
            res["anchors_only"] = run_e2e(p, a.anchor_len, work, only_anchors=True)
        elif a.only == "screen":
            res["screen"] = bench_screen(p, a.anchor_len, a.chunk_bases, 1)
        else:
            res["index"] = [bench_index(int(n)) for n in a.index_regions.split(",")]
            res["screen"] = bench_screen(p, a.anchor_len, a.chunk_bases, a.reps)
            res["e2e"] = run_e2e(p, a.anchor_len, work)
            res["recall"] = run_recall(a.recall_regions, a.anchor_len, work, "ont", seed=44)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "args"})[:3000])


if __name__ == "__main__":
    main()
