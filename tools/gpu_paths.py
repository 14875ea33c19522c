"""Times nra_align_paths against nra_align_pairs on the same pairs and writes one JSON line.

The pairs are the cores of config 5 (hifi, TATTG, alleles of 60 and 420 units: cores of 0.5 and 2.3 kb) with a third
allele of --long-units units whose cores pass 3072 bases and run in chained row blocks, each core against the template
of its true size (1 kb anchors).  Both calls are timed whole, as the pipeline pays them: host packing, transfers,
kernels and, for the paths, the walk back and the CIGAR strings.  No target is set: the trace is one byte stored per
cell.

  python tools/gpu_paths.py --reads 300 --out paths.json
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


def timed(fn, repeats):
    fn()                                                   # warm-up: module load, arena growth
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=300)
    ap.add_argument("--long-units", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = synth.make_1d(a.reads, "TATTG", (60, 420, a.long_units), "hifi", kwin=(5, 500), seed=synth.SEED)
    left, unit, right = d["regions"][0]
    templates = {int(k): left + unit * int(k) + right for k in set(d["k_true"].tolist())}
    keys = sorted(templates)
    seqs = list(d["reads"]) + [templates[k] for k in keys]
    pq = list(range(a.reads))
    pt = [a.reads + keys.index(int(k)) for k in d["k_true"]]
    cells = sum(len(seqs[q]) * len(seqs[t]) for q, t in zip(pq, pt))
    t_pairs, p = timed(lambda: _capi.align_pairs(seqs, pq, pt), a.repeats)
    t_paths, g = timed(lambda: _capi.align_paths_chunked(seqs, pq, pt), a.repeats)
    for k in ("score", "tstart", "tend"):
        assert np.array_equal(p[k], g[k]), k
    res = dict(reads=a.reads, alleles=[60, 420, a.long_units], cells=cells,
               queries_beyond_3072=int(sum(len(seqs[q]) > 3072 for q in pq)),
               align_pairs_s=round(t_pairs, 4), align_paths_s=round(t_paths, 4), ratio=round(t_paths / t_pairs, 2),
               pairs_gcells_per_s=round(cells / t_pairs / 1e9, 1), paths_gcells_per_s=round(cells / t_paths / 1e9, 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
