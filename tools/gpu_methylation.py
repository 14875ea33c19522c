"""Measures the methylation call (nra_read_methylation) on one GPU; writes one JSON file.

Two workloads, both from host arrays to host arrays (packing, the copies and the chunks included):
  * --reads reads of --length bases with every CpG listed (tract in the middle, the default flank and bin): the wall
    time of one call (median and best of --reps after one warm-up call), the numpy form of the restatement
    (tests/methylation_ref.py, np_read_methylation) on the same reads on this host, and that the two agree;
  * one read of 4 000 000 bases with a quarter of its C listed, alone: the wall time of the call.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_methylation.py
--device-only --reps 1` (k_read_methylation).  NRA_DEBUG=1 in the environment shows the chunks.

  python tools/gpu_methylation.py --out methylation.json [--reads 10000] [--length 20000] [--reps 5] [--device-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nanorepeat_amd import _capi  # noqa: E402

ALPHABET = np.frombuffer(b"ACGT", np.uint8)


def cpg_list(s, reverse):
    """(deltas, probs) naming every CpG of the read (s: uint8 bases, upper case)."""
    is_c = (s[::-1] == ord("G")) if reverse else (s == ord("C"))
    rank = np.cumsum(is_c) - is_c
    site = np.flatnonzero((s[:-1] == ord("C")) & (s[1:] == ord("G")))
    listed = np.sort(rank[len(s) - 2 - site] if reverse else rank[site])
    deltas = np.diff(np.concatenate([[-1], listed])) - 1
    return deltas.astype(np.int32), ((listed * 37) % 256).astype(np.uint8)


def workload(n_reads, length, seed=1):
    rng = np.random.default_rng(seed)
    reads, mods = [], []
    flags = (np.arange(n_reads) % 4).astype(np.uint8)
    for i in range(n_reads):
        s = ALPHABET[rng.integers(0, 4, length)]
        reads.append(s.tobytes().decode())
        mods.append(cpg_list(s, bool(flags[i] & 1)))
    lo = np.full(n_reads, length // 2 - 150, np.int32)
    hi = np.full(n_reads, length // 2 + 150, np.int32)
    return reads, mods, flags, lo, hi


def timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--length", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    args = workload(a.reads, a.length)
    _capi.read_methylation(*args)                                  # warm-up (module load, first allocations)
    got, times = timed(lambda: _capi.read_methylation(*args), a.reps)
    row = dict(reads=a.reads, length=a.length, listed=int(sum(len(d) for d, _ in args[1])),
               call_s_median=statistics.median(times), call_s_best=min(times), call_s_all=times)
    if not a.device_only:
        import methylation_ref
        want, t_np = timed(lambda: methylation_ref.np_read_methylation(*args), 1)
        row.update(numpy_s=t_np[0], equal=bool(all(np.array_equal(got[k], want[k]) for k in ("counts", "n_c", "status"))))
    print(json.dumps(row), flush=True)

    rng = np.random.default_rng(2)
    s = ALPHABET[rng.integers(0, 4, 4000000)]
    n_c = int((s == ord("C")).sum())
    listed = np.sort(rng.choice(n_c, size=n_c // 4, replace=False))
    mods = [((np.diff(np.concatenate([[-1], listed])) - 1).astype(np.int32), (listed % 256).astype(np.uint8))]
    one = ([s.tobytes().decode()], mods, np.array([2], np.uint8), np.array([1999000], np.int32),
           np.array([2001000], np.int32))
    _capi.read_methylation(*one)
    _, times = timed(lambda: _capi.read_methylation(*one), a.reps)
    longest = dict(reads=1, length=4000000, listed=len(listed), call_s_median=statistics.median(times),
                   call_s_best=min(times))
    print(json.dumps(longest), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(batch=row, longest=longest), f, indent=1)


if __name__ == "__main__":
    main()
