"""Measures the flank haplotype call (nra_flank_phase) on one GPU and writes one JSON file.

The panel: --regions regions, two reference sides of --flank-len random bases each, --reads rows per region on two
haplotypes (six substitutions per side), nine rows in ten with both segments and the rest with one; a segment is the
first flank_len - flank_len // 16 bases of its haplotype's side (every tenth one stops earlier) through the --model error
channel.  Timed, --reps times each and alternating in one process after one warm-up call of each, every repetition
shown: the nra_flank_phase call from packed host buffers to host results, and as a yardstick the nra_allele_split call
(k_split_align: the same band DP, global on both ends) over the same segments, one group per region and side with the
side's first bases as backbone and max_dist chosen so that it starts in the band class the flank call uses.  Rows per
second are tract rows swept (the calls' rows_* counters) over the call time; the calls' other kernels and copies are in
both, the per-kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_flank.py --reps 1` (k_flank_align<C>, k_flank_count, k_split_phase
against k_split_align<C>).

  python tools/gpu_flank.py --out profiles/flank_1000_regions.json [--regions 1000] [--reads 46] [--flank-len 3000]
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

WIDTHS = (64, 128, 256, 512, 1024)


def make_panel(n_regions, n_reads, flank_len, model, seed):
    rng = np.random.default_rng(seed)
    cut = flank_len - flank_len // 16
    offsets = [flank_len * q // 7 + 25 for q in range(6)]
    raw, plan, backbones = [], [], []
    for g in range(n_regions):
        sides = [synth.rand_seq(rng, flank_len) for _ in (0, 1)]
        alts = []
        for s in sides:
            for o in offsets:
                s = s[:o] + "ACGT"[("ACGT".index(s[o]) + 1) % 4] + s[o + 1:]
            alts.append(s)
        backbones.append(tuple(sides))
        for r in range(n_reads):
            src = alts if r % 2 else sides
            for side in (0, 1):
                if r % 10 == 9 and side == r // 10 % 2:
                    plan.append(None)
                    continue
                reach = cut if (r + side) % 10 else int(rng.integers(200, cut))
                plan.append(len(raw))
                raw.append(src[side][:reach])
    seqs = synth.apply_errors_batch(rng, raw, model)
    segs = ["" if q is None else seqs[q] for q in plan]
    groups = [[(segs[2 * (g * n_reads + r)], segs[2 * (g * n_reads + r) + 1]) for r in range(n_reads)]
              for g in range(n_regions)]
    return groups, backbones, cut


def timed(fn, reps_of):
    t0 = time.perf_counter()
    out = fn()
    reps_of.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=46)
    ap.add_argument("--flank-len", type=int, default=3000)
    ap.add_argument("--model", default="hifi")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("no HIP device: this tool measures on a GPU and has no other path")
    groups, backbones, cut = make_panel(a.regions, a.reads, a.flank_len, a.model, a.seed)
    # the yardstick's groups: per region and side the segments that reach the cut, on the side's first `cut` bases
    y_groups = [[row[side] for row in g if len(row[side]) > cut * 9 // 10] for g in groups for side in (0, 1)]
    y_bbs = [bb[side][:cut] for bb in backbones for side in (0, 1)]

    def flank():
        return _capi.flank_phase(groups, backbones)

    def yard(max_dist):
        return _capi.allele_split(y_groups, y_bbs, max_dist=max_dist)

    out = flank()                                               # warm-up: module load, first allocations
    st = out["stats"]
    used = max(w for w in WIDTHS if st[f"aligned_{w}"])
    y_max_dist = min(1000, used - 6)                            # proven(c) >= want picks the class of `used` diagonals
    t_flank, t_yard = [], []
    y_st = None
    if not a.no_yardstick:
        y_st = yard(y_max_dist)["stats"]
    for _ in range(a.reps):
        timed(flank, t_flank)
        if not a.no_yardstick:
            timed(lambda: yard(y_max_dist), t_yard)
    rows = sum(st[f"rows_{w}"] for w in WIDTHS)
    res = dict(regions=a.regions, reads_per_region=a.reads, flank_len=a.flank_len, model=a.model, cut=cut,
               segments=int(sum(bool(s) for g in groups for row in g for s in row)),
               segment_bases=int(sum(len(s) for g in groups for row in g for s in row)),
               flank_call_s=t_flank, flank_stats=st, flank_rows_per_s=[rows / t for t in t_flank],
               phased=int(out["phased"].sum()), sites=int(out["n_sites"].sum()), undecided=int(out["undecided"].sum()),
               left_out=int(out["left_out"].sum()),
               note="call times are the Python wrapper around the C call: packing the strings is in them, for both calls")
    if y_st is not None:
        y_rows = sum(y_st[f"rows_{w}"] for w in WIDTHS)
        res.update(yardstick_max_dist=y_max_dist, yardstick_call_s=t_yard, yardstick_stats=y_st,
                   yardstick_rows_per_s=[y_rows / t for t in t_yard],
                   yardstick_spread=(max(t_yard) - min(t_yard)) / min(t_yard),
                   flank_over_yardstick_rows_per_s=(rows / min(t_flank)) / (y_rows / min(t_yard)))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
