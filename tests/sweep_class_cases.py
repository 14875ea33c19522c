"""Cases shared by test_sweep_classes_cpu.py and test_sweep_classes_gpu.py: for every rows-per-lane class R of NRA_R_LIST
one small batch whose reads all lie in that class, at the class's borders, once without and once with an N, and the
forms of the 1D and 2D sweep kernels each batch runs in.  The planner folds small buckets into the next class, sends
reads of up to 32 * NRA_RING32_MAX_R bases to the half-wave classes and reads above NRA_RING_MT_FROM to row blocks, so a
batch picked by read length alone runs another instantiation than the one it was picked for; a batch of one class has
nothing to fold into, and the flags and NRA_CHAIN_FROM choose the rest.  test_sweep_classes_cpu.py proves from the plans
that every (form, class, N) is reached by exactly one bucket.

Everything is seeded and pure Python; nothing here needs a device."""
import functools

import numpy as np

from nanorepeat_amd import _capi as A, synth
from paths_cases import r_list

RING32_MAX_R = 24            # NRA_RING32_MAX_R: the largest half-wave class
PARK_FROM_R = 28             # nra_sweep.hip: the forward sweep parks the R side of the junction in AGPRs from here on
CHAIN_FROM_ENV = {"NRA_CHAIN_FROM": "3072"}      # its presence switches the fitted row-block model off
KNOBS = ("NRA_RELAX_C", "NRA_CHAIN_FROM", "NRA_TEST_QSTEPS", "NRA_TEST_SAT", "NRA_TEST_SAT_STEPS")
UNIT_1D = "TATTG"
ANCHOR_1D = 400              # beyond the relaxed-cell margin NRA_RELAX_C_DEFAULT = 256: TAINT buckets run relaxed columns
ANCHOR_2D, FLANK_2D = 160, 150                   # NRA_JOINT_PACKED_COLS(160) = 150 >= NRA_JOINT_PACKED_MIN_COLS = 64
UNIT1_2D, MID_2D, UNIT2_2D = "CAG", "CAACAGCCGCCAC", "CCG"


def prev_class(R):
    rs = r_list()
    i = rs.index(R)
    return rs[i - 1] if i else 0


def length_range(R, unit):
    """(first, last) read length of class R in rows of `unit` per row of a lane: 64 full-wave, 32 half-wave."""
    return unit * prev_class(R) + 1, unit * R


def _with_n(s, at):
    return s[:at] + "N" + s[at + 1:]


def _spare(n):
    """Bases a read's source is built longer by before the error channel (which shortens by 1.5 % on average)."""
    return 10 + n // 24


def _errors(rng, src, n, model="ont"):
    """`src` (built _spare(n) bases longer) through the error channel, cut to n bases at its right end."""
    s = synth.apply_errors(rng, src, model)[:n]
    assert len(s) == n, (len(s), n)
    return s


# ------------------------------------------------------------------------------------------------ 1D
def _read_1d(L, Rt, n, left=True, right=True):
    """An error-free read of n bases, the repeat count it holds: up to 100 bases of either flank around
    whole units; what is left over after whole units lengthens a flank."""
    f = min(100, n // 3)
    a, b = (f if left else 0), (f if right else 0)
    k = (n - a - b) // len(UNIT_1D)
    rest = n - a - b - k * len(UNIT_1D)
    if left:
        a += rest
    else:
        b += rest
    s = (L[len(L) - a:] if a else "") + UNIT_1D * k + Rt[:b]
    assert len(s) == n and (left or right)
    return s, k


@functools.lru_cache(maxsize=None)
def batch_1d(R, unit, with_n):
    """The 1D batch of class R (`unit` = 64: full-wave lengths, 32: half-wave lengths): seven reads of one region,

      0  error-free, exactly unit * R bases, its last base a match: the best cell in the last row of the last lane
      1  unit * R bases, ont errors -- sorted by length it shares a wave with read 0
      2  error-free, unit * R - 1 bases
      3  the middle of the class's range, ont errors -- shares a wave with read 2 (and, half-wave, with 0 and 1)
      4  no right flank
      5  no left flank: its tract starts at its first base
      6  unit * R_prev + 1 bases, the first length of the class: most lanes are padding

    in descending length, so that the tasks are (0 1)(2 3)(4 5)(6) full-wave -- the last pair holds one read -- and
    (0 1 2 3)(4 5 6) half-wave -- the last task is short.  Windows of 6 candidates around the count the read was built
    with (5 from R = 28 on, for the oracle's sake).  `with_n`: one N in read 0, in a row of the last lane
    (lane l of a read's 64 or 32 lanes holds rows l R .. l R + R - 1).  Batches of fewer than 100 rows a read run
    with min_dp_score = 20 instead of 80, so that the reads of the first classes give records, not only NO_RECORD."""
    assert unit in (32, 64) and R in r_list()
    rng = np.random.default_rng([20261020, R, unit])
    L, Rt = synth.rand_seq(rng, ANCHOR_1D), synth.rand_seq(rng, ANCHOR_1D)
    lo, hi = length_range(R, unit)
    mid = (lo + hi) // 2
    reads, ks = [], []
    for n, kind in ((hi, "exact"), (hi, "ont"), (hi - 1, "exact"), (mid, "ont"), (lo + (hi - lo) // 3, "no_right"),
                    (lo + (hi - lo) // 4, "no_left"), (lo, "exact")):
        if kind == "ont":
            s, k = _read_1d(L, Rt, n + _spare(n))
            s = _errors(rng, s, n)
        else:
            s, k = _read_1d(L, Rt, n, left=kind != "no_left", right=kind != "no_right")
        reads.append(s); ks.append(k)
    assert [len(r) for r in reads] == sorted((len(r) for r in reads), reverse=True) and len(reads[0]) == hi
    assert all(lo <= len(r) <= hi for r in reads), (R, unit)
    if with_n:
        at = hi - 1 - R // 2
        assert at >= hi - R                            # a row of the last lane
        reads[0] = _with_n(reads[0], at)
    half = 3 if R < PARK_FROM_R else 2
    ks = np.array(ks, np.int32)
    return dict(regions=[(L, UNIT_1D, Rt)], reads=reads, kmin=np.maximum(ks - 2, 0).astype(np.int32),
                kmax=(ks + half).astype(np.int32), k_true=ks, sc=dict(min_dp_score=20) if hi < 100 else {},
                R=R, unit=unit, with_n=with_n)


def forms_1d():
    """The forms of the 1D sweeps: name -> flags, the row unit of the batches it takes (32: the half-wave classes up to
    NRA_RING32_MAX_R, 64: all 24), what its one bucket and the plan's `brute` must say, whether it is a ring form (run twice,
    NRA_CHAIN_FROM from class 28 on) and which extents it fills."""
    ring = dict(ring=1, quanta=1, taint=1)

    def form(flags, unit, brute=0, extents=None, **bucket):
        b = dict(dict(half=int(unit == 32), ring=0, quanta=0, taint=0, chain=0, mt=0), **bucket)
        return dict(flags=flags, unit=unit, brute=brute, extents=extents, bucket=b, ring_form=bool(b["ring"]))

    H = A.F_NO_HALF_WAVE
    return {
        "half_quanta": form(0, 32, **ring),                                               # k_sweep_ringq<HALF>
        "half_two_launches": form(A.F_NO_QUANTA, 32, **dict(ring, quanta=0)),             # k_sweep_ring32
        "half_tie_extents": form(A.F_TIE_EXTENTS, 32, extents="ties", **ring),            # ... + k_payload<ORIGIN>
        "full_quanta": form(H, 64, **ring),                                               # k_sweep_ringq
        "full_two_launches": form(H | A.F_NO_QUANTA, 64, **dict(ring, quanta=0)),         # k_sweep_ring
        "full_exact_anchors": form(H | A.F_FULL_ANCHORS, 64, **dict(ring, taint=0)),      # TAINT off
        "full_two_launches_exact_anchors": form(H | A.F_NO_QUANTA | A.F_FULL_ANCHORS, 64, **dict(ring, quanta=0, taint=0)),
        "full_tie_extents": form(H | A.F_TIE_EXTENTS, 64, extents="ties", **ring),
        "dpp": form(A.F_DPP_SWEEP, 64),                                                   # k_sweep_pk16
        "brute": form(A.F_BRUTE_FORCE, 64, brute=1),                                      # k_score_pk16
        "all_extents": form(A.F_ALL_EXTENTS, 64, brute=1, extents="all"),                 # k_payload<ORIGIN> per candidate
    }


def classes_of(form):
    """The classes a 1D form is built for: all of NRA_R_LIST, but for the half-wave forms, which end at
    NRA_RING32_MAX_R (longer reads have no half-wave kernel)."""
    return [R for R in r_list() if form["unit"] == 64 or R <= RING32_MAX_R]


def env_of(form, R):
    """NRA_CHAIN_FROM = 3072 for the ring forms from class 28 on: without it reads above NRA_RING_MT_FROM run as row blocks."""
    return dict(CHAIN_FROM_ENV) if form["ring_form"] and R >= PARK_FROM_R else {}


def parse_plan1d(text):
    """-> (scalars, buckets) of a plan1d digest."""
    scalars, buckets = {}, []
    for line in text.splitlines():
        key, _, value = line.partition(" ")
        if key.startswith("bucket"):
            b = dict(kv.split("=") for kv in value.split())
            buckets.append({k: v if k == "mt_groups" else int(v) for k, v in b.items()})
        else:
            scalars[key] = value
    assert int(scalars["n_buckets"]) == len(buckets)
    return scalars, buckets


def plan_1d(d, flags, simds=1024):
    """The plan of a batch under `flags` (the caller has set the environment)."""
    return parse_plan1d(A.plan1d_digest(d["regions"], d["reads"], d["kmin"], d["kmax"], sc=A.default_scoring(**d["sc"]),
                                        flags=flags, simds=simds))


def agpr_test_inputs():
    """The inputs of test_gpu_parity.test_large_row_counts_park_the_junction_in_agprs."""
    rng = np.random.default_rng(91)
    L, R = synth.rand_seq(rng, 400), synth.rand_seq(rng, 400)
    reads, kmin, kmax = [], [], []
    for k_true in (300, 310, 350, 360, 440, 450, 520, 530, 560):          # cores of 1.7 ... 3.0 kb
        s = synth.apply_errors(rng, L[-100:] + "TATTG" * k_true + R[:100], "hifi")
        if k_true == 440:
            s = s[:700] + "NN" + s[702:]
        reads.append(s[:3072]); kmin.append(k_true - 6); kmax.append(k_true + 6)
    return dict(regions=[(L, "TATTG", R)], reads=reads, kmin=kmin, kmax=kmax, sc={})


# ------------------------------------------------------------------------------------------------ 2D
def _read_2d(region, n):
    """An error-free plus-strand read of n bases over the joint region and its (k1, k2): a quarter of the read on
    either flank, at least 74 and at most FLANK_2D bases -- fewer than 74 only where the read cannot hold them around two
    units of each motif and the mid."""
    left, u1, mid, u2, right = region
    least = 2 * len(u1) + len(mid) + 2 * len(u2)
    if n < least + 2:
        return (left[-1:] + u1 * 2 + mid + u2 * 2 + right)[:n], (2, 2)
    f = min((n - least) // 2, max(74, min(FLANK_2D, n // 4)))
    core = n - 2 * f - len(mid)
    k1 = core // 2 // len(u1)
    k2 = (core - k1 * len(u1)) // len(u2)
    rest = core - k1 * len(u1) - k2 * len(u2)
    assert 0 <= rest < len(u2) and f + rest <= len(left)
    s = left[len(left) - f - rest:] + u1 * k1 + mid + u2 * k2 + right[:f]
    assert len(s) == n
    return s, (k1, k2)


@functools.lru_cache(maxsize=None)
def batch_2d(R, with_n):
    """The 2D batch of class R: seven reads of both strands over one joint region (CAG, a 13-base mid, CCG, anchors of
    160 bases: packed flank sweeps apply), at the lengths of batch_1d, in this order (pairs are made in read order:
    (0 1)(2 3)(4 5)(6)):

      0  +  error-free, exactly 64 R bases        1  -  64 R bases, ont errors
      2  -  error-free, 64 R - 1 bases            3  +  the middle of the range, ont errors
      4  -  the middle of the range, hifi errors  5  +  error-free, 64 R_prev + 1 bases
      6  -  error-free, 64 R_prev + 1 bases

    `with_n`: one N in read 0 in a row of the last lane.  Classes whose reads are shorter than 100 bases run with
    min_dp_score = 20.  The cells of a read are the 3 x 3 grid around the counts it was built with (floored at 0)."""
    assert R in r_list()
    rng = np.random.default_rng([20261021, R])
    region = (synth.rand_seq(rng, ANCHOR_2D), UNIT1_2D, MID_2D, UNIT2_2D, synth.rand_seq(rng, ANCHOR_2D))
    lo, hi = length_range(R, 64)
    mid = (lo + hi) // 2
    reads, strands, truth = [], [], []
    for n, model, st in ((hi, None, 1), (hi, "ont", -1), (hi - 1, None, -1), (mid, "ont", 1), (mid, "hifi", -1),
                         (lo, None, 1), (lo, None, -1)):
        if model:
            s, t = _read_2d(region, n + _spare(n))
            s = _errors(rng, s, n, model)
        else:
            s, t = _read_2d(region, n)
        assert len(s) == n
        reads.append(s if st > 0 else synth.revcomp(s)); strands.append(st); truth.append(t)
    assert all(lo <= len(r) <= hi for r in reads)
    if with_n:
        at = hi - 1 - R // 2
        assert at >= hi - R
        reads[0] = _with_n(reads[0], at)
    truth = np.array(truth, np.int32)
    k1max, k2max = int(truth[:, 0].max()) + 4, int(truth[:, 1].max()) + 4
    assert 6 * (len(UNIT1_2D) * k1max + len(MID_2D) + len(UNIT2_2D) * k2max + 20) < 32768
    return dict(region=region, reads=reads, strand=np.array(strands, np.int8), truth=truth,
                sc=dict(min_dp_score=20) if hi < 100 else {}, R=R, with_n=with_n)


def grids_2d(j):
    """(cells grid, coarse grid, refinement bounds and steps) of a 2D batch.  The cells grid has step 1 and per read the
    bounds [t - 1, t + 2): its cell list (nra_joint_grid_cells) is the 3 x 3 grid around the read's counts, which
    set_cells and set_grid then both run.  The coarse grid has step 2 over [t - 3, t + 4); the refinement behind it
    (buffers 1, 1) scores the 2 x 2 cells around the coarse size."""
    t1, t2 = j["truth"][:, 0].astype(np.float64), j["truth"][:, 1].astype(np.float64)
    c1, c2 = int(t1.max()) + 6, int(t2.max()) + 6
    cells = A.Grid((0, 1, c1), np.maximum(t1 - 1, 0), t1 + 2, (0, 1, c2), np.maximum(t2 - 1, 0), t2 + 2)
    bounds = (np.maximum(t1 - 3, 0), t1 + 4, np.maximum(t2 - 3, 0), t2 + 4)
    coarse = A.Grid((0, 2, c1 // 2 + 1), bounds[0], bounds[1], (0, 2, c2 // 2 + 1), bounds[2], bounds[3])
    return cells, coarse, bounds, (1, 1)


def forms_2d():
    """The forms of the 2D sweeps: name -> batch flags, `grid` (set_grid) or cells (set_cells), strands given or left
    to the probe, whether the packed flank sweeps are meant to run, and whether a refinement follows."""
    def form(flags=0, grid=False, given=True, packed=True, refine=False):
        return dict(flags=flags, grid=grid, given=given, packed=packed, refine=refine)

    return {
        "cells": form(),
        "cells_strands_probed": form(given=False),
        "cells_no_joint_pack": form(A.F_NO_JOINT_PACK, packed=False),
        "grid_chained_mid": form(grid=True),
        "grid_mid_per_k1": form(A.F_JOINT_NO_CHAIN, grid=True),
        "grid_tails": form(A.F_JOINT_TAILS, grid=True),
        "grid_refined": form(grid=True, refine=True),
    }


def steps_2d(j, form):
    """The plan2d_digest steps of a form on a batch."""
    cells, coarse, bounds, buf = grids_2d(j)
    st = j["strand"] if form["given"] else None
    if form["refine"]:
        return [dict(kind="grid", grid=coarse, strand=st), dict(kind="refine", bounds=bounds, buf=buf)]
    if form["grid"]:
        return [dict(kind="grid", grid=cells, strand=st)]
    return [dict(kind="cells", cells=A.joint_grid_cells(cells), strand=st)]


def parse_plan2d(text):
    """-> [per step: dict of its lines; `buckets`: list of dicts]"""
    steps = []
    for block in text.split("\nstep ")[1:]:
        first, *lines = block.splitlines()
        d = {"buckets": []}
        for line in lines:
            key, _, value = line.partition(" ")
            if key.startswith("bucket") and key[6:].isdigit():
                d["buckets"].append({k: int(v) for k, v in (kv.split("=") for kv in value.split())})
            else:
                d[key] = value
        steps.append(d)
    return steps


def plan_2d(j, form):
    return parse_plan2d(A.plan2d_digest(j["region"], j["reads"], steps_2d(j, form), sc=A.default_scoring(**j["sc"]),
                                        flags=form["flags"]))
