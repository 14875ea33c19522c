"""Inputs of the 1D plan test (tests/test_plan1d_cpu.py): name -> the arguments of nanorepeat_amd._capi.plan1d_digest and
the environment knobs of the case.  Everything is seeded; the plan reads lengths, regions and windows only, so the reads are
plain random sequences of the wanted lengths."""
import functools

import numpy as np

from nanorepeat_amd import _capi as A, synth


def region(rng, unit="TATTG", left=100, right=100):
    return synth.rand_seq(rng, left), unit, synth.rand_seq(rng, right)


def case(regions, lens, kwin, read_region=None, seed=0, **kw):
    """`lens`: read lengths; `kwin`: one (kmin, kmax) for all reads, or one per read."""
    rng = np.random.default_rng(9000 + seed)
    reads = [synth.rand_seq(rng, int(n)) for n in lens]
    win = np.array([kwin] * len(reads) if np.ndim(kwin) == 1 else kwin, np.int32).reshape(len(reads), 2)
    return dict(regions=regions, reads=reads, kmin=win[:, 0].copy(), kmax=win[:, 1].copy(), read_region=read_region,
                flags=0, simds=1024, sc={}, env={}, **kw)


def with_(c, **over):
    d = dict(c)
    d.update(over)
    return d


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261)
    two = [region(rng, "TATTG"), region(rng, "CAG")]
    one = [region(rng, "TATTG")]
    out = {}

    # 1, 2: 40 short reads over two regions
    short_lens = rng.integers(100, 701, size=40)
    short_rr = rng.integers(0, 2, size=40).astype(np.int32)
    short = case(two, short_lens, (5, 60), read_region=short_rr, seed=1)
    out["short"] = short
    out["short_no_half_wave"] = with_(short, flags=A.F_NO_HALF_WAVE)

    # 3: the fitted model, both outcomes
    mid = case(one, rng.integers(1600, 3001, size=600), (5, 200), seed=3)
    out["mid_simds1024"] = mid
    out["mid_simds16"] = with_(mid, simds=16)

    # 4: stragglers next to row blocks (as the issue words it: every read above NRA_RING_MT_FROM = 1536), and the same
    # with the short reads at or below that line, where the rule is what moves them
    out["stragglers_1550"] = case(one, [2000] * 300 + list(rng.integers(1550, 1601, size=30)), (5, 200), seed=4)
    out["stragglers_1500"] = case(one, [2000] * 300 + list(rng.integers(1480, 1537, size=30)), (5, 200), seed=4)

    # 5, 7: a packed chain of row blocks
    long_ = case(one, [4000] * 6 + [6000] * 5, (5, 200), seed=5)
    out["long"] = long_
    out["long_serial_chain"] = with_(long_, flags=A.F_SERIAL_CHAIN)
    out["long_dpp_sweep"] = with_(long_, flags=A.F_DPP_SWEEP)
    out["short_test_chain"] = with_(short, flags=A.F_TEST_CHAIN)

    # 6: the int32 chain bucket, by score and by template length (NRA_MAX_TLEN = 65000)
    out["wide_by_score"] = case(one, [7000], (5, 200), seed=6)
    out["wide_by_template"] = case(one, [500, 600], [(13090, 13100), (5, 60)], seed=6)

    # 8: every flag that changes the plan of the short reads
    for name, flag in (("brute_force", A.F_BRUTE_FORCE), ("all_extents", A.F_ALL_EXTENTS), ("tie_extents", A.F_TIE_EXTENTS),
                       ("no_quanta", A.F_NO_QUANTA), ("full_anchors", A.F_FULL_ANCHORS)):
        out["short_" + name] = with_(short, flags=flag)

    # 9: a unit above NRA_SWEEP_RING_MAX_M = 8
    out["unit9"] = case([region(rng, "TATTGACCG")], short_lens, (5, 60), seed=9)
    # 10: no left flank
    out["no_left_flank"] = case([region(rng, "TATTG", left=0)], short_lens, (5, 60), seed=10)
    # 11: scorings the sweeps, or the taint scheme alone, do not hold
    out["scoring_brute"] = with_(short, sc=dict(mismatch=8))
    out["scoring_no_taint"] = with_(short, sc=dict(gap_open1=30, gap_open2=40))

    # 12: reads without a window, and an empty read with one
    win = np.array([(5, 60)] * 40, np.int32)
    win[[3, 17, 30]] = (7, 6)
    lens = short_lens.copy()
    lens[11] = 0
    out["skipped_and_empty"] = case(two, lens, win, read_region=short_rr, seed=12)

    # 13: quanta on a device of 4 SIMDs
    out["quanta_parts"] = with_(short, simds=4)
    many = case(two, rng.integers(100, 701, size=200), (5, 60), read_region=rng.integers(0, 2, size=200).astype(np.int32), seed=13)
    out["quanta_too_many"] = with_(many, simds=4)
    out["quanta_qsteps64"] = with_(short, simds=4, env={"NRA_TEST_QSTEPS": "64"})

    # 14: the errors
    bad = np.array([(5, 60)] * 40, np.int32)
    bad[5] = (-1, 60)
    out["error_kmin_negative"] = case(two, short_lens, bad, read_region=short_rr, seed=1)
    out["error_template_too_long"] = case(one, [500], (800000, 800001), seed=14)
    out["error_brute_long_read"] = with_(case(one, [500, 3100], (5, 60), seed=14), flags=A.F_BRUTE_FORCE)
    out["error_test_chain_brute"] = with_(short, flags=A.F_TEST_CHAIN | A.F_BRUTE_FORCE)
    return out


KNOBS = ("NRA_RELAX_C", "NRA_CHAIN_FROM", "NRA_TEST_QSTEPS", "NRA_TEST_SAT", "NRA_TEST_SAT_STEPS")


def digest(c):
    """The digest text of a case, or ("error", code, text).  The caller has set the case's environment."""
    try:
        return A.plan1d_digest(c["regions"], c["reads"], c["kmin"], c["kmax"], read_region=c["read_region"],
                               sc=A.default_scoring(**c["sc"]), flags=c["flags"], simds=c["simds"])
    except A.NraError as e:
        return ["error", e.code, str(e).split(": ", 1)[1]]
