"""The error contract of the tract-feature entry points: every bad-argument case the test_*_cpu.py files run, the
checks of the tract offsets and arrays that the entry points share, and one good-argument call per entry point give
the return code and the nra_last_error text recorded in golden/capi_errors.json.  The bad-argument cases fail before
the device is touched, so they run with and without a GPU; the good-argument cases ("no HIP device") are skipped where
a GPU is present."""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_errors.json")
TWO = ["ATTTT", "ATTTC"]


def _mix(**change):
    good = dict(samples=np.arange(24, dtype=np.float64), prob_off=[0, 4], prob_n=[12, 10], prob_d=[2, 1],
                fit_problem=[0, 1], fit_n=[2, 3], starts=[0, 5, 1, 2, 9])
    return {**good, **change}


def cases(capi):
    """[(entry point, case, call)]: a call returns a code or a result, or raises NraError.  The case "good" has good
    arguments."""
    lib = capi.load()
    i64 = lambda a: capi._ptr(a, C.c_int64)
    data, off = capi.pack_reads(["CAG"])
    data2, off2 = capi.pack_reads(["ACGT", "ACGT"])
    out = []

    def add(entry, case, call):
        out.append((entry, case, call))

    anchors = [("ACGTACGTTGCATGCAAGT", "TTGACCATGACCAGTACAG")]
    h = C.c_void_p()
    for kw in (dict(k=14), dict(k=9), dict(k=17), dict(max_occ=0), dict(max_occ=256)):
        add("nra_screen_create", repr(kw), lambda kw=kw: capi.screen_create(anchors, **kw))
    add("nra_screen_create", "anchor_off NULL", lambda: lib.nra_screen_create(0, 1, data2, None, 15, 16, C.byref(h)))
    add("nra_screen_create", "no regions", lambda: lib.nra_screen_create(0, 0, data2, i64(off2), 15, 16, C.byref(h)))
    add("nra_screen_create", "out NULL", lambda: lib.nra_screen_create(0, 1, data2, i64(off2), 15, 16, None))
    bad_off = np.array([0, 4, 2], np.int64)
    add("nra_screen_create", "offsets decrease",
        lambda: lib.nra_screen_create(0, 1, data2, i64(bad_off), 15, 16, C.byref(h)))
    add("nra_screen_create", "good", lambda: capi.screen_create(anchors))
    n = C.c_int64(0)
    add("nra_screen_reads", "handle NULL",
        lambda: lib.nra_screen_reads(None, 1, data2, i64(off2), 4, C.byref(n), None, None, None, None))
    add("nra_screen_stats", "handle NULL", lambda: lib.nra_screen_stats(None, C.byref(capi.ScreenStats())))

    for name, call, none_out in (("nra_read_structure", capi.read_structure, (None,) * 3),
                                 ("nra_extend_tracts", capi.extend_tracts, (2, 4, 6) + (None,) * 4)):
        fn = getattr(lib, name)
        for motif in ("", "A" * 65, "CAN", "cag"):
            add(name, "motif " + repr(motif if len(motif) < 9 else "A*65"),
                lambda call=call, motif=motif: call([motif], ["CAGCAG"], [0]))
        add(name, "read_motif out of range", lambda call=call: call(["CAG"], ["CAG"], [1]))
        add(name, "tract too long", lambda call=call: call(["CAG"], ["A" * 200001], [0]))
        add(name, "no motifs", lambda fn=fn, o=none_out: fn(0, 0, data, i64(off), 0, None, None, None, *o))
        add(name, "motif_off NULL", lambda fn=fn, o=none_out: fn(0, 1, data, None, 0, None, None, None, *o))
    for kw in (dict(match=0), dict(match=128), dict(mismatch=-1), dict(mismatch=128), dict(gap=0), dict(gap=128)):
        add("nra_extend_tracts", repr(kw), lambda kw=kw: capi.extend_tracts(["CAG"], ["CAGCAG"], [0], **kw))
    add("nra_read_structure", "good", lambda: capi.read_structure(["CAG", "A" * 64], ["CAGCAG", ""], [0, 1]))
    add("nra_extend_tracts", "good",
        lambda: capi.extend_tracts(["CAG", "A" * 64], ["CAGCAG", ""], [0, 1], mismatch=0, gap=127))

    for kw in (dict(max_period=0), dict(max_period=7), dict(top_n=0), dict(top_n=9)):
        add("nra_tract_motifs", repr(kw), lambda kw=kw: capi.tract_motifs(["CAGCAG"], **kw))
    add("nra_tract_motifs", "tract too long", lambda: capi.tract_motifs(["CAG", "A" * 200001]))
    add("nra_tract_motifs", "negative count",
        lambda: lib.nra_tract_motifs(0, -1, data, i64(off), 6, 4, None, None, None, None))
    add("nra_tract_motifs", "every array NULL",
        lambda: lib.nra_tract_motifs(0, 1, data, None, 6, 4, None, None, None, None))
    add("nra_tract_motifs", "good", lambda: capi.tract_motifs(["CAGCAG", "", "A" * 200000]))

    for q, change in enumerate((dict(prob_d=[3, 1]), dict(prob_d=[2, 0]), dict(fit_n=[0, 3], starts=[1, 2, 9]),
                                dict(fit_n=[2, 11], starts=[0, 5] + list(range(10)) + [0]),
                                dict(starts=[0, 12, 1, 2, 9]), dict(starts=[0, 5, 1, 2, 10]),
                                dict(starts=[0, -1, 1, 2, 9]), dict(fit_problem=[0, 2]), dict(prob_off=[0, 15]),
                                dict(samples=np.where(np.arange(24) == 7, np.nan, np.arange(24.0))),
                                dict(samples=np.where(np.arange(24) == 23, np.inf, np.arange(24.0))), dict(flags=4))):
        add("nra_mixture_fit", f"change {q}: {sorted(change)}", lambda change=change: capi.mixture_fit(**_mix(**change)))
    add("nra_mixture_fit", "33 components",
        lambda: capi.mixture_fit(np.zeros(40), [0], [40], [1], [0], [33], list(range(33))))
    one = np.zeros(1)
    po, pn, pd = np.zeros(1, np.int64), np.array([(1 << 22) + 1], np.int32), np.ones(1, np.int32)
    add("nra_mixture_fit", "too many points",
        lambda: lib.nra_mixture_fit(0, 1 << 23, capi._ptr(one, C.c_double), 1, i64(po), capi._ptr(pn, C.c_int32),
                                    capi._ptr(pd, C.c_int32), 0, *(None,) * 3, 0, *(None,) * 6))
    add("nra_mixture_fit", "negative count",
        lambda: lib.nra_mixture_fit(0, -1, None, 0, None, None, None, 0, *(None,) * 3, 0, *(None,) * 6))
    add("nra_mixture_fit", "good", lambda: capi.mixture_fit(**_mix()))

    for kw in (dict(max_dist=-1), dict(max_dist=1001), dict(max_rounds=0), dict(max_rounds=65)):
        add("nra_tract_consensus", repr(kw), lambda kw=kw: capi.tract_consensus([["CAGCAG"]], **kw))
    add("nra_tract_consensus", "tract too long", lambda: capi.tract_consensus([["A" * 200001]]))
    goff = np.array([0, 2], np.int64)
    res, coff = np.zeros(4, np.int32), np.zeros(2, np.int64)
    args = (1, data, i64(off), 100, 8, 0, None, None, i64(coff), capi._ptr(res, C.c_int32), None)
    add("nra_tract_consensus", "groups beyond the tracts", lambda: lib.nra_tract_consensus(0, 1, i64(goff), *args))
    add("nra_tract_consensus", "group_off NULL", lambda: lib.nra_tract_consensus(0, 1, None, *args))
    add("nra_tract_consensus", "good", lambda: capi.tract_consensus([["CAGCAG", "CAGCAA"], []]))

    for kw in (dict(max_dist=-1), dict(max_dist=1001), dict(min_count=0), dict(min_sites=0), dict(min_share_pct=0),
               dict(min_share_pct=101), dict(min_purity_pct=101), dict(max_sites=0), dict(max_sites=4097),
               dict(max_iter=0), dict(max_iter=65)):
        add("nra_allele_split", repr(kw), lambda kw=kw: capi.allele_split([["CAGCAG"]], ["CAGCAG"], **kw))
    add("nra_allele_split", "tract too long", lambda: capi.allele_split([["A" * 200001]], ["ACGT"]))
    add("nra_allele_split", "backbone too long", lambda: capi.allele_split([["ACGT"]], ["A" * 200001]))
    add("nra_allele_split", "backbone with N", lambda: capi.allele_split([["ACGT"]], ["ACNT"]))
    add("nra_allele_split", "good", lambda: capi.allele_split([["CAGCAG", "CAGCAA"], []], ["CAGCAG", ""]))

    for q, (sets, tracts, W) in enumerate((([TWO], ["ATTTT"], 0), ([TWO], ["ATTTT"], -3), ([[]], ["ATTTT"], 3),
                                           ([["ATTTT", ""]], ["ATTTT"], 3), ([["ATTNT"]], ["ATTTT"], 3),
                                           ([["attt"]], ["ATTTT"], 3), ([["A"] * 9], ["ATTTT"], 3),
                                           ([["ACGT" * 8, "A"]], ["ATTTT"], 3), ([["A" * 33]], ["ATTTT"], 3),
                                           ([TWO], ["A" * 200001], 3), ([TWO], ["ATTTT"], 1001))):
        add("nra_tract_segments", f"bad {q}",
            lambda sets=sets, tracts=tracts, W=W: capi.tract_segments(sets, tracts, [0] * len(tracts), W))
    add("nra_tract_segments", "tract_set out of range", lambda: capi.tract_segments([TWO], ["ATTTT"], [1], 3))
    add("nra_tract_segments", "good", lambda: capi.tract_segments([TWO], ["ATTTTATTTC", ""], [0, 0], 3))

    # the tract offsets and arrays of one tract, the same for the six calls that take tracts
    i32 = lambda a: capi._ptr(a, C.c_int32)
    u8 = lambda a: capi._ptr(a, C.c_uint8)
    mdata, moff = capi.pack_reads(["CAG"])
    zero, bytes4 = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    z64, soff, goff1 = np.zeros(4, np.int64), np.array([0, 1], np.int32), np.array([0, 1], np.int64)
    takers = {
        "nra_read_structure": lambda s, o, a, b: lib.nra_read_structure(
            0, 1, mdata, i64(moff), 1, s, o, a and i32(zero), i32(zero), i32(zero), b and u8(bytes4)),
        "nra_extend_tracts": lambda s, o, a, b: lib.nra_extend_tracts(
            0, 1, mdata, i64(moff), 1, s, o, i32(zero), 2, 4, 6, a and i32(zero), i32(zero), i32(zero), i32(zero)),
        "nra_tract_segments": lambda s, o, a, b: lib.nra_tract_segments(
            0, 1, i32(soff), mdata, i64(moff), 1, s, o, i32(zero), 3, a and i32(zero), i32(zero), i32(zero),
            u8(bytes4), b and u8(bytes4)),
        "nra_tract_motifs": lambda s, o, a, b: lib.nra_tract_motifs(
            0, 1, s, o, 6, 4, a and i32(np.zeros(8, np.int32)), capi._ptr(np.zeros(4, np.int8), C.c_int8),
            i32(zero), i32(zero)),
        "nra_tract_consensus": lambda s, o, a, b: lib.nra_tract_consensus(
            0, 1, i64(goff1), 1, s, o, 100, 8, 0, None, None, i64(z64), i32(zero), None),
        "nra_allele_split": lambda s, o, a, b: lib.nra_allele_split(
            0, 1, i64(goff1), 1, s, o, mdata, i64(moff), 100, 3, 25, 75, 1, 256, 16, i32(zero), i32(zero),
            i32(np.zeros(8, np.int32)), 0, None, i64(z64), 0, None, i64(z64), None),
    }
    negative, decreasing = np.array([-1, 2], np.int64), np.array([3, 1], np.int64)
    for name, call in takers.items():
        add(name, "negative tract offset", lambda call=call: call(data, i64(negative), True, True))
        add(name, "tract offsets decrease", lambda call=call: call(data, i64(decreasing), True, True))
        add(name, "seq_off NULL", lambda call=call: call(data, None, True, True))
        add(name, "seqs NULL", lambda call=call: call(None, i64(off), True, True))
    for name in ("nra_read_structure", "nra_extend_tracts", "nra_tract_segments", "nra_tract_motifs"):
        add(name, "first output NULL", lambda call=takers[name]: call(data, i64(off), None, True))
    for name in ("nra_read_structure", "nra_tract_segments"):
        add(name, "last output NULL", lambda call=takers[name]: call(data, i64(off), True, None))
    return out


def outcome(capi, call):
    """(return code, nra_last_error text) of a call; the text of a call that succeeds is ""."""
    try:
        rc = call()
    except capi.NraError as e:
        rc = e.code
    rc = rc if isinstance(rc, int) else 0
    return rc, (capi.load().nra_last_error().decode(errors="replace") if rc != 0 else "")


@pytest.fixture(scope="module")
def golden():
    return {(g["entry"], g["case"]): (g["code"], g["text"]) for g in json.load(open(GOLDEN))}


def test_every_recorded_case_is_replayed(capi, golden):
    have = [(entry, case) for entry, case, _ in cases(capi)]
    assert len(set(have)) == len(have) and set(have) == set(golden)
    assert {entry for entry, case in have if case == "good"} == {
        "nra_screen_create", "nra_read_structure", "nra_tract_motifs", "nra_extend_tracts", "nra_mixture_fit",
        "nra_tract_consensus", "nra_allele_split", "nra_tract_segments"}


def test_bad_arguments_give_the_recorded_code_and_text(capi, golden):
    for entry, case, call in cases(capi):
        if case != "good":
            assert outcome(capi, call) == golden[(entry, case)], (entry, case)
            assert golden[(entry, case)][0] in (-1, -3), (entry, case)


def test_good_arguments_without_a_device_give_the_recorded_code_and_text(capi, golden):
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for entry, case, call in cases(capi):
        if case == "good":
            assert outcome(capi, call) == golden[(entry, case)], (entry, case)
            assert golden[(entry, case)][0] == -2 and "no HIP device" in golden[(entry, case)][1], entry
