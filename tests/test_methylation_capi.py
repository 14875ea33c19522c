"""The error contract of nra_read_methylation, in the manner of test_periods_capi.py: every bad argument gives its code
and its nra_last_error text before the device is touched, so these run with and without a GPU; good arguments without a
device fail loudly (skipped where a GPU is present: the GPU suite covers the call there)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_RANGE = -1, -2, -3
TRACT = "a tract outside 0 <= lo <= hi <= n"
BYTES = "call bytes must satisfy 0 <= lo_byte < hi_byte <= 255"


def _bad_calls(capi):
    """[(case, call, code, text)]"""
    lib = capi.load()
    i64, i32, u8 = (lambda a: capi._ptr(a, C.c_int64)), (lambda a: capi._ptr(a, C.c_int32)), (lambda a: capi._ptr(a, C.c_uint8))
    data, off = capi.pack_reads(["ACGCGT"])
    deltas, probs, mod_off = np.array([0, 1], np.int32), np.array([9, 200], np.uint8), np.array([0, 2], np.int64)
    flags, lo, hi = np.zeros(1, np.uint8), np.array([2], np.int32), np.array([4], np.int32)
    counts, n_c, status = np.zeros(21 * 5, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    good = dict(n=1, data=data, off=i64(off), deltas=i32(deltas), probs=u8(probs), mod_off=i64(mod_off), flags=u8(flags),
                lo=i32(lo), hi=i32(hi), flank=2000, bin=200, lo_byte=63, hi_byte=192, counts=i32(counts), n_c=i32(n_c),
                status=i32(status))
    keep = []

    def raw(**over):
        a = {**good, **{k: v for k, v in over.items()}}
        return lambda: lib.nra_read_methylation(0, a["n"], a["data"], a["off"], a["deltas"], a["probs"], a["mod_off"],
                                                a["flags"], a["lo"], a["hi"], a["flank"], a["bin"], a["lo_byte"],
                                                a["hi_byte"], a["counts"], a["n_c"], a["status"])

    def arr(values, dtype, ptr):
        keep.append(np.array(values, dtype))
        return ptr(keep[-1])

    one = (["ACGCGT"], [(deltas, probs)], flags, lo, hi)
    cases = [
        ("flank 0", raw(flank=0), E_ARG, "flank must be at least 1"),
        ("flank -1", raw(flank=-1), E_ARG, "flank must be at least 1"),
        ("flank 100001", raw(flank=100001, bin=100001), E_RANGE, "flank is longer than 100000 bases"),
        ("bin 0", raw(bin=0), E_ARG, "bin must be in 1..flank"),
        ("bin over flank", raw(flank=100, bin=101), E_ARG, "bin must be in 1..flank"),
        ("65 bins", raw(flank=6401, bin=100), E_RANGE, "more than 64 bins per flank"),
        ("lo_byte -1", raw(lo_byte=-1), E_ARG, BYTES),
        ("hi_byte 256", raw(hi_byte=256), E_ARG, BYTES),
        ("lo_byte = hi_byte", raw(lo_byte=100, hi_byte=100), E_ARG, BYTES),
        ("negative count", raw(n=-1), E_ARG, "negative read count"),
        ("read too long", lambda: capi.read_methylation(["ACG", "A" * 4000001], [one[1][0]] * 2, np.zeros(2, np.uint8),
                                                        np.zeros(2, np.int32), np.zeros(2, np.int32)),
         E_RANGE, "read 1 is longer than 4000000 bases"),
        ("seqs NULL", raw(data=None), E_ARG, "seqs is NULL"),
        ("deltas NULL", raw(deltas=None), E_ARG, "NULL modification array"),
        ("probs NULL", raw(probs=None), E_ARG, "NULL modification array"),
        ("negative read offset", raw(off=arr([-1, 5], np.int64, i64)), E_ARG, "negative read offset"),
        ("read offsets decrease", raw(off=arr([6, 0], np.int64, i64)), E_ARG, "read offsets must not decrease"),
        ("negative modification offset", raw(mod_off=arr([-1, 1], np.int64, i64)), E_ARG, "negative modification offset"),
        ("modification offsets decrease", raw(mod_off=arr([2, 0], np.int64, i64)), E_ARG,
         "modification offsets must not decrease"),
        ("flag bit 2", raw(flags=arr([4], np.uint8, u8)), E_ARG, "read 0 has a flag bit other than 0 and 1"),
        ("tract lo < 0", raw(lo=arr([-1], np.int32, i32)), E_ARG, "read 0 has " + TRACT),
        ("tract lo > hi", raw(lo=arr([5], np.int32, i32)), E_ARG, "read 0 has " + TRACT),
        ("tract hi > n", raw(hi=arr([7], np.int32, i32)), E_ARG, "read 0 has " + TRACT),
        ("negative delta", raw(deltas=arr([0, -1], np.int32, i32)), E_ARG, "negative delta"),
    ]
    for name in ("off", "mod_off", "flags", "lo", "hi", "counts", "n_c", "status"):
        cases.append((f"{name} NULL", raw(**{name: None}), E_ARG, "NULL read array"))
    # the binding passes what it is given on: the library refuses it, not the binding
    cases.append(("binding: bin over flank", lambda: capi.read_methylation(*one, flank=10, bin=11), E_ARG,
                  "bin must be in 1..flank"))
    cases.append(("binding: 65 bins", lambda: capi.read_methylation(*one, flank=65, bin=1), E_RANGE,
                  "more than 64 bins per flank"))
    return cases, keep


def _outcome(capi, call):
    try:
        rc = call()
    except capi.NraError as e:
        rc = e.code
    rc = rc if isinstance(rc, int) else 0
    return rc, (capi.load().nra_last_error().decode(errors="replace") if rc != 0 else "")


def test_bad_arguments_give_their_code_and_text(capi):
    cases, _keep = _bad_calls(capi)
    for case, call, code, text in cases:
        assert _outcome(capi, call) == (code, text), case


def test_good_arguments_without_a_device_fail_loudly(capi):
    """n_reads = 0 too: like the other entry points, the call still looks for its device."""
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    empty = (np.zeros(0, np.int32), np.zeros(0, np.uint8))
    for reads in (["ACGCGT", "", "cgN"], []):
        n = len(reads)
        with pytest.raises(capi.NraError) as e:
            capi.read_methylation(reads, [empty] * n, np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32))
        assert e.value.code == E_DEVICE and "no HIP device" in str(e.value)


def test_symbol_is_declared_exported_and_additive(capi):
    assert "nra_read_methylation" in capi.EXPORTS and hasattr(capi.load(), "nra_read_methylation")
    header = open(os.path.join(ROOT, "include", "nanorepeat_amd.h")).read()
    assert re.search(r"int nra_read_methylation\(int device, int32_t n_reads, const char\* seqs, const int64_t\* seq_off,\s+"
                     r"const int32_t\* deltas, const uint8_t\* probs, const int64_t\* mod_off,\s+"
                     r"const uint8_t\* flags, const int32_t\* tract_lo, const int32_t\* tract_hi,\s+"
                     r"int32_t flank, int32_t bin, int32_t lo_byte, int32_t hi_byte,\s+"
                     r"int32_t\* counts, int32_t\* n_c, int32_t\* status\);", header)
    assert capi.load().nra_abi_version() == 4
