"""The error contract of nra_tract_periods, in the manner of test_capi_errors.py: every bad argument gives its code and
its nra_last_error text before the device is touched, so these run with and without a GPU; good arguments without a
device fail loudly (skipped where a GPU is present: the GPU suite covers the call there)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_RANGE = -1, -2, -3


def _bad_calls(capi):
    """[(case, call, code, text)]"""
    lib = capi.load()
    i64 = lambda a: capi._ptr(a, C.c_int64)
    i32 = lambda a: capi._ptr(a, C.c_int32)
    data, off = capi.pack_reads(["CAG"])
    m, v = np.zeros(64, np.int32), np.zeros(64, np.int32)
    negative, decreasing = np.array([-1, 2], np.int64), np.array([3, 1], np.int64)
    raw = lambda *a: lib.nra_tract_periods(0, *a)
    return [
        ("max_period 0", lambda: capi.tract_periods(["CAGCAG"], max_period=0), E_ARG, "max_period must be in 1..64"),
        ("max_period 65", lambda: capi.tract_periods(["CAGCAG"], max_period=65), E_ARG, "max_period must be in 1..64"),
        ("max_period -1", lambda: raw(1, data, i64(off), -1, i32(m), i32(v)), E_ARG, "max_period must be in 1..64"),
        ("tract too long", lambda: capi.tract_periods(["CAG", "A" * 200001]), E_RANGE,
         "tract 1 is longer than 200000 bases"),
        ("negative count", lambda: raw(-1, data, i64(off), 64, i32(m), i32(v)), E_ARG, "negative tract count"),
        ("every array NULL", lambda: raw(1, data, None, 64, None, None), E_ARG, "NULL tract array"),
        ("seq_off NULL", lambda: raw(1, data, None, 64, i32(m), i32(v)), E_ARG, "NULL tract array"),
        ("match NULL", lambda: raw(1, data, i64(off), 64, None, i32(v)), E_ARG, "NULL tract array"),
        ("valid NULL", lambda: raw(1, data, i64(off), 64, i32(m), None), E_ARG, "NULL tract array"),
        ("seqs NULL", lambda: raw(1, None, i64(off), 64, i32(m), i32(v)), E_ARG, "seqs is NULL"),
        ("negative tract offset", lambda: raw(1, data, i64(negative), 64, i32(m), i32(v)), E_ARG,
         "negative tract offset"),
        ("tract offsets decrease", lambda: raw(1, data, i64(decreasing), 64, i32(m), i32(v)), E_ARG,
         "tract offsets must not decrease"),
    ]


def _outcome(capi, call):
    try:
        rc = call()
    except capi.NraError as e:
        rc = e.code
    rc = rc if isinstance(rc, int) else 0
    return rc, (capi.load().nra_last_error().decode(errors="replace") if rc != 0 else "")


def test_bad_arguments_give_their_code_and_text(capi):
    for case, call, code, text in _bad_calls(capi):
        assert _outcome(capi, call) == (code, text), case


def test_good_arguments_without_a_device_fail_loudly(capi):
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    for tracts in (["CAGCAG", "", "A" * 200000], []):
        with pytest.raises(capi.NraError) as e:
            capi.tract_periods(tracts)
        assert e.value.code == E_DEVICE and "no HIP device" in str(e.value)


def test_symbol_is_declared_exported_and_additive(capi):
    assert "nra_tract_periods" in capi.EXPORTS and hasattr(capi.load(), "nra_tract_periods")
    header = open(os.path.join(ROOT, "include", "nanorepeat_amd.h")).read()
    assert re.search(r"int nra_tract_periods\(int device, int32_t n_tracts, const char\* seqs, const int64_t\* seq_off,\s+"
                     r"int32_t max_period,\s+int32_t\* match, int32_t\* valid\);", header)
    assert capi.load().nra_abi_version() == 4
