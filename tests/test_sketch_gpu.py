"""nra_sketch_pairs on the device against tests/sketch_ref.py: every comparison is exact, pairs,
sketch_size and the counters n_windows, n_kmers and n_compared."""
import ctypes as C

import numpy as np
import pytest

import sketch_cases as cases
import sketch_ref as R

pytestmark = pytest.mark.gpu
KEYS = ("a", "b", "shared")
COUNTERS = ("n_windows", "n_kmers", "n_compared")


def as_tuples(got):
    return list(zip(*(got[key].tolist() for key in KEYS)))


def same(capi, c, **over):
    """The device's result for a case equals the restatement's; returns (pairs, sketch sizes, the device's stats)."""
    c = dict(c, **over)
    got = capi.sketch_pairs(c["seqs"], c["groups"], c["k"], c["min_shared"])
    want, sizes, stats = R.pairs(c["seqs"], c["groups"], c["k"], c["min_shared"])
    assert as_tuples(got) == want
    assert got["sketch_size"].tolist() == sizes
    assert {key: got["stats"][key] for key in COUNTERS} == stats
    return want, sizes, got["stats"]


@pytest.mark.parametrize("k", [11, 13, 15])
def test_sequence_edges(capi, k):
    c = cases.edge_case(k)
    pairs, sizes, st = same(capi, c)
    shared = {(a, b): n for a, b, n in pairs}
    assert sizes[0] == sizes[1] == sizes[6] == sizes[9] == sizes[10] == 0 and sizes[2] == 1 and sizes[3] == 2
    assert sizes[4] > 2000 and sizes[7] == sizes[8] == sizes[4]
    assert shared[(4, 7)] == shared[(4, 8)] == shared[(4, 11)] == sizes[4] == sizes[11]   # case, reverse complement
    assert sizes[12] == sizes[13] == shared[(12, 13)] and 298 <= sizes[12] <= 300          # every k-mer twice: once
    assert shared[(2, 3)] == 1 and shared[(3, 14)] == 2 and (0, 1) not in shared
    assert st["n_tiles"] == len(c["seqs"]) - 1 and st["kernel_ms"] > 0


def test_every_byte_offset(capi):
    c = cases.offset_case()
    pairs, sizes, _ = same(capi, c)
    assert len(pairs) > 60 and min(sizes) > 50
    for i in range(15):                                     # each alone with its neighbour: other offsets again
        same(capi, cases.case(c["seqs"][i:i + 2], [0, 0], c["k"]))


def test_group_sizes(capi):
    c = cases.group_size_case()
    pairs, _, st = same(capi, c)
    sizes = (1, 2, 64, 65, 257)
    assert st["n_compared"] == sum(n * (n - 1) // 2 for n in sizes)
    assert st["n_tiles"] == sum(sum((n - 1 - s + 63) // 64 for s in range(n)) for n in sizes)
    first = np.cumsum((0,) + sizes)
    per_group = [sum(1 for a, _, _ in pairs if first[g] <= a < first[g + 1]) for g in range(5)]
    assert per_group[0] == 0 and per_group[1] == 1 and per_group[4] > 257 * 100
    assert all(np.searchsorted(first, a, "right") == np.searchsorted(first, b, "right") for a, b, _ in pairs)


def test_group_boundaries(capi):
    c = cases.boundary_case()
    pairs, _, _ = same(capi, c)
    assert [(a, b) for a, b, _ in pairs] == [(0, 1), (0, 2), (1, 2), (3, 4), (5, 6), (5, 7), (6, 7), (8, 9)]
    # shuffled, non-contiguous group ids: the same pairs, mapped back
    n = cases.noisy_case("hifi")
    want, _, _ = same(capi, n)
    order = np.random.default_rng(3).permutation(len(n["seqs"]))
    shuffled = cases.case([n["seqs"][i] for i in order], [1000 - 13 * n["groups"][i] for i in order], n["k"],
                          n["min_shared"])
    got, _, _ = same(capi, shuffled)
    back = sorted((min(order[a], order[b]), max(order[a], order[b]), s) for a, b, s in got)
    assert back == want and len(want) >= 30 * 12


def test_min_shared_and_capacity(capi, monkeypatch, capfd):
    c = cases.noisy_case("ont")
    want, _, _ = same(capi, c)
    a, b, n = want[len(want) // 2]
    pair = cases.case([c["seqs"][a], c["seqs"][b]], [0, 0], c["k"])
    at, _, _ = same(capi, pair, min_shared=n)
    above, _, _ = same(capi, pair, min_shared=n + 1)
    assert at == [(0, 1, n)] and above == []

    lib = capi.load()
    data, off = capi.pack_reads(c["seqs"])
    grp = np.asarray(c["groups"], np.int32)
    for cap in (len(want) - 1, len(want)):
        out = [np.full(len(want), -7, np.int32) for _ in KEYS]
        size = np.full(len(c["seqs"]), -7, np.int32)
        n_pairs = C.c_int64(cap)
        rc = lib.nra_sketch_pairs(0, len(c["seqs"]), data, capi._ptr(off, C.c_int64), capi._ptr(grp, C.c_int32), c["k"],
                                  c["min_shared"], C.byref(n_pairs), *(capi._ptr(x, C.c_int32) for x in out),
                                  capi._ptr(size, C.c_int32), None)
        assert n_pairs.value == len(want)
        if cap < len(want):
            assert rc == capi.E_RANGE and all((x == -7).all() for x in out) and (size == -7).all()
        else:
            assert rc == 0 and list(zip(*(x.tolist() for x in out))) == want

    monkeypatch.setenv("NRA_DEBUG", "1")
    monkeypatch.setenv("NRA_TEST_SKETCH_PAIR_CAP", "1")
    capfd.readouterr()
    same(capi, c)
    assert capfd.readouterr().err.count(f"pair list grows from 1 to {len(want)}") == 1
    monkeypatch.delenv("NRA_DEBUG")
    monkeypatch.delenv("NRA_TEST_SKETCH_PAIR_CAP")
    same(capi, c)                                           # the variables are read at every call
    assert capfd.readouterr().err == ""


def test_argument_errors(capi):
    lib = capi.load()
    seqs = ["ACGTTGCAAGGCTTAACCGGATAT" * 4] * 3
    data, off = capi.pack_reads(seqs)
    grp = np.zeros(3, np.int32)
    out = [np.zeros(8, np.int32) for _ in range(4)]

    def call(n=3, data=data, off=off, grp=grp, k=13, min_shared=1, cap=8, arrays=out, n_pairs=True):
        n_pairs_v = C.c_int64(cap)
        return lib.nra_sketch_pairs(0, n, data, capi._ptr(off, C.c_int64), capi._ptr(grp, C.c_int32), k, min_shared,
                                    C.byref(n_pairs_v) if n_pairs else None,
                                    *(capi._ptr(x, C.c_int32) for x in arrays), None)

    E_ARG, E_RANGE = -1, capi.E_RANGE
    assert call() == 0 and call(n=0) == 0
    for k in (9, 10, 12, 14, 16, 17):
        assert call(k=k) == E_ARG
    assert call(min_shared=0) == E_ARG and call(n=-1) == E_ARG and call(cap=-1) == E_ARG
    assert call(n_pairs=False) == E_ARG and call(off=None) == E_ARG and call(grp=None) == E_ARG
    assert call(data=None) == E_ARG and call(arrays=[None] + out[1:]) == E_ARG
    assert call(arrays=out[:3] + [None]) == 0                                 # sketch_size may be NULL
    assert call(off=off[::-1].copy()) == E_ARG                                # offsets that decrease
    long_data, long_off = capi.pack_reads(["A" * 2049, "ACGT"])
    assert call(n=2, data=long_data, off=long_off) == E_RANGE
    ok_data, ok_off = capi.pack_reads(["A" * 2048, "ACGT"])
    assert call(n=2, data=ok_data, off=ok_off) == 0
    big = capi.SKETCH_MAX_GROUP + 1
    many_off = np.zeros(big + 1, np.int64)
    assert call(n=big, data=b"", off=many_off, grp=np.full(big, 5, np.int32)) == E_RANGE
    assert b"65536" in lib.nra_last_error()
    at_limit = np.full(big, 5, np.int32)
    at_limit[-1] = 6
    size = np.full(big, -1, np.int32)                                          # one sketch size per sequence
    assert call(n=big, data=b"", off=many_off, grp=at_limit, cap=0, arrays=out[:3] + [size]) == 0   # 65 536 in a group
    assert not size.any()


def test_every_tile_of_the_largest_group(capi):
    """65 536 sequences in one group are 33.5 M tiles, 2^33 threads: more than one launch can hold.  All but seven of the
    sequences are empty (their tiles end at once); the seven sit where the first, the middle and the last tiles are.  The
    result does not depend on the other sequences, so the restatement of the seven alone says what to expect."""
    n = capi.SKETCH_MAX_GROUP
    flank = cases.synth.rand_seq(np.random.default_rng(37), 60)
    where = [0, 1, 30000, 50000, 65000, n - 2, n - 1]
    seqs = [""] * n
    for i in where:
        seqs[i] = flank
    got = capi.sketch_pairs(seqs, [9] * n, 13, 1)
    small, sizes, _ = R.pairs([flank] * len(where), [0] * len(where), 13, 1)
    assert len(small) == 21 and as_tuples(got) == [(where[a], where[b], s) for a, b, s in small]
    assert got["sketch_size"][where].tolist() == sizes and int(got["sketch_size"].sum()) == sum(sizes)
    assert got["stats"]["n_tiles"] == sum((n - 1 - s + 63) // 64 for s in range(n)) > 1 << 25
    assert got["stats"]["n_compared"] == n * (n - 1) // 2


@pytest.mark.parametrize("model", ["ont", "hifi"])
def test_noisy_flanks(capi, model):
    c = cases.noisy_case(model)
    pairs, _, _ = same(capi, c)
    locus = lambda i: (i // 10, (0, 0, 0, 0, 1, 1, 1, 2, 2, 2)[i % 10])
    assert all(locus(a) == locus(b) for a, b, _ in pairs) and len(pairs) == 30 * (6 + 3 + 3)


def test_full_sequences(capi):
    c = cases.full_case()
    pairs, sizes, _ = same(capi, c)
    assert min(sizes) > 2000 and [(a, b) for a, b, n in pairs if n > 100] == [(2 * i, 2 * i + 1) for i in range(10)]
