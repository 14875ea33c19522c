"""nra_place_* on the device against tests/place_ref.py: every comparison is exact, the candidates
and every counter the contract defines."""
import ctypes as C

import numpy as np
import pytest

import place_cases as cases
import place_ref as R

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -5


def run(capi, c, again=()):
    """The device's (candidates, stats) for a case; with `again`, the candidates of further nra_place_candidates calls
    on the same handle, each a dict of the parameters that differ."""
    h = capi.place_create(c["queries"], c["k"], c["max_occ"])
    try:
        for t, pos0, bases in c["chunks"]:
            capi.place_scan(h, t, pos0, bases)
        out = []
        for over in ({},) + tuple(again):
            p = dict(c, **over)
            got = capi.place_candidates(h, p["bin"], p["max_target_occ"], p["min_votes"])
            out.append((list(zip(*(got[key].tolist() for key in R.KEYS))), capi.place_stats(h)))
        return out if again else out[0]
    finally:
        capi.place_destroy(h)


def same(capi, c, **over):
    """The device's result for a case equals the restatement's; returns (candidates, the device's stats)."""
    c = dict(c, **over)
    got, st = run(capi, c)
    want, counters = R.candidates(**c)
    assert got == want
    assert {key: st[key] for key in R.COUNTERS} == counters
    assert st["tile_windows"] == cases.TILE
    return got, st


def votes_of(cands, q, t, s):
    return {b: v for cq, ct, cs, b, v in cands if (cq, ct, cs) == (q, t, s)}


@pytest.mark.parametrize("k", [11, 13, 15])
def test_query_edges_and_both_strands(capi, k):
    c = cases.edge_case(k)
    cands, st = same(capi, c, bin=1)
    n_win = cases.MAX_LEN - k + 1
    assert not [x for x in cands if x[0] in (0, 1, 5, 8, 9)]                      # no posting: no candidate
    at = 300 + k + 1 + 100
    assert votes_of(cands, 3, 0, 0)[300] == 2 and votes_of(cands, 2, 0, 0) == {}  # min_votes = 2: query 2 has one window
    for q in (4, 6, 7):                                                           # either case: d = i - j
        v = votes_of(cands, q, 0, 0)
        assert v[at] >= n_win - 20 and v[at - 1] >= n_win - 20 and max(v.values()) == max(v[at], v[at - 1])
    for t, pos0 in ((1, 0), (2, (1 << 30) - len(c["chunks"][1][2]))):             # d = i + j + k - len(q)
        v = votes_of(cands, 4, t, 1)
        assert v[pos0 + 150] >= n_win - 20 and votes_of(cands, 4, t, 0).get(pos0 + 150, 0) < 10
        v = votes_of(cands, 10, t, 0)                                             # the last windows before the Ns
        assert v[pos0 + 150 + 2048 + 50] >= n_win - 20
    assert st["kernel_ms"] > 0 and st["n_chunks"] == 3
    same(capi, c, bin=64, min_votes=1)


def test_every_byte_offset_of_the_queries(capi):
    c = cases.offset_case()
    cands, _ = same(capi, c)
    assert {q for q, *_ in cands} == set(range(16)) and {s for _, _, s, _, _ in cands} == {0, 1}


@pytest.mark.parametrize("n", [1, 2, 65, 4096])
def test_query_counts(capi, n):
    cands, st = same(capi, cases.count_case(n))
    planted = sorted({0, n // 3, n // 2, (2 * n) // 3, n - 1})
    assert sorted({q for q, _, _, _, v in cands if v >= 20}) == planted
    assert st["n_postings"] >= n * 27 and all(t == 5 for _, t, _, _, _ in cands)


@pytest.mark.parametrize("tiles, extra", [(1, -1), (1, 0), (1, 1), (2, 1)])
def test_tile_edges_and_first_and_last_window(capi, tiles, extra):
    n_win = tiles * cases.TILE + extra
    c = cases.tile_case(n_win)
    cands, st = same(capi, c, min_votes=10)
    assert st["n_target_windows"] == n_win
    assert votes_of(cands, 0, 0, 0)[77 // 64] == 18 and max(votes_of(cands, 1, 0, 1).values()) == 18
    same(capi, c, min_votes=1)


def test_chunks_cut_at_every_offset(capi):
    whole, st_whole = same(capi, cases.cut_case(cuts=()))
    parts, st_parts = same(capi, cases.cut_case())
    assert parts == whole and len(whole) >= 8 and st_parts["n_chunks"] == 17 and st_whole["n_chunks"] == 1
    for key in ("n_target_windows", "n_hits_kept"):
        assert st_parts[key] == st_whole[key]
    assert st_parts["target_bases"] == st_whole["target_bases"] + 16 * 12


def test_chunk_order_and_interleaved_contigs(capi):
    results = [same(capi, c) for c in cases.two_contig_case()]
    assert results[0][0] == results[1][0] == results[2][0] and {t for _, t, _, _, _ in results[0][0]} == {0, 1}
    assert {key: results[0][1][key] for key in R.COUNTERS} == {key: results[1][1][key] for key in R.COUNTERS}


@pytest.mark.parametrize("bin", [1, 64, 4096])
def test_diagonals_at_bin_edges(capi, bin):
    c, ds = cases.bin_edge_case(bin)
    cands, _ = same(capi, c, min_votes=20)
    for t, d in enumerate(ds):
        v = votes_of(cands, 0, t, 0)
        hits = 300 - 13 + 1 - max(0, -d)                  # an overhanging query loses the windows before the contig
        assert v == {d // bin - 1: hits, d // bin: hits}, (t, d)
    c, ds = cases.reverse_edge_case(bin=64)
    cands, _ = same(capi, c, min_votes=20)
    for t, d in enumerate(ds):
        hits = 300 - 13 + 1 - max(0, -d)
        assert votes_of(cands, 0, t, 1) == {d // 64 - 1: hits, d // 64: hits}, (t, d)


def test_thresholds_at_the_value_and_one_past(capi):
    c = cases.occ_case()
    kept, st = same(capi, c)                                                      # max_occ = 3: X in, Y out
    assert st["n_masked_max_occ"] == 150 - 13 + 1 and {q for q, *_ in kept} == {0, 1, 2}
    none, st = same(capi, c, max_occ=2)
    assert none == [] and st["n_keys"] == 0 and st["n_target_windows"] > 0
    both, _ = same(capi, c, max_occ=4)
    assert {q for q, *_ in both} == set(range(7))
    at, st_at = same(capi, c, max_target_occ=5)                                   # occ = 5 for every key
    past, st_past = same(capi, c, max_target_occ=4)
    assert at and past == [] and st_at["n_keys_over"] == 0 and st_past["n_keys_over"] == st_past["n_keys"]
    top = max(v for *_, v in kept)
    assert [x for x in same(capi, c, min_votes=top)[0] if x[4] == top] and same(capi, c, min_votes=top + 1)[0] == []


def test_hot_keys_leave_no_candidate(capi):
    c = cases.hot_case()
    cands, st = same(capi, c)
    assert cands == [] and st["n_hits_kept"] == 0 and st["n_keys_over"] == st["n_keys"] == 2000 - 13 + 1


def test_a_target_dense_with_hits_counts_every_window_once(capi):
    c = cases.dense_case()
    cands, st = same(capi, c)
    assert st["n_hits_kept"] >= 8 * 1980 and st["n_keys_over"] <= 4 and len(cands) >= 16    # a few k-mers occur twice
    assert all(v >= 1980 for *_, v in cands)
    assert same(capi, c, max_target_occ=7)[0] == []


def test_candidates_again_on_the_same_handle(capi):
    c, _ = cases.noisy_case("hifi", n_sides=20, contig_len=50_000, n_contigs=2)
    others = (dict(bin=16, min_votes=3), dict(bin=4096, max_target_occ=1, min_votes=1), {})
    results = run(capi, c, again=others)
    for over, (got, st) in zip(({},) + others, results):
        want, counters = R.candidates(**dict(c, **over))
        assert got == want and {key: st[key] for key in R.COUNTERS} == counters
    assert results[0][0] == results[3][0] and results[0][0] != results[1][0]
    # more chunks after a candidates call: the same as all of them before it
    h = capi.place_create(c["queries"], c["k"], c["max_occ"])
    half = len(c["chunks"]) // 2
    for t, pos0, bases in c["chunks"][:half]:
        capi.place_scan(h, t, pos0, bases)
    capi.place_candidates(h, c["bin"], c["max_target_occ"], c["min_votes"])
    for t, pos0, bases in c["chunks"][half:]:
        capi.place_scan(h, t, pos0, bases)
    got = capi.place_candidates(h, c["bin"], c["max_target_occ"], c["min_votes"])
    capi.place_destroy(h)
    assert list(zip(*(got[key].tolist() for key in R.KEYS))) == results[0][0]


def test_capacity_exact_and_one_too_small(capi):
    c = cases.count_case(65)
    want, _ = R.candidates(**c)
    lib = capi.load()
    h = capi.place_create(c["queries"], c["k"], c["max_occ"])
    for t, pos0, bases in c["chunks"]:
        capi.place_scan(h, t, pos0, bases)
    for cap in (len(want) - 1, len(want)):
        out = [np.full(len(want), -7, np.int32) for _ in R.KEYS]
        n = C.c_int64(cap)
        rc = lib.nra_place_candidates(h, c["bin"], c["max_target_occ"], c["min_votes"], C.byref(n),
                                      *(capi._ptr(x, C.c_int32) for x in out))
        assert n.value == len(want) > 4
        if cap < len(want):
            assert rc == capi.E_RANGE and all((x == -7).all() for x in out)
        else:
            assert rc == 0 and list(zip(*(x.tolist() for x in out))) == want
    got = capi.place_candidates(h, c["bin"], c["max_target_occ"], c["min_votes"], capacity=1)   # the wrapper retries
    capi.place_destroy(h)
    assert list(zip(*(got[key].tolist() for key in R.KEYS))) == want


def test_errors_and_limits(capi, monkeypatch):
    lib = capi.load()
    seqs = ["ACGTTGCAAGGCTTAACCGGATAT" * 4] * 3
    data, off = capi.pack_reads(seqs)

    def create(n=3, data=data, off=off, k=13, max_occ=16, out=True):
        h = C.c_void_p()
        rc = lib.nra_place_create(0, n, data, capi._ptr(off, C.c_int64), k, max_occ, C.byref(h) if out else None)
        if rc == 0:
            capi.place_destroy(h)
        return rc

    assert create() == 0 and create(n=0) == 0 and create(n=0, data=None, off=None) == 0
    for k in (9, 10, 12, 14, 16, 17):
        assert create(k=k) == E_ARG
    assert create(max_occ=0) == E_ARG and create(max_occ=256) == E_ARG and create(max_occ=255) == 0
    assert create(n=-1) == E_ARG and create(out=False) == E_ARG and create(off=None) == E_ARG
    assert create(data=None) == E_ARG and create(off=off[::-1].copy()) == E_ARG
    long_data, long_off = capi.pack_reads(["A" * 2049, "ACGT"])
    assert create(n=2, data=long_data, off=long_off) == capi.E_RANGE and b"2048" in lib.nra_last_error()
    ok_data, ok_off = capi.pack_reads(["A" * 2048, "ACGT"])
    assert create(n=2, data=ok_data, off=ok_off) == 0
    many = capi.PLACE_MAX_QUERIES + 1
    assert create(n=many, data=b"", off=np.zeros(many + 1, np.int64)) == capi.E_RANGE
    assert create(n=many - 1, data=b"", off=np.zeros(many, np.int64)) == 0

    h = capi.place_create(seqs)
    target = seqs[0] * 3
    scan = lambda contig=0, pos0=0, bases=target.encode(), n=len(target): lib.nra_place_scan(h, contig, pos0, bases, n)
    assert scan() == 0 and scan(n=0) == 0 and scan(n=12) == 0 and scan(bases=None, n=0) == 0
    assert scan(contig=-1) == E_ARG and scan(pos0=-1) == E_ARG and scan(n=-1) == E_ARG and scan(bases=None) == E_ARG
    top = capi.PLACE_MAX_POS
    assert scan(pos0=top - len(target)) == 0 and scan(pos0=top - len(target) + 1) == capi.E_RANGE
    assert lib.nra_place_scan(None, 0, 0, target.encode(), len(target)) == E_ARG
    assert capi.place_stats(h)["n_chunks"] == 5                                   # the failed scans left no trace

    out = [np.zeros(4096, np.int32) for _ in R.KEYS]

    def cand(bin=64, occ=64, votes=1, cap=4096, arrays=out, n=True):
        n_cand = C.c_int64(cap)
        return lib.nra_place_candidates(h, bin, occ, votes, C.byref(n_cand) if n else None,
                                        *(capi._ptr(x, C.c_int32) for x in arrays))

    assert cand() == 0 and cand(bin=1) == 0 and cand(bin=4096) == 0 and cand(occ=1) == 0
    assert cand(bin=0) == E_ARG and cand(bin=4097) == E_ARG and cand(occ=0) == E_ARG and cand(occ=65536) == E_ARG
    assert cand(votes=0) == E_ARG and cand(cap=-1) == E_ARG and cand(n=False) == E_ARG
    assert cand(arrays=out[:4] + [None]) == E_ARG
    assert cand(occ=capi.PLACE_OCC_CEILING) == 0 and cand(occ=capi.PLACE_OCC_CEILING + 1) == capi.E_RANGE
    assert str(capi.PLACE_OCC_CEILING).encode() in lib.nra_last_error()
    assert lib.nra_place_stats(h, None) == E_ARG and lib.nra_place_destroy(None) == 0
    capi.place_destroy(h)

    # the cap on kept hits, lowered for the test: the scan that passes it fails, and so does every call after it
    monkeypatch.setenv("NRA_TEST_PLACE_MAX_HITS", str(3 * (96 - 13 + 1) - 1))
    h = capi.place_create(seqs[:1])
    monkeypatch.delenv("NRA_TEST_PLACE_MAX_HITS")
    assert lib.nra_place_scan(h, 0, 0, target.encode(), len(target)) == capi.E_RANGE
    assert b"max_occ" in lib.nra_last_error()
    assert lib.nra_place_scan(h, 0, 0, target.encode(), len(target)) == E_STATE and cand() == E_STATE
    capi.place_destroy(h)


@pytest.mark.parametrize("model", ["ont", "hifi"])
def test_noisy_sides_in_a_2_mb_reference(capi, model):
    c, truth = cases.noisy_case(model)
    cands, st = same(capi, c)
    assert st["n_chunks"] == 8 and st["target_bases"] > 2_000_000
    best = {}
    for q, t, s, b, v in cands:
        if v > best.get(q, (0,))[0]:
            best[q] = (v, t, s, b)
    for q, (t, s, at) in enumerate(truth):                 # every side's best candidate is where it was cut from
        v, bt, bs, b = best[q]
        assert (bt, bs) == (t, s) and abs(b * 64 - at) <= 3 * 64 and v >= 8, (q, best[q], truth[q])
