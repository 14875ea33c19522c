"""Alignment paths on the device across every form of the trace kernels (nra_trace.hip).

Each pair's record from nra_align_pairs_cigar / nra_align_paths is held three ways: against the oracle's traceback bit
for bit (score, CIGAR, tstart, tend, qstart, qend), against the independent path check of tests/path_check.py (grammar,
extents, bases, score; the oracle's traceback itself is pinned by test_path_check_cpu.py), and against the extents of
nra_align_pairs.  The cases (tests/paths_cases.py) walk the forms the kernels are built in: the 24 rows-per-lane classes
of k_trace_fill at their first and last query length, the 9 row-block heights of k_trace_fill_mt in int32 and 64-bit
cells, each with and without N (HAS_N is a property of a call, so a list is split into a call without N and one with),
nine scoring schemes that turn the choices of the trace byte into ties, target lengths where the chunk count turns
over, origin columns beyond 15 bits, equal maxima across lanes and row blocks, and the last score of the int32 cell."""
import importlib.util
import os

import numpy as np
import pytest

import paths_cases as PC
from path_check import check_path

pytestmark = pytest.mark.gpu

FIELDS = ("score", "cigar", "tstart", "tend", "qstart", "qend")
BLOCK_ROWS_ENV = "NRA_TEST_TRACE_BLOCK_ROWS"


@pytest.fixture(scope="module")
def want_of(oracle):
    """The oracle's record of a pair under a scheme, computed once per (scheme, pair) of the module."""
    memo = {}

    def want(pair, over):
        key = (tuple(sorted(over.items())), pair["q"], pair["t"])
        if key not in memo:
            memo[key] = oracle.align_cigar(pair["q"], pair["t"], oracle.default_scoring(**PC.scheme_values(over)))
        return memo[key]
    return want


def run_pairs(capi, want_of, pairs, over, call):
    """`pairs` through `call` (capi.align_pairs_cigar or capi.align_paths), the pairs without N in one call and those
    with N in another; every field against the oracle, the device's record through check_path, and score / tstart / tend
    against nra_align_pairs.  Returns ({pair name: device record}, the set of HAS_N forms that ran)."""
    v = PC.scheme_values(over)
    sc = capi.default_scoring(**v)
    got, forms = {}, set()
    for with_n in (False, True):
        part = [p for p in pairs if PC.has_n(p) == with_n]
        if not part:
            continue
        forms.add(with_n)
        seqs = [s for p in part for s in (p["q"], p["t"])]
        pq, pt = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
        g = call(seqs, pq, pt, sc=sc)
        ext = capi.align_pairs(seqs, pq, pt, sc=sc)
        for i, p in enumerate(part):
            o = want_of(p, over)
            assert o["score"] >= 1, p["name"]                            # every pair here is meant to give a record
            rec = dict(score=int(g["score"][i]), cigar=g["cigar"][i], **{k: int(g[k][i]) for k in FIELDS[2:]})
            assert tuple(rec[k] for k in FIELDS) == tuple(o[k] for k in FIELDS), \
                (p["name"], call.__name__, [(k, rec[k], o[k]) for k in FIELDS if rec[k] != o[k]])
            check_path(p["q"], p["t"], rec, v, optimum=o["score"])
            assert tuple(int(ext[k][i]) for k in ("score", "tstart", "tend")) == (rec["score"], rec["tstart"], rec["tend"]), p["name"]
            got[p["name"]] = rec
    return got, forms


def three_ways(capi, want_of, monkeypatch, pairs, over, cigar_pairs=None):
    """nra_align_pairs_cigar, nra_align_paths, and nra_align_paths in row blocks of 64 rows."""
    monkeypatch.delenv(BLOCK_ROWS_ENV, raising=False)
    a, fa = run_pairs(capi, want_of, pairs if cigar_pairs is None else cigar_pairs, over, capi.align_pairs_cigar)
    b, fb = run_pairs(capi, want_of, pairs, over, capi.align_paths)
    monkeypatch.setenv(BLOCK_ROWS_ENV, "64")
    c, fc = run_pairs(capi, want_of, pairs, over, capi.align_paths)
    monkeypatch.delenv(BLOCK_ROWS_ENV)
    return (a, b, c), (fa, fb, fc)


def test_every_register_class_of_the_one_block_fill(capi, want_of, monkeypatch):
    """k_trace_fill<R, HAS_N> for the 24 classes of NRA_R_LIST, each at 64 R bases (every lane full, the best cell in the
    last lane) and at 64 R_prev + 1 (the first length of the class), in a call without N and a call with N."""
    monkeypatch.delenv(BLOCK_ROWS_ENV, raising=False)
    plain, with_n = PC.class_border_pairs()
    for pairs, n in ((plain, False), (with_n, True)):
        assert {p["R"] for p in pairs} == set(PC.r_list()) and len(PC.r_list()) == 24
        assert all(PC.has_n(p) == n for p in pairs)
        for call in (capi.align_pairs_cigar, capi.align_paths):
            got, forms = run_pairs(capi, want_of, pairs, {}, call)
            assert forms == {n} and len(got) == len(pairs)
            for p in pairs:
                if p["last_lane"] and not n:
                    assert (got[p["name"]]["qend"] - 1) // p["R"] == 63, p["name"]


@pytest.mark.parametrize("rows", PC.TRACE_BLOCK_ROWS)
def test_every_row_block_height(capi, want_of, monkeypatch, rows):
    """k_trace_fill_mt<R, HAS_N, W> at each height it is built for, in int32 and in 64-bit cells, without and with N: a
    30-base insertion across the first seam, a path across the last seam into a block of 5 rows, N runs across both, the
    same under match = 64, and equal maxima in two row blocks for k_trace_best."""
    monkeypatch.setenv(BLOCK_ROWS_ENV, str(rows))
    forms = set()                                                      # (64-bit cells, HAS_N)
    # the queries of 2 * rows + 5 bases, those again under match = 64, and under match = 64 one of more than 500 bases
    for wide, nb in [(False, 2)] + sorted({(True, 2), (True, max(2, -(-496 // rows)))}):
        over = dict(match=64) if wide else {}
        pairs = PC.row_block_pairs(rows, wide, nb)
        assert max(len(p["q"]) for p in pairs) <= 3077 and max(len(p["t"]) for p in pairs) <= 520
        w = {PC.is_wide(p, PC.scheme_values(over)["match"]) for p in pairs}
        assert len(w) == 1
        got, ns = run_pairs(capi, want_of, pairs, over, capi.align_paths)
        assert ns == {False, True}
        forms |= {(min(w), n) for n in ns}
        for p in pairs:
            r = got[p["name"]]
            assert r["qstart"] < p["seam"] < r["qend"], (p["name"], r["qstart"], r["qend"])
            assert p["planted"] is None or p["planted"] in r["cigar"], (p["name"], r["cigar"])
    assert forms == {(False, False), (False, True), (True, False), (True, True)}, forms
    ties = PC.best_cell_tie_pairs(rows)
    got, _ = run_pairs(capi, want_of, ties, {}, capi.align_paths)
    assert all(got[p["name"]]["score"] == 80 for p in ties)
    assert got[ties[0]["name"]]["qend"] < rows and got[ties[2]["name"]]["qend"] < rows      # the copy in the first block


@pytest.mark.parametrize("name,over", PC.SCHEMES, ids=[n for n, _ in PC.SCHEMES])
def test_scoring_schemes_and_tie_rules(capi, want_of, monkeypatch, name, over):
    """The repeat panel (where the surplus units go is tie-breaking alone) and gaps on either side of the knee under each
    scheme, three ways."""
    pairs = PC.repeat_panel(over) + PC.knee_pairs(over)
    match = PC.scheme_values(over)["match"]
    short = [p for p in pairs if match * len(p["q"]) <= 32000]         # what nra_align_pairs_cigar accepts
    assert short and (name == "match64" or len(short) == len(pairs))
    got, forms = three_ways(capi, want_of, monkeypatch, pairs, over, cigar_pairs=short)
    assert all(f == {False, True} for f in forms)
    assert len(got[0]) == len(short) and len(got[1]) == len(got[2]) == len(pairs)


def test_target_lengths_at_the_chunk_edges(capi, want_of, monkeypatch):
    """Targets of 1, 63 .. 65, 127 .. 129 and 191 .. 193 columns: (ncols + 126) >> 6 chunks of 64 pipeline steps."""
    pairs = PC.target_edge_pairs()
    assert sorted({len(p["t"]) for p in pairs}) == [1, 63, 64, 65, 127, 128, 129, 191, 192, 193]
    got, _ = three_ways(capi, want_of, monkeypatch, pairs, {})
    for way in got:
        for p in pairs:
            r = way[p["name"]]
            assert (r["tend"] == len(p["t"])) if p["edge"] == "end" else (r["tstart"] == 0), (p["name"], r)


def test_origin_columns_beyond_15_bits(capi, want_of, monkeypatch):
    """The origin column in the low 16 bits of the int32 cell, beyond 32767 and at the end of the longest target."""
    pairs = PC.long_target_pairs()
    assert max(len(p["t"]) for p in pairs) == 65000
    monkeypatch.delenv(BLOCK_ROWS_ENV, raising=False)
    a, _ = run_pairs(capi, want_of, pairs, {}, capi.align_pairs_cigar)
    monkeypatch.setenv(BLOCK_ROWS_ENV, "64")
    b, _ = run_pairs(capi, want_of, pairs, {}, capi.align_paths)
    for got in (a, b):
        for p in pairs:
            assert (got[p["name"]]["tstart"], got[p["name"]]["tend"]) == (p["tstart"], p["tend"]), p["name"]
        assert sum(r["tstart"] > 32767 for r in got.values()) == 2
        assert got["long:65000:end"]["tstart"] == 64840 and got["long:65000:end"]["tend"] == 64990


def test_score_32000_and_the_first_wide_pair(capi, want_of, monkeypatch):
    """match = 64: 500 identical bases score 32 000 in int32 cells through both entry points; 501 score 32 064 in 64-bit
    cells through nra_align_paths, without and with an N, and are out of nra_align_pairs_cigar's range."""
    monkeypatch.delenv(BLOCK_ROWS_ENV, raising=False)
    over = dict(match=64)
    p500, p501, p501n = PC.score_border_pairs()
    assert not PC.is_wide(p500, 64) and PC.is_wide(p501, 64) and PC.is_wide(p501n, 64)
    for call in (capi.align_pairs_cigar, capi.align_paths):
        got, _ = run_pairs(capi, want_of, [p500], over, call)
        assert got[p500["name"]]["score"] == 32000 and got[p500["name"]]["cigar"] == "500="
    got, forms = run_pairs(capi, want_of, [p501, p501n], over, capi.align_paths)
    assert forms == {False, True}
    assert got[p501["name"]]["score"] == 32064 and got[p501["name"]]["cigar"] == "501="
    assert got[p501n["name"]]["score"] == 31999 and got[p501n["name"]]["cigar"] == "250=1X250="
    for p in (p501, p501n):
        with pytest.raises(capi.NraError) as e:
            capi.align_pairs_cigar([p["q"], p["t"]], [0], [1], sc=capi.default_scoring(**PC.scheme_values(over)))
        assert e.value.code == capi.E_RANGE


def test_differential_fuzz_paths():
    """40 rounds of tools/gpu_fuzz.py's fuzz_cigar (both path entry points and a random row-block height against the
    oracle and the path check) and 10 of fuzz_pairs, seed fixed.  Measured on an MI355X: 1.0 s for the 40 + 10 rounds."""
    spec = importlib.util.spec_from_file_location(
        "gpu_fuzz", os.path.join(os.path.dirname(__file__), "..", "tools", "gpu_fuzz.py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    rng = np.random.default_rng(20260509)
    for _ in range(40):
        assert fz.fuzz_cigar(rng) is None
    for _ in range(10):
        assert fz.fuzz_pairs(rng) is None
