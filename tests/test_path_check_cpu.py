"""The oracle's traceback against an independent check of the path it returns (no GPU needed).

tests/path_check.py reads a record as a claim and prices it from the published objective: grammar, extents, bases,
score, and optimality against a score found another way.  "HIP == oracle" on CIGARs compares two tracebacks of one
design (five states, the preference d, E, F, E2, F2, extend on ties); this file is what stands behind the oracle's."""
import pytest

import paths_cases as PC
from path_check import PROPERTIES, PathError, check_path
from test_oracle_independent import _cases, general_gap_local

# ---- a path worked out by hand (default scheme: 2, 4, 4 + 2 l, 24 + l, N 1) -------------------------------------------
#   target  GG  A             B             CC  C             D              TT        (A .. D: 12 bases each)
#   query   c   A, C>A at 6   B lower case  --  C, G>N at 4   AAA  D         g
# D holds an N at its base 5 in both sequences (N against N: '=', scored -1).  From (qstart 1, tstart 2):
#   6= 1X 5=  |  12=  |  2D  |  4= 1X 7=  |  3I  |  12=       45 matches 90, N/N -1, mismatch -4, N/G -1,
#   2D -min(4 + 4, 24 + 2) = -8, 3I -min(4 + 6, 24 + 3) = -10:  66
_A, _B, _C, _D = "ACGTTGCAAGCT", "TAGGCTAACGTT", "GACCGGTATCGG", "ATCAANGCTTAA"
HAND_T = "GG" + _A + _B + "CC" + _C + _D + "TT"
HAND_Q = "c" + "ACGTTGAAAGCT" + _B.lower() + "GACCNGTATCGG" + "AAA" + _D + "g"
HAND = dict(score=66, cigar="6=1X17=2D4=1X7=3I12=", qstart=1, qend=52, tstart=2, tend=52)
HAND_SCHEME = PC.scheme_values({})

CORRUPTIONS = {
    "grammar": dict(cigar="6=1X17=2D4=1X7=3I6=6="),                       # two adjacent runs of one operation
    "extents": dict(qend=53),                                             # the walk ends one query base earlier
    "bases": dict(cigar="7=1X16=2D4=1X7=3I12="),                          # the X one column late: same extents
    "score": dict(score=68),
    # a shorter path that is right in itself: without 3I12= (12= is 11 matches and N/N, 21; 66 - 21 + 10)
    "optimality": dict(cigar="6=1X17=2D4=1X7=", qend=37, tend=40, score=55),
}


def test_hand_case_passes_and_is_optimal(oracle):
    assert (len(HAND_Q), len(HAND_T)) == (53, 54)
    d = HAND_SCHEME
    # (that DP compares bytes: it gets the query in one case)
    want = general_gap_local(HAND_Q.upper(), HAND_T, d["match"], d["mismatch"], d["gap_open1"], d["gap_ext1"], d["gap_open2"],
                             d["gap_ext2"], d["sc_ambi"])
    assert want[0] == 66 and HAND["tend"] in want[1]
    check_path(HAND_Q, HAND_T, HAND, HAND_SCHEME, optimum=want[0])
    check_path(HAND_Q, HAND_T, HAND, oracle.default_scoring(min_dp_score=0), optimum=want[0])     # a ctypes Scoring as well
    o = oracle.align_cigar(HAND_Q, HAND_T, oracle.default_scoring(min_dp_score=0))
    check_path(HAND_Q, HAND_T, o, HAND_SCHEME, optimum=66)
    assert {k: o[k] for k in HAND if k != "cigar"} == {k: v for k, v in HAND.items() if k != "cigar"}


@pytest.mark.parametrize("prop", PROPERTIES)
def test_each_corruption_fails_for_its_own_reason(prop):
    assert set(CORRUPTIONS) == set(PROPERTIES)
    bad = dict(HAND, **CORRUPTIONS[prop])
    with pytest.raises(PathError) as e:
        check_path(HAND_Q, HAND_T, bad, HAND_SCHEME, optimum=66)
    assert e.value.prop == prop and str(e.value).startswith(prop + ":"), str(e.value)
    if prop != "optimality":                                   # the shorter path is a path: only its score falls short
        with pytest.raises(PathError):
            check_path(HAND_Q, HAND_T, bad, HAND_SCHEME)
    else:
        check_path(HAND_Q, HAND_T, bad, HAND_SCHEME)


@pytest.mark.parametrize("cigar", ["", "12", "=12", "0=3X", "03=", "5M", "3=2S", "3= 2X", "2I3=", "3=2D", "3=2N1="])
def test_grammar_rejects(cigar):
    with pytest.raises(PathError) as e:
        check_path("ACGTA", "ACGTA", dict(score=0, cigar=cigar, qstart=0, qend=0, tstart=0, tend=0), HAND_SCHEME)
    assert e.value.prop == "grammar"


def test_oracle_paths_on_the_independent_cases(oracle):
    """Every case of test_oracle_independent: the path re-scores to its score, and the score is the optimum of the
    general-gap-cost DP, which has no gap states and no traceback."""
    n_paths = 0
    for q, t, (a, b, go1, ge1, go2, ge2, amb) in _cases():
        v = dict(match=a, mismatch=b, gap_open1=go1, gap_ext1=ge1, gap_open2=go2, gap_ext2=ge2, sc_ambi=amb, min_dp_score=0)
        want = general_gap_local(q, t, a, b, go1, ge1, go2, ge2, amb)[0]
        r = oracle.align_cigar(q, t, oracle.default_scoring(**v)) if q and t else dict(score=0, cigar="")
        if r["score"] < 1:
            assert want < 1 and r["cigar"] == "", (q, t, v, r, want)
            continue
        try:
            check_path(q, t, r, v, optimum=want)
        except PathError as e:
            raise AssertionError((str(e), q, t, v, r)) from e
        n_paths += 1
    assert n_paths >= 280


def _check_under_oracle(oracle, pairs, over):
    sc = oracle.default_scoring(**PC.scheme_values(over))
    out = []
    for p in pairs:
        r = oracle.align_cigar(p["q"], p["t"], sc)
        assert r["score"] >= 1, p["name"]                              # the record threshold: max(1, min_dp_score)
        try:
            check_path(p["q"], p["t"], r, PC.scheme_values(over), optimum=oracle.align(p["q"], p["t"], sc)[0])
        except PathError as e:
            raise AssertionError((p["name"], str(e), r)) from e
        out.append(r)
    return out


def test_scheme_table(oracle):
    names = [n for n, _ in PC.SCHEMES]
    assert len(names) == len(set(names)) >= 9
    d = oracle.default_scoring()
    assert {k: getattr(d, k) for k in PC.DEFAULT_SCHEME if k != "min_dp_score"} == \
           {k: v for k, v in PC.DEFAULT_SCHEME.items() if k != "min_dp_score"}
    for _, over in PC.SCHEMES:
        v = PC.scheme_values(over)
        assert PC.scheme_in_range(v) and v["min_dp_score"] == 0, v
    knees = {n: PC.knee_of(PC.scheme_values(o)) for n, o in PC.SCHEMES}
    assert knees["default"] == 20 and knees["knee16"] == 16 and knees["pieces_swapped"] == 26


@pytest.mark.parametrize("name,over", PC.SCHEMES, ids=[n for n, _ in PC.SCHEMES])
def test_oracle_paths_under_every_scheme(oracle, name, over):
    """The repeat panel and the gaps around the knee: every pair gives a record whose path passes the check."""
    panel, knee = PC.repeat_panel(over), PC.knee_pairs(over)
    assert len(panel) >= 90 and len(knee) == 8
    _check_under_oracle(oracle, panel, over)
    got = _check_under_oracle(oracle, knee, over)
    if name == "default":                                      # the planted gap is the gap of the path, either side of l = 20
        assert [p["planted"] for p in knee] == ["19I", "19D", "20I", "20D", "21I", "21D", "22I", "22D"]
        for p, r in zip(knee, got):
            assert p["planted"] in r["cigar"], (p["name"], r["cigar"])


def test_oracle_paths_on_the_shape_cases(oracle):
    """The pairs the GPU tests feed the kernel forms with: each gives a record under the oracle, and the path passes."""
    plain, with_n = PC.class_border_pairs()
    assert len(plain) == 48 and len(with_n) == 47 and {p["R"] for p in plain} == set(PC.r_list())
    assert all("N" in p["q"] for p in with_n) and not any(PC.has_n(p) for p in plain)
    _check_under_oracle(oracle, plain + with_n, {})
    _check_under_oracle(oracle, PC.target_edge_pairs(), {})
    for p, r in zip(PC.score_border_pairs(), _check_under_oracle(oracle, PC.score_border_pairs(), dict(match=64))):
        assert r["score"] == p["score"], p["name"]
    for rows in PC.TRACE_BLOCK_ROWS:
        for p, r in zip(PC.best_cell_tie_pairs(rows), _check_under_oracle(oracle, PC.best_cell_tie_pairs(rows), {})):
            assert r["score"] == p["score"] == 80, p["name"]
        for wide, nb in [(False, 2)] + sorted({(True, 2), (True, max(2, -(-496 // rows)))}):
            pairs = PC.row_block_pairs(rows, wide, nb)
            for p, r in zip(pairs, _check_under_oracle(oracle, pairs, dict(match=64) if wide else {})):
                assert r["qstart"] < p["seam"] < r["qend"], (p["name"], r["qstart"], r["qend"])
                assert p["planted"] is None or p["planted"] in r["cigar"], (p["name"], r["cigar"])


def test_oracle_paths_on_the_long_targets(oracle):
    pairs = PC.long_target_pairs()
    for p, r in zip(pairs, _check_under_oracle(oracle, pairs, {})):
        assert (r["tstart"], r["tend"]) == (p["tstart"], p["tend"]), p["name"]
    assert sum(p["tstart"] > 32767 for p in pairs) == 2
