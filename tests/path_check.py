"""An independent check of one alignment record (score, CIGAR, extents) against the two sequences and the scoring.

Plain Python, no ctypes, and no code shared with oracle/ or with the kernels: no DP, no gap states, no traceback.  The
record is read as a claim -- "this path through these bases scores this much" -- and the claim is priced from the
published objective alone: the alignment definition of oracle/nr_oracle.h (bases compared without case, U as T, every
other byte one code N, N against N written '=' and scored -sc_ambi) and the gap cost of test_oracle_independent.py,
g(l) = min(gap_open1 + l * gap_ext1, gap_open2 + l * gap_ext2) per maximal run of I or of D.

check_path raises PathError, whose message begins with the name of the FIRST violated property, in this order:
grammar, extents, bases, score, optimality.
"""
import re

PROPERTIES = ("grammar", "extents", "bases", "score", "optimality")
SCORING_FIELDS = ("match", "mismatch", "gap_open1", "gap_ext1", "gap_open2", "gap_ext2", "sc_ambi", "min_dp_score")
_RUN = re.compile(r"([0-9]+)([A-Za-z=])")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


class PathError(AssertionError):
    def __init__(self, prop, text):
        assert prop in PROPERTIES
        super().__init__(f"{prop}: {text}")
        self.prop = prop


def scoring_values(scoring):
    """The eight scoring values of a mapping or of any object that has them as attributes."""
    if isinstance(scoring, dict):
        return {k: int(scoring[k]) for k in SCORING_FIELDS}
    return {k: int(getattr(scoring, k)) for k in SCORING_FIELDS}


def base_code(ch):
    return _CODE.get(ch.upper(), 4)


def gap_cost(l, sc):
    return min(sc["gap_open1"] + l * sc["gap_ext1"], sc["gap_open2"] + l * sc["gap_ext2"])


def parse_cigar(cigar):
    """[(n, op)] of a CIGAR that obeys the grammar; PathError("grammar") otherwise."""
    if not isinstance(cigar, str) or not cigar:
        raise PathError("grammar", f"empty CIGAR {cigar!r}")
    runs, at = [], 0
    for m in _RUN.finditer(cigar):
        if m.start() != at:
            break
        at = m.end()
        if m.group(1)[0] == "0":
            raise PathError("grammar", f"run {m.group(0)!r}: a length starts with 0")
        if m.group(2) not in "=XID":
            raise PathError("grammar", f"run {m.group(0)!r}: operation outside =XID")
        runs.append((int(m.group(1)), m.group(2)))
    if at != len(cigar):
        raise PathError("grammar", f"not a sequence of <n><op> at offset {at}: {cigar[at:at + 12]!r}")
    for k in range(1, len(runs)):
        if runs[k][1] == runs[k - 1][1]:
            raise PathError("grammar", f"adjacent runs {k - 1} and {k} are both {runs[k][1]!r}")
    if runs[0][1] not in "=X" or runs[-1][1] not in "=X":
        raise PathError("grammar", f"the path begins with {runs[0][1]!r} and ends with {runs[-1][1]!r}: both must be = or X")
    return runs


def check_path(q, t, result, scoring, optimum=None):
    """Raises PathError unless `result` (score, cigar, tstart, tend, qstart, qend) is a well-formed local alignment path
    of q (query) against t (target) that scores what it says under `scoring`, and `optimum` when that is given."""
    sc = scoring_values(scoring)
    score, qs, qe, ts, te = (int(result[k]) for k in ("score", "qstart", "qend", "tstart", "tend"))
    runs = parse_cigar(result["cigar"])

    if not (0 <= qs <= qe <= len(q) and 0 <= ts <= te <= len(t)):
        raise PathError("extents", f"query [{qs}, {qe}) of {len(q)}, target [{ts}, {te}) of {len(t)}")
    nq = sum(n for n, op in runs if op in "=XI")
    nt = sum(n for n, op in runs if op in "=XD")
    if (qs + nq, ts + nt) != (qe, te):
        raise PathError("extents", f"the walk from ({qs}, {ts}) ends at ({qs + nq}, {ts + nt}), the record at ({qe}, {te})")

    i, j, total = qs, ts, 0
    for n, op in runs:
        if op in "ID":
            total -= gap_cost(n, sc)
            if op == "I":
                i += n
            else:
                j += n
            continue
        for _ in range(n):
            a, b = base_code(q[i]), base_code(t[j])
            if (a == b) != (op == "="):
                raise PathError("bases", f"{op!r} at query {i} ({q[i]!r}) against target {j} ({t[j]!r})")
            total += -sc["sc_ambi"] if a == 4 or b == 4 else (sc["match"] if a == b else -sc["mismatch"])
            i += 1
            j += 1
    if total != score:
        raise PathError("score", f"the path scores {total}, the record says {score}")
    if optimum is not None and score != int(optimum):
        raise PathError("optimality", f"score {score}, optimum {int(optimum)}")
