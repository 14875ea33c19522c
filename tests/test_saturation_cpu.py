"""The premise of the saturation exit, on the CPU: once the DP column of a read at a unit boundary of
L + unit^k equals the column at the boundary before it -- H, the two horizontal gap states and the running maximum, each
with its origin bit --, the candidate's score and flank verdicts stop changing with k.  A numpy restatement of the column
recurrence (the oracle's dp_core, scores doubled, the low bit "the best path starts at a column >= |L|") finds the first
such boundary; the oracle aligns the read against L + unit^k + R for every later k.  This guards the premise, not the
kernel (tests/test_saturation_gpu.py does that)."""
import functools

import numpy as np
import pytest

from nanorepeat_amd import synth

NEG = -(1 << 40)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def encode(s):
    return np.array([CODE.get(c, 4) for c in s], np.int64)


class Columns:
    """The forward DP of one read, column by column, in packed values 2 * score + origin bit.  `step(tc, bit)` takes the
    next template column (its base code; bit: an alignment starting here starts at a column >= |L|)."""

    def __init__(self, read, sc):
        self.q = encode(read)
        n = len(self.q)
        self.sc = sc
        self.H = np.full(n, NEG, np.int64)
        self.E = np.full(n, NEG, np.int64)
        self.E2 = np.full(n, NEG, np.int64)
        self.M = 0
        self.rows = np.arange(n, dtype=np.int64)

    def step(self, tc, bit):
        sc, q = self.sc, self.q
        sub = np.where((q >= 4) | (tc >= 4), -sc.sc_ambi, np.where(q == tc, sc.match, -sc.mismatch)).astype(np.int64)
        diag = np.concatenate([[NEG], self.H[:-1]])
        h0 = np.maximum(np.maximum(np.maximum(diag, bit) + 2 * sub, self.E), self.E2)
        # the vertical gap states of this column: F(i) = max over i' < i of h(i') - open - ext * (i - 1 - i').  A gap opened
        # from a cell that a vertical gap produced is strictly worse than the longer gap it continues, so h0 serves for h
        h = h0
        for opn, ext in ((sc.gap_open1 + sc.gap_ext1, sc.gap_ext1), (sc.gap_open2 + sc.gap_ext2, sc.gap_ext2)):
            g = np.maximum.accumulate(h0 + 2 * ext * self.rows)
            f = np.concatenate([[NEG], g[:-1] - 2 * opn - 2 * ext * self.rows[:-1]])
            h = np.maximum(h, f)
        self.M = max(self.M, int(h.max()))
        self.H = h
        self.E = np.maximum(self.E - 2 * sc.gap_ext1, h - 2 * (sc.gap_open1 + sc.gap_ext1))
        self.E2 = np.maximum(self.E2 - 2 * sc.gap_ext2, h - 2 * (sc.gap_open2 + sc.gap_ext2))

    def state(self):
        return self.H.copy(), self.E.copy(), self.E2.copy(), self.M


def first_repeat(read, left, unit, kmax, sc):
    """The first k whose boundary column state equals that of k - 1, or None."""
    dp = Columns(read, sc)
    for c in encode(left[:-1]):
        dp.step(c, 0)
    dp.step(encode(left[-1:])[0], 0)
    prev = None
    u = encode(unit)
    for k in range(1, kmax + 1):
        for c in u:
            dp.step(c, 1)
        cur = dp.state()
        if prev is not None and cur[3] == prev[3] and all(np.array_equal(a, b) for a, b in zip(cur[:3], prev[:3])):
            return k
        prev = cur
    return None


def verdict(oracle, read, left, unit, right, k, sc):
    """(score, left flank reached, right flank reached) of the oracle's alignment against L + unit^k + R."""
    score, tstart, tend = oracle.align(read, left + unit * k + right, sc)
    return score, tstart < len(left), tend > len(left) + len(unit) * k


SHAPES = {"A": ("A", 150, 40), "AC": ("AC", 150, 40), "TATTG": ("TATTG", 150, 40), "8-mer": ("ACGGTCAT", 150, 40),
          "TATTG, anchors of 400": ("TATTG", 400, 60)}


@functools.lru_cache(maxsize=None)
def shape(name):
    unit, anchor, flank = SHAPES[name]
    rng = np.random.default_rng(7000 + 100 * len(unit) + anchor)
    left, right = synth.rand_seq(rng, anchor), synth.rand_seq(rng, anchor)
    reads = [synth.apply_errors(rng, left[anchor - flank:] + unit * 10 + right[:flank], "ont") for _ in range(6)]
    return left, unit, right, reads


def test_restatement_is_the_oracles_recurrence(oracle):
    """The packed column recurrence over the whole template gives the oracle's score and the origin bit of its tstart."""
    sc = oracle.default_scoring()
    left, unit, right, reads = shape("TATTG")
    for read in reads[:3]:
        for k in (3, 10, 40):
            dp = Columns(read, sc)
            for j, c in enumerate(encode(left + unit * k + right)):
                dp.step(c, int(j >= len(left)))
            score, tstart, _ = oracle.align(read, left + unit * k + right, sc)
            assert dp.M >> 1 == score and (dp.M & 1) == int(tstart >= len(left)), (k, dp.M, score, tstart)


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_repeated_boundary_state_fixes_every_later_candidate(oracle, name):
    sc = oracle.default_scoring()
    left, unit, right, reads = shape(name)
    kmax = 150
    found = []
    for read in reads:
        k0 = first_repeat(read, left, unit, kmax, sc)
        found.append(k0)
        if k0 is None:
            continue
        want = verdict(oracle, read, left, unit, right, k0, sc)
        for k in range(k0 + 1, kmax + 1):
            assert verdict(oracle, read, left, unit, right, k, sc) == want, (name, k0, k)
    print(name, "first repeated boundary per read:", found)
    # the allele has 10 units: the state cannot repeat before the read's tract is through, and on these shapes it does
    # long before k = 150 (the deletion that reaches back into L grows by a unit per boundary, the alternatives do not)
    assert all(k0 is not None and 10 < k0 < kmax for k0 in found), found
