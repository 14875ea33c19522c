"""Tracts shared by test_periods_cpu.py and test_periods_gpu.py: the lengths at the edges of the kernel's 32-base words
and of the two words a shifted word borrows, tracts of exactly p and p + 1 bases, bytes other than ACGT at the edges of
a word and of the tract and in a run longer than 64, lower case, and seeded short tracts of mixed lengths."""
import numpy as np

from nanorepeat_amd import synth

EDGE_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 2049)
MAX_PERIODS = (1, 6, 63, 64)


def _periodic(rng, n):
    p = int(rng.integers(1, 65))
    u = synth.rand_seq(rng, p)
    return (u * (n // p + 2))[int(rng.integers(0, p)):][:n]


def edge_tracts(seed=31):
    """Per edge length a random tract, a periodic one and a HiFi-noisy periodic one cut to the length."""
    rng = np.random.default_rng(seed)
    out = []
    for n in EDGE_LENGTHS:
        out += [synth.rand_seq(rng, n), _periodic(rng, n), synth.apply_errors(rng, _periodic(rng, n + 8), "hifi")[:n]]
    return out


def p_and_p_plus_one():
    """Tracts of exactly p and p + 1 bases for p = 1 and 64: no position, and one position, at lag p."""
    u = "ACGTTGCA" * 8
    return ["A", "AA", "AC", u, u + "A", u + "C"]


def non_acgt_tracts(seed=32):
    """N (and other bytes) at the first and last base of a word and of the tract, and runs of more than 64 of them."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (33, 64, 65, 130, 300):
        base = list(_periodic(rng, n))
        for at in (0, 31, 32, 63, 64, n - 1):
            if at < n:
                s = list(base)
                s[at] = "N"
                out.append("".join(s))
        s = list(base)
        for at in (0, 31, 32, 63, 64, n - 1):
            if at < n:
                s[at] = "nRY-*"[at % 5]
        out.append("".join(s))
    cag = "CAG" * 60
    out += [cag[:50] + "N" * 70 + cag[:90], "N" * 65 + cag, cag + "N" * 100, "N" * 200, "N", "NA", "AN" * 40]
    return out


def lower_case_tracts(seed=33):
    rng = np.random.default_rng(seed)
    s = _periodic(rng, 150)
    return [s.lower(), s[:70].lower() + s[70:], "".join(c.lower() if i % 3 else c for i, c in enumerate(s)), "acgtn" * 20]


def short_mixed(seed=34, count=300):
    """`count` short tracts of mixed lengths and kinds."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = 0 if i % 41 == 0 else int(rng.integers(1, 40)) if i % 5 == 2 else int(rng.integers(1, 700))
        kind = i % 4
        s = _periodic(rng, n) if kind == 0 else synth.rand_seq(rng, n) if kind == 1 else \
            synth.apply_errors(rng, _periodic(rng, n), "ont") if kind == 2 else \
            "".join(c if rng.random() > 0.03 else "N" for c in _periodic(rng, n))
        out.append(s)
    return out


def long_tracts(seed=35):
    """A 200 000-base homopolymer and a 200 000-base tract of a 64-mer."""
    rng = np.random.default_rng(seed)
    u = synth.primitive_unit(rng, 64)
    return ["A" * 200000, u * 3125]
