"""Seeded motif sets and tracts for the motif-run tests (test_segments_cpu.py, test_segments_gpu.py)."""
import numpy as np

from nanorepeat_amd import synth


def rand_set(rng, n_states=None, n_motifs=None):
    """A motif set of `n_states` states in all (default 1..32) in `n_motifs` motifs (default random, <= 8); now and
    then a motif is a one-base variant of another one, or shares a long prefix with it."""
    S = int(rng.integers(1, 33)) if n_states is None else n_states
    M = int(rng.integers(1, min(8, S) + 1)) if n_motifs is None else n_motifs
    cuts = np.sort(rng.choice(np.arange(1, S), M - 1, replace=False)) if M > 1 else np.zeros(0, np.int64)
    lens = np.diff(np.r_[0, cuts, S]).tolist()
    out = []
    for p in lens:
        same = [u for u in out if len(u) == p]
        if same and rng.random() < 0.5:                       # a variant of an earlier motif: one base changed
            u = list(same[int(rng.integers(0, len(same)))])
            at = int(rng.integers(0, p))
            u[at] = "ACGT"[("ACGT".index(u[at]) + int(rng.integers(1, 4))) % 4]
            u = "".join(u)
        elif out and rng.random() < 0.3:                      # shares a prefix with an earlier motif
            v = out[int(rng.integers(0, len(out)))]
            u = (v * (p // len(v) + 1))[:max(1, p - 1)]
            u = (u + synth.rand_seq(rng, p))[:p]
        else:
            u = synth.rand_seq(rng, p)
        out.append(u)
    return out


KINDS = ("runs", "runs_hifi", "runs_ont", "random", "other_bytes", "lower")


def rand_tract(rng, motifs, length, kind="runs_ont"):
    """A tract of about `length` bases: runs of the set's motifs, through an error channel, or random sequence."""
    if length == 0:
        return ""
    if kind == "random":
        return synth.rand_seq(rng, length)
    parts, total = [], 0
    while total < length:
        u = motifs[int(rng.integers(0, len(motifs)))]
        k = int(rng.integers(1, max(2, length // (2 * len(u)) + 1)))
        phase = int(rng.integers(0, len(u)))
        parts.append((u * (k + 1))[phase:phase + k * len(u)])
        total += len(parts[-1])
    s = "".join(parts)[:length]
    if kind in ("runs_hifi", "lower"):
        s = synth.apply_errors(rng, s, "hifi")
    elif kind in ("runs_ont", "other_bytes"):
        s = synth.apply_errors(rng, s, "ont")
    if kind == "other_bytes" and s:
        s = list(s)
        for _ in range(max(1, len(s) // 40)):
            s[int(rng.integers(0, len(s)))] = "NRY-"[int(rng.integers(0, 4))]
        s = "".join(s)
    if kind == "lower":
        s = s.lower() if rng.random() < 0.5 else s[:len(s) // 2].lower() + s[len(s) // 2:]
    return s


def seeded_case(n_tracts, seed, max_len=600, n_states=None, n_sets=None):
    """-> (sets, tracts, tract_set): `n_sets` random sets (default: one per four tracts), tracts of 0..max_len bases of
    every kind, in a shuffled order."""
    rng = np.random.default_rng(seed)
    n_sets = n_sets or max(1, n_tracts // 4)
    sets = [rand_set(rng, n_states=n_states) for q in range(n_sets)]
    tracts, ts = [], []
    for i in range(n_tracts):
        q = int(rng.integers(0, n_sets))
        n = 0 if i % 19 == 0 else int(rng.integers(1, max_len + 1))
        tracts.append(rand_tract(rng, sets[q], n, KINDS[i % len(KINDS)]))
        ts.append(q)
    return sets, tracts, np.array(ts, np.int32)
