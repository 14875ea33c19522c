"""The sketch-pair contract (include/nanorepeat_amd.h) restated twice: pairs_loops in plain Python
loops over strings, pairs_numpy with arrays.  Both return (pairs, sketch_size, stats): pairs = a list of (a, b, shared)
in the order of the result, sketch_size = a list with one size per sequence, stats = dict(n_windows, n_kmers,
n_compared).  tests/test_loci_cpu.py holds the two equal; the GPU tests compare nra_sketch_pairs with them."""
import numpy as np

MAX_PERIOD = 6
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def word_value(word):
    v = 0
    for c in word:
        v = v * 4 + "ACGT".index(c)
    return v


def is_periodic(w):
    return any(all(w[i] == w[i + q] for i in range(len(w) - q)) for q in range(1, MAX_PERIOD + 1))


def sketch_loops(seq, k):
    """(the set of canonical codes, the number of valid windows) of one sequence."""
    seq = seq.upper()
    out, valid = set(), 0
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if any(c not in "ACGT" for c in w):
            continue
        valid += 1
        if not is_periodic(w):
            out.add(min(word_value(w), word_value(revcomp(w))))
    return out, valid


def pairs_loops(seqs, groups, k, min_shared):
    sketches, stats = [], dict(n_windows=0, n_kmers=0, n_compared=0)
    for s in seqs:
        sk, valid = sketch_loops(s, k)
        sketches.append(sk)
        stats["n_windows"] += valid
        stats["n_kmers"] += len(sk)
    pairs = []
    for a in range(len(seqs)):
        for b in range(a + 1, len(seqs)):
            if groups[a] < 0 or groups[a] != groups[b]:
                continue
            stats["n_compared"] += 1
            shared = len(sketches[a] & sketches[b])
            if shared >= min_shared:
                pairs.append((a, b, shared))
    return pairs, [len(sk) for sk in sketches], stats


_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def sketch_numpy(seq, k):
    """(the ascending array of canonical codes, the number of valid windows) of one sequence."""
    raw = seq.encode() if isinstance(seq, str) else bytes(seq)
    n_win = len(raw) - k + 1
    if n_win <= 0:
        return np.zeros(0, np.int64), 0
    code = _CODE[np.frombuffer(raw, np.uint8)]
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    valid = bad[k:] - bad[:-k] == 0
    periodic = np.zeros(n_win, bool)
    for q in range(1, MAX_PERIOD + 1):
        ne = np.concatenate([[0], np.cumsum(code[:-q] != code[q:])])
        periodic |= ne[k - q:k - q + n_win] - ne[:n_win] == 0
    c = np.minimum(code, 3)
    fwd = np.zeros(n_win, np.int64)
    rev = np.zeros(n_win, np.int64)
    for j in range(k):
        fwd = fwd * 4 + c[j:j + n_win]
        rev += (3 - c[j:j + n_win]) << (2 * j)
    return np.unique(np.minimum(fwd, rev)[valid & ~periodic]), int(valid.sum())


def pairs_numpy(seqs, groups, k, min_shared):
    groups = np.asarray(groups, np.int64)
    sketches, stats = [], dict(n_windows=0, n_kmers=0, n_compared=0)
    for s in seqs:
        sk, valid = sketch_numpy(s, k)
        sketches.append(sk)
        stats["n_windows"] += valid
        stats["n_kmers"] += len(sk)
    pairs = []
    for g in np.unique(groups[groups >= 0]):
        members = np.flatnonzero(groups == g)
        n = len(members)
        stats["n_compared"] += n * (n - 1) // 2
        sizes = np.array([len(sketches[m]) for m in members])
        every = np.concatenate([sketches[m] for m in members]) if n else np.zeros(0, np.int64)
        owner = np.repeat(np.arange(n), sizes)
        start = np.concatenate([[0], np.cumsum(sizes)])
        for x in range(n - 1):
            later = slice(start[x + 1], None)
            shared = np.bincount(owner[later][np.isin(every[later], sketches[members[x]], assume_unique=False)],
                                 minlength=n)
            for y in np.flatnonzero(shared >= min_shared):
                pairs.append((int(members[x]), int(members[y]), int(shared[y])))
    pairs.sort()
    return pairs, [len(sk) for sk in sketches], stats


def pairs(seqs, groups, k, min_shared):
    """The restatement the GPU tests compare with (the array form: the two are held equal on the CPU)."""
    return pairs_numpy(seqs, groups, k, min_shared)


def engine(seqs, groups, k=13, min_shared=1, device=0):
    """pairs() with the signature and the result of _capi.sketch_pairs: a stand-in for tests without a GPU."""
    got, sizes, stats = pairs(list(seqs), list(groups), k, min_shared)
    cols = list(zip(*got)) if got else [(), (), ()]
    out = {key: np.asarray(col, np.int32) for key, col in zip(("a", "b", "shared"), cols)}
    out["sketch_size"] = np.asarray(sizes, np.int32)
    out["stats"] = stats
    return out
