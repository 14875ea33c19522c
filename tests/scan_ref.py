"""The repeat scan's contract (include/nanorepeat_amd.h) restated twice: scan_loops in plain
Python loops over strings, scan_numpy with arrays.  Both return (runs, stats): runs = a list of
(read, start, end, class, windows, fwd_windows) in the order of the result, stats = dict(n_windows, n_periodic,
n_segments).  tests/test_scan_cpu.py holds the two equal; the GPU tests compare nra_scan_repeats with them."""
import numpy as np

TILE = 4096          # window positions per workgroup: a segment never crosses a multiple of it
MAX_ROOT = 6
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def class_offset(p):
    return (4 ** p - 4) // 3


def word_value(word):
    v = 0
    for c in word:
        v = v * 4 + "ACGT".index(c)
    return v


def classify_word(word):
    """(class id, forward) of a primitive word of 1..6 upper-case bases."""
    p = len(word)
    own = [word[i:] + word[:i] for i in range(p)]
    rc = revcomp(word)
    other = [rc[i:] + rc[:i] for i in range(p)]
    canon = min(own + other)
    return class_offset(p) + word_value(canon), canon in own


def window_class(w):
    """w: a k-window as a string.  None if it is not valid or not periodic, else (class id, forward)."""
    w = w.upper()
    if any(c not in "ACGT" for c in w):
        return None
    k = len(w)
    for q in range(1, MAX_ROOT + 1):
        if all(w[i] == w[i + q] for i in range(k - q)):
            return classify_word(w[:q])
    return None


def islands_of(positions, k, max_gap):
    """positions: ascending (position, forward) of one class in one read -> [(start, end, windows, fwd_windows)]."""
    out = []
    for pos, fwd in positions:
        if out and pos - out[-1][4] <= max_gap:
            start, _, n, nf, _ = out[-1]
            out[-1] = (start, pos + k, n + 1, nf + int(fwd), pos)
        else:
            out.append((pos, pos + k, 1, int(fwd), pos))
    return [o[:4] for o in out]


def scan_loops(reads, k, max_gap, min_span):
    runs = []
    stats = dict(n_windows=0, n_periodic=0, n_segments=0)
    seen = {}
    for r, read in enumerate(reads):
        by_class = {}
        prev = None
        for i in range(len(read) - k + 1):
            w = read[i:i + k].upper()
            if w not in seen:
                seen[w] = (all(c in "ACGT" for c in w), window_class(w))
            valid, wc = seen[w]
            stats["n_windows"] += int(valid)
            if wc is None:
                prev = None
                continue
            stats["n_periodic"] += 1
            by_class.setdefault(wc[0], []).append((i, wc[1]))
            if prev != wc or i % TILE == 0:
                stats["n_segments"] += 1
            prev = wc
        mine = []
        for cid, positions in by_class.items():
            for start, end, n, nf in islands_of(positions, k, max_gap):
                if end - start >= min_span:
                    mine.append((r, start, end, cid, n, nf))
        runs.extend(sorted(mine))
    return runs, stats


def _word_table():
    """per period p: arrays over the 4^p words of (class id, reverse); -1 for a word that is not primitive."""
    tabs = {}
    for p in range(1, MAX_ROOT + 1):
        cid = np.full(4 ** p, -1, np.int64)
        rev = np.zeros(4 ** p, np.int64)
        for v in range(4 ** p):
            word = "".join("ACGT"[(v >> (2 * (p - 1 - j))) & 3] for j in range(p))
            if any(word == word[i:] + word[:i] for i in range(1, p)):
                continue
            c, fwd = classify_word(word)
            cid[v], rev[v] = c, 0 if fwd else 1
        tabs[p] = (cid, rev)
    return tabs


_TABS = None
_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def read_windows(read, k):
    """Per window position of one read: (valid, class id or -1, reverse) as arrays."""
    global _TABS
    if _TABS is None:
        _TABS = _word_table()
    raw = read.encode() if isinstance(read, str) else bytes(read)
    n_win = len(raw) - k + 1
    if n_win <= 0:
        z = np.zeros(0, np.int64)
        return z.astype(bool), z, z
    code = _CODE[np.frombuffer(raw, np.uint8)]
    bad = np.concatenate([[0], np.cumsum(code > 3)])
    valid = bad[k:] - bad[:-k] == 0
    cid = np.full(n_win, -1, np.int64)
    rev = np.zeros(n_win, np.int64)
    for q in range(MAX_ROOT, 0, -1):                    # the smallest period is written last
        ne = np.concatenate([[0], np.cumsum(code[:-q] != code[q:])])
        has = valid & (ne[k - q:k - q + n_win] - ne[:n_win] == 0)
        value = np.zeros(n_win, np.int64)
        for j in range(q):
            value = value * 4 + np.minimum(code[j:j + n_win], 3)
        c, v = _TABS[q]
        cid = np.where(has, c[value], cid)
        rev = np.where(has, v[value], rev)
    return valid, cid, rev


def scan_numpy(reads, k, max_gap, min_span):
    runs = []
    stats = dict(n_windows=0, n_periodic=0, n_segments=0)
    for r, read in enumerate(reads):
        valid, cid, rev = read_windows(read, k)
        stats["n_windows"] += int(valid.sum())
        pos = np.flatnonzero(cid >= 0)
        if not len(pos):
            continue
        stats["n_periodic"] += len(pos)
        entry = np.where(cid >= 0, cid * 2 + rev, -1)
        first = np.ones(len(entry), bool)
        first[1:] = entry[1:] != entry[:-1]
        first[::TILE] = True
        stats["n_segments"] += int((first & (entry >= 0)).sum())
        order = np.lexsort((pos, cid[pos]))
        pos = pos[order]
        c = cid[pos]
        cut = np.ones(len(pos), bool)
        cut[1:] = (c[1:] != c[:-1]) | (pos[1:] - pos[:-1] > max_gap)
        head = np.flatnonzero(cut)
        tail = np.concatenate([head[1:], [len(pos)]]) - 1
        fwd = np.concatenate([[0], np.cumsum(1 - rev[pos])])
        mine = [(r, int(pos[h]), int(pos[t]) + k, int(c[h]), int(t - h + 1), int(fwd[t + 1] - fwd[h]))
                for h, t in zip(head, tail) if pos[t] + k - pos[h] >= min_span]
        runs.extend(sorted(mine))
    return runs, stats


def scan(reads, k, max_gap, min_span):
    """The restatement the GPU tests compare with (the array form: the two are held equal on the CPU)."""
    return scan_numpy(reads, k, max_gap, min_span)
