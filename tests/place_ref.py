"""The placement contract (include/nanorepeat_amd.h) restated twice: candidates_loops in plain
Python loops over strings, candidates_numpy with arrays.  Both take the queries, the chunks [(contig, pos0, bases)] in
the order they are scanned, k, max_occ, bin, max_target_occ and min_votes, and return (candidates, stats): candidates =
a list of (query, contig, strand, bin, votes) in the order of the result, stats = a dict of the COUNTERS.
tests/test_place_cpu.py holds the two equal; the GPU tests compare nra_place_* with them.  Engine is the array form behind
the interface of _capi.place_*: the stand-in of place.py's tests without a GPU."""
import numpy as np

MAX_PERIOD = 6
CEILING = 1024                  # NRA_PLACE_OCC_CEILING
COUNTERS = ("n_keys", "n_postings", "n_masked_periodic", "n_masked_max_occ", "target_bases", "n_target_windows",
            "n_hits_kept", "n_keys_over", "n_chunks")
KEYS = ("query", "contig", "strand", "bin", "votes")
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


def windows_loops(seq, k):
    """(position, canon, forward, periodic) of every valid window of one sequence."""
    seq = seq.upper()
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if all(c in "ACGT" for c in w):
            code, rc = word_value(w), word_value(revcomp(w))
            yield i, min(code, rc), code < rc, is_periodic(w)


def candidates_loops(queries, chunks, k, max_occ, bin, max_target_occ, min_votes):
    postings, periodic = {}, set()
    for q, seq in enumerate(queries):
        for j, canon, f, per in windows_loops(seq, k):
            if per:
                periodic.add(canon)
            else:
                postings.setdefault(canon, []).append((q, j, f))
    masked = [c for c, p in postings.items() if len(p) > max_occ]
    for c in masked:
        del postings[c]
    stats = dict(n_keys=len(postings), n_postings=sum(len(p) for p in postings.values()),
                 n_masked_periodic=len(periodic), n_masked_max_occ=len(masked), target_bases=0, n_target_windows=0,
                 n_chunks=len(chunks))
    occ, windows = {}, []
    for t, pos0, bases in chunks:
        stats["target_bases"] += len(bases)
        for i, canon, g, _ in windows_loops(bases, k):
            stats["n_target_windows"] += 1
            occ[canon] = occ.get(canon, 0) + 1
            if canon in postings:
                windows.append((t, pos0 + i, g, canon))
    stats["n_hits_kept"] = sum(occ.get(c, 0) * len(p) for c, p in postings.items() if occ.get(c, 0) <= CEILING)
    stats["n_keys_over"] = sum(1 for c in postings if occ.get(c, 0) > max_target_occ)
    votes = {}
    for t, i, g, canon in windows:
        if occ[canon] > max_target_occ:
            continue
        for q, j, f in postings[canon]:
            s = 0 if f == g else 1
            d = i - j if s == 0 else i + j + k - len(queries[q])
            b = d // bin                            # Python's // floors towards minus infinity
            for vb in (b - 1, b):                   # floor(d / bin) in {vb, vb + 1}
                votes[(q, t, s, vb)] = votes.get((q, t, s, vb), 0) + 1
    return sorted(key + (v,) for key, v in votes.items() if v >= min_votes), stats


_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def windows_numpy(seq, k):
    """(positions, canon, forward, periodic) of the valid windows of one sequence, as arrays."""
    raw = seq.encode() if isinstance(seq, str) else bytes(seq)
    n_win = len(raw) - k + 1
    if n_win <= 0:
        z = np.zeros(0, np.int64)
        return z, z, z.astype(bool), z.astype(bool)
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
    at = np.flatnonzero(valid)
    return at, np.minimum(fwd, rev)[at], (fwd < rev)[at], periodic[at]


class Engine:
    """The array form behind the interface of _capi.place_create / _scan / _candidates / _stats / _destroy."""

    class Handle:
        pass

    def place_create(self, queries, k=15, max_occ=16, device=0):
        h = self.Handle()
        queries = list(queries)
        h.k = k
        h.qlen = np.array([len(s) for s in queries] + [0], np.int64)
        parts = [windows_numpy(s, k) for s in queries]
        q = np.concatenate([np.full(len(p[0]), i, np.int64) for i, p in enumerate(parts)] + [np.zeros(0, np.int64)])
        j, canon, f, per = (np.concatenate([p[x] for p in parts] + [np.zeros(0, parts[0][x].dtype if parts else np.int64)])
                            for x in range(4))
        per = per.astype(bool)
        keys, count = np.unique(canon[~per], return_counts=True)
        order = np.argsort(canon[~per], kind="stable")
        h.keys = keys[count <= max_occ]
        keep = np.isin(canon[~per][order], h.keys)
        h.post_key = np.searchsorted(h.keys, canon[~per][order][keep])      # ascending: the postings of key x are a slice
        h.post_q, h.post_j, h.post_f = (a[~per][order][keep] for a in (q, j, f.astype(bool)))
        h.first = np.searchsorted(h.post_key, np.arange(len(h.keys) + 1))
        h.occ = np.zeros(len(h.keys), np.int64)
        h.hits = []                                                         # (key index, contig, position, forward)
        h.stats = dict(n_keys=len(h.keys), n_postings=len(h.post_key), n_masked_periodic=len(np.unique(canon[per])),
                       n_masked_max_occ=int((count > max_occ).sum()), target_bases=0, n_target_windows=0, n_hits_kept=0,
                       n_keys_over=0, n_chunks=0)
        return h

    def place_scan(self, h, contig, pos0, bases):
        at, canon, g, _ = windows_numpy(bases, h.k)
        h.stats["target_bases"] += len(bases)
        h.stats["n_target_windows"] += len(at)
        h.stats["n_chunks"] += 1
        if len(h.keys):
            x = np.minimum(np.searchsorted(h.keys, canon), len(h.keys) - 1)
            hit = h.keys[x] == canon
            h.occ += np.bincount(x[hit], minlength=len(h.keys))
            h.hits.append((x[hit], np.full(int(hit.sum()), contig, np.int64), at[hit] + pos0, g[hit]))

    def place_candidates(self, h, bin=64, max_target_occ=64, min_votes=8, capacity=None):
        h.stats["n_keys_over"] = int((h.occ > max_target_occ).sum())
        n_post = np.diff(h.first)
        x, t, i, g = (np.concatenate([c[col] for c in h.hits] + [np.zeros(0, np.int64)]) for col in range(4))
        g = g.astype(bool)
        ok = h.occ[x] <= max_target_occ if len(x) else np.zeros(0, bool)
        x, t, i, g = x[ok], t[ok], i[ok], g[ok]
        rep = n_post[x]
        p = np.repeat(h.first[x], rep) + (np.arange(rep.sum()) - np.repeat(np.cumsum(rep) - rep, rep))
        t, i, g = np.repeat(t, rep), np.repeat(i, rep), np.repeat(g, rep)
        q, j, f = h.post_q[p], h.post_j[p], h.post_f[p]
        s = (f != g).astype(np.int64)
        d = np.where(s == 0, i - j, i + j + h.k - h.qlen[q])
        b = np.floor_divide(d, bin)
        rows = np.stack([np.concatenate([q, q]), np.concatenate([t, t]), np.concatenate([s, s]),
                         np.concatenate([b - 1, b])], axis=1)
        out = {key: np.zeros(0, np.int32) for key in KEYS}
        if len(rows):
            uniq, votes = np.unique(rows, axis=0, return_counts=True)       # rows in lexicographic order
            keep = votes >= min_votes
            out = {key: uniq[keep, c].astype(np.int32) for c, key in enumerate(KEYS[:4])}
            out["votes"] = votes[keep].astype(np.int32)
        return out

    def place_stats(self, h):
        n_post = np.diff(h.first)
        h.stats["n_hits_kept"] = int((h.occ * n_post)[h.occ <= CEILING].sum())
        return dict(h.stats, tile_windows=4096)

    def place_destroy(self, h):
        pass


def candidates_numpy(queries, chunks, k, max_occ, bin, max_target_occ, min_votes):
    e = Engine()
    h = e.place_create(queries, k, max_occ)
    for t, pos0, bases in chunks:
        e.place_scan(h, t, pos0, bases)
    got = e.place_candidates(h, bin, max_target_occ, min_votes)
    stats = e.place_stats(h)
    return list(zip(*(got[key].tolist() for key in KEYS))), {key: stats[key] for key in COUNTERS}


def candidates(queries, chunks, k, max_occ, bin, max_target_occ, min_votes):
    """The restatement the GPU tests compare with (the array form: the two are held equal on the CPU)."""
    return candidates_numpy(queries, chunks, k, max_occ, bin, max_target_occ, min_votes)
