"""CPU restatements of the anchor screen's contract, for the tests only.

`RefScreen` is the numpy restatement, with the constructor and `screen_reads` of nanorepeat_amd.screen.Screen, so
that it can stand in for it (`screener=`).  `plain_screen` says the same with Python sets and loops, to check the
numpy one on small cases."""
import numpy as np

_LUT = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _LUT[_c + 32] = _i


def _as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _all_true(flags, width):
    """For every start i: flags[i:i + width] all true."""
    c = np.r_[0, np.cumsum(~flags)]
    return (c[width:] - c[:-width]) == 0


def _windows(seqs, k, periodic=False):
    """Valid windows of many sequences: (owner, canonical code, periodic flag or None), rolled without materialising
    the windows."""
    # one byte that is not a base after every sequence: no window crosses into the next one
    blob = b"".join(_as_bytes(s) + b"\x00" for s in seqs)
    codes = _LUT[np.frombuffer(blob, np.uint8)]
    n = len(codes) - k + 1
    if n <= 0:
        e = np.zeros(0, np.int64)
        return e, e, (np.zeros(0, bool) if periodic else None)
    bad = codes == 255
    valid = _all_true(~bad, k)
    c = np.where(bad, 0, codes).astype(np.int64)
    fwd = np.zeros(n, np.int64)
    rev = np.zeros(n, np.int64)
    for j in range(k):
        fwd = fwd * 4 + c[j:j + n]
        rev += (3 - c[j:j + n]) << (2 * j)
    lens = np.array([len(_as_bytes(s)) + 1 for s in seqs], np.int64)
    owner = np.repeat(np.arange(len(seqs)), lens)[:n][valid]
    per = None
    if periodic:                     # w[i] == w[i + p] for all i, some p in 1..6
        per = np.zeros(n, bool)
        for p in range(1, 7):
            per |= _all_true(c[:-p] == c[p:], k - p)[:n]
        per = per[valid]
    return owner, np.minimum(fwd, rev)[valid], per


class RefScreen:
    """numpy restatement of nra_screen_create / nra_screen_reads."""

    def __init__(self, anchors, k=15, max_occ=16, device=0):
        self.k, self.n_regions = k, len(anchors)
        owner, canon, per = _windows([a for pair in anchors for a in pair], k, periodic=True)
        self.n_masked_periodic = len(np.unique(canon[per]))
        pairs = np.unique(canon[~per] << 32 | owner[~per])           # (k-mer, set), each once
        keys, sets = pairs >> 32, pairs & 0xffffffff
        ukeys, first, occ = np.unique(keys, return_index=True, return_counts=True)
        masked = np.repeat(occ > max_occ, occ)
        self.set_size = np.bincount(sets[~masked], minlength=2 * self.n_regions)
        self.keys = ukeys[occ <= max_occ]
        self.first = np.r_[0, np.cumsum(occ[occ <= max_occ])][:-1]
        self.occ = occ[occ <= max_occ]
        self.postings = sets[~masked]
        self.n_masked_max_occ = int((occ > max_occ).sum())
        sz = self.set_size.reshape(-1, 2)
        self.empty = np.flatnonzero((sz == 0).all(1))

    def stats(self):
        return dict(n_keys=len(self.keys), n_postings=len(self.postings), n_masked_periodic=self.n_masked_periodic,
                    n_masked_max_occ=self.n_masked_max_occ, n_empty_regions=len(self.empty))

    def hits(self, seqs):
        """{(read, set): count} as parallel arrays (read, set, count)."""
        owner, canon, _ = _windows(seqs, self.k)
        idx = np.searchsorted(self.keys, canon)
        found = idx < len(self.keys)
        found[found] = self.keys[idx[found]] == canon[found]
        idx, owner = idx[found], owner[found]
        cnt = self.occ[idx]
        total = int(cnt.sum())
        starts = np.repeat(self.first[idx] - (np.cumsum(cnt) - cnt), cnt)
        sets = self.postings[np.arange(total) + starts]
        key, c = np.unique(np.repeat(owner, cnt) * (2 * self.n_regions) + sets, return_counts=True)
        return key // (2 * self.n_regions), key % (2 * self.n_regions), c

    def screen_reads(self, seqs, min_hits=4):
        read, sets, c = self.hits(seqs)
        rg = read * self.n_regions + sets // 2
        u, inv = np.unique(rg, return_inverse=True)
        hl = np.zeros(len(u), np.int64)
        hr = np.zeros(len(u), np.int64)
        np.add.at(hl, inv[sets % 2 == 0], c[sets % 2 == 0])
        np.add.at(hr, inv[sets % 2 == 1], c[sets % 2 == 1])
        need = np.minimum(min_hits, self.set_size).reshape(-1, 2)
        g = u % self.n_regions
        ok = (hl >= need[g, 0]) & (hr >= need[g, 1])
        u, hl, hr = u[ok], hl[ok], hr[ok]
        if len(self.empty):
            e = (np.arange(len(seqs))[:, None] * self.n_regions + self.empty[None, :]).ravel()
            u = np.r_[u, e]; hl = np.r_[hl, np.zeros(len(e), np.int64)]; hr = np.r_[hr, np.zeros(len(e), np.int64)]
            o = np.argsort(u, kind="stable")
            u, hl, hr = u[o], hl[o], hr[o]
        return dict(read=(u // self.n_regions).astype(np.int32), region=(u % self.n_regions).astype(np.int32),
                    hits_left=hl.astype(np.int32), hits_right=hr.astype(np.int32))

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


# ----------------------------------------------------------------------------------- plain Python
_CODE = {c: i for i, c in enumerate("ACGT")}


def _plain_windows(seq, k):
    """(position, canonical k-mer, window string) of the valid windows."""
    s = seq.decode() if isinstance(seq, bytes) else seq
    out = []
    for i in range(len(s) - k + 1):
        w = s[i:i + k]
        if all(ch in "ACGTacgt" for ch in w):
            w = w.upper()
            f = 0
            r = 0
            for j, ch in enumerate(w):
                f = f * 4 + _CODE[ch]
                r += (3 - _CODE[ch]) * 4 ** j
            out.append((i, min(f, r), w))
    return out


def plain_screen(anchors, seqs, k, max_occ, min_hits):
    """The contract word for word: [(read, region, c_left, c_right)] sorted by read, then region."""
    sets = []
    for pair in anchors:
        for a in pair:
            sets.append({c for _, c, w in _plain_windows(a, k)
                         if not any(all(w[i] == w[i + p] for i in range(k - p)) for p in range(1, 7))})
    occ = {}
    for st in sets:
        for c in st:
            occ[c] = occ.get(c, 0) + 1
    sets = [{c for c in st if occ[c] <= max_occ} for st in sets]
    out = []
    for r, seq in enumerate(seqs):
        wins = [c for _, c, _ in _plain_windows(seq, k)]
        for g in range(len(anchors)):
            cl = sum(c in sets[2 * g] for c in wins)
            cr = sum(c in sets[2 * g + 1] for c in wins)
            if cl >= min(min_hits, len(sets[2 * g])) and cr >= min(min_hits, len(sets[2 * g + 1])):
                out.append((r, g, cl, cr))
    return out


def as_tuples(d):
    return list(zip(d["read"].tolist(), d["region"].tolist(), d["hits_left"].tolist(), d["hits_right"].tolist()))
