"""CPU restatements of the motif screen's contract (include/nanorepeat_amd.h), for the tests only.

`RefScreenPartial` is the numpy restatement: tests/screen_ref.py's RefScreen with `motifs=` and
`screen_reads_partial`, so that it can stand in for nanorepeat_amd.screen.Screen (`screener=`).
`plain_screen_partial` says the same with Python strings, sets and loops, to check the numpy one on small cases."""
import numpy as np

from screen_ref import RefScreen, _LUT, _all_true, _as_bytes, _plain_windows

MAX_ROOT = 6
_COMP = str.maketrans("ACGT", "TGCA")


# ----------------------------------------------------------------------------------- classes (shared, plain Python)
def motif_root(motif):
    """The shortest word w with motif = w^j."""
    m = motif.upper()
    for p in range(1, len(m) + 1):
        if len(m) % p == 0 and m[:p] * (len(m) // p) == m:
            return m[:p]


def rotations(w):
    return {w[i:] + w[:i] for i in range(len(w))}


def class_members(root):
    """Every word of the class of `root`: its rotations and those of its reverse complement."""
    return rotations(root) | rotations(root.translate(_COMP)[::-1])


def classes_of(motifs):
    """-> (class_of per region, [member set per class]); classes are numbered in order of first appearance."""
    class_of, members = [], []
    for m in motifs:
        root = motif_root(m)
        if len(root) > MAX_ROOT:
            class_of.append(-1)
            continue
        for c, words in enumerate(members):
            if root in words:
                class_of.append(c)
                break
        else:
            class_of.append(len(members))
            members.append(class_members(root))
    return class_of, members


# ----------------------------------------------------------------------------------- numpy
def _code(word):
    v = 0
    for ch in word:
        v = v * 4 + "ACGT".index(ch)
    return v


def class_windows(seqs, k, members):
    """m(r, C) as an array [len(seqs), len(members)]."""
    m = np.zeros((len(seqs), len(members)), np.int64)
    if not members:
        return m
    blob = b"".join(_as_bytes(s) + b"\x00" for s in seqs)
    codes = _LUT[np.frombuffer(blob, np.uint8)]
    n = len(codes) - k + 1
    if n <= 0:
        return m
    bad = codes == 255
    valid = _all_true(~bad, k)
    c = np.where(bad, 0, codes).astype(np.int64)
    lens = np.array([len(_as_bytes(s)) + 1 for s in seqs], np.int64)
    owner = np.repeat(np.arange(len(seqs)), lens)[:n]
    undecided = valid.copy()
    for p in range(1, MAX_ROOT + 1):
        has_p = _all_true(c[:-p] == c[p:], k - p)[:n] & undecided     # the smallest period is p
        undecided &= ~has_p
        first = np.zeros(n, np.int64)                                # code of w[0:p]
        for j in range(p):
            first = first * 4 + c[j:j + n]
        table = np.full(4 ** p, -1, np.int64)
        for cl, words in enumerate(members):
            for w in words:
                if len(w) == p:
                    table[_code(w)] = cl
        cls = table[first[has_p]]
        np.add.at(m, (owner[has_p][cls >= 0], cls[cls >= 0]), 1)
    return m


class RefScreenPartial(RefScreen):
    """numpy restatement of nra_screen_set_motifs / nra_screen_reads_partial."""

    def __init__(self, anchors, k=15, max_occ=16, device=0, motifs=None):
        super().__init__(anchors, k=k, max_occ=max_occ, device=device)
        self.class_of, self.members = np.zeros(0, np.int64), []
        if motifs is not None:
            self.set_motifs(motifs)

    def set_motifs(self, motifs):
        assert len(motifs) == self.n_regions
        class_of, self.members = classes_of(motifs)
        self.class_of = np.array(class_of, np.int64)

    def stats(self):
        return dict(super().stats(), n_classes=len(self.members))

    def screen_reads_partial(self, seqs, min_hits=4, motif_share_pct=5):
        n, g = len(seqs), self.n_regions
        read, sets, c = self.hits(seqs)
        cnt = np.zeros((n, 2 * g), np.int64)
        cnt[read, sets] = c
        cl, cr = cnt[:, 0::2], cnt[:, 1::2]
        size = self.set_size.reshape(-1, 2)
        need = np.minimum(min_hits, size)
        ok_l, ok_r = cl >= need[:, 0], cr >= need[:, 1]              # nra_screen_reads' rule: an empty set passes
        pass_l, pass_r = ok_l & (size[:, 0] > 0), ok_r & (size[:, 1] > 0)
        kind0 = ok_l & ok_r
        kind1 = pass_l & (size[:, 1] > 0) & ~pass_r
        kind2 = pass_r & (size[:, 0] > 0) & ~pass_l
        m = class_windows(seqs, self.k, self.members)
        mw = np.zeros((n, g), np.int64)
        if len(self.members):
            has = self.class_of >= 0
            mw[:, has] = m[:, self.class_of[has]]
            has_class = np.broadcast_to(has, (n, g))
        else:
            has_class = np.zeros((n, g), bool)
        w = np.array([max(0, len(_as_bytes(s)) - self.k + 1) for s in seqs], np.int64)
        need_m = np.maximum(min_hits, -(-motif_share_pct * w // 100))
        kind3 = ~(kind0 | kind1 | kind2) & has_class & (w >= 1)[:, None] & (mw >= need_m[:, None])
        kind = np.full((n, g), 255, np.uint8)
        for v, mask in ((3, kind3), (2, kind2), (1, kind1), (0, kind0)):
            kind[mask] = v
        r, gg = np.nonzero(kind != 255)                               # row-major: by read, then region
        return dict(read=r.astype(np.int32), region=gg.astype(np.int32), hits_left=cl[r, gg].astype(np.int32),
                    hits_right=cr[r, gg].astype(np.int32), motif_windows=mw[r, gg].astype(np.int32), kind=kind[r, gg])


# ----------------------------------------------------------------------------------- plain Python
def plain_class_windows(seq, k, members):
    """[m(r, C) for every class C] of one read."""
    m = [0] * len(members)
    for _, _, w in _plain_windows(seq, k):
        for p in range(1, MAX_ROOT + 1):
            if all(w[i] == w[i + p] for i in range(k - p)):
                for c, words in enumerate(members):
                    if w[:p] in words:
                        m[c] += 1
                break
    return m


def plain_screen_partial(anchors, motifs, seqs, k, max_occ, min_hits, motif_share_pct):
    """The contract word for word: [(read, region, c_left, c_right, motif_windows, kind)] sorted by read, region."""
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
    class_of, members = classes_of(motifs) if motifs is not None else ([-1] * len(anchors), [])
    out = []
    for r, seq in enumerate(seqs):
        wins = [c for _, c, _ in _plain_windows(seq, k)]
        m = plain_class_windows(seq, k, members)
        n_pos = max(0, len(seq) - k + 1)
        for g in range(len(anchors)):
            left, right = sets[2 * g], sets[2 * g + 1]
            cl = sum(c in left for c in wins)
            cr = sum(c in right for c in wins)
            pass_l = len(left) > 0 and cl >= min(min_hits, len(left))
            pass_r = len(right) > 0 and cr >= min(min_hits, len(right))
            mw = m[class_of[g]] if class_of[g] >= 0 else 0
            if cl >= min(min_hits, len(left)) and cr >= min(min_hits, len(right)):
                kind = 0
            elif pass_l and len(right) > 0 and not pass_r:
                kind = 1
            elif pass_r and len(left) > 0 and not pass_l:
                kind = 2
            elif (class_of[g] >= 0 and n_pos >= 1
                  and mw >= max(min_hits, (motif_share_pct * n_pos + 99) // 100)):
                kind = 3
            else:
                continue
            out.append((r, g, cl, cr, mw, kind))
    return out


def as_tuples(d):
    return list(zip(*(d[key].tolist() for key in ("read", "region", "hits_left", "hits_right", "motif_windows", "kind"))))
