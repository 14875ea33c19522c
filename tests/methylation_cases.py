"""Seeded cases for the methylation tests: reads with CG pairs planted across every lane, wave and tile edge, lists of
every kind, a BAM writer that attaches tags, and the two-allele region of the command tests."""
import struct
import zlib

import numpy as np

from nanorepeat_amd import bam as B
from methylation_ref import sequenced_strand

LO_BYTE, HI_BYTE = 63, 192
EDGE_BYTES = (0, LO_BYTE, LO_BYTE + 1, HI_BYTE - 1, HI_BYTE, 255)
EDGE_LENGTHS = [0, 1, 2] + [(1 << k) + d for k in range(6, 14) for d in (-1, 0, 1)]
LIST_KINDS = ("empty", "all", "cpg", "random", "last", "beyond", "huge", "too_many")
# (flank, bin): nb = 10; a flank longer than any read; a bin that does not divide the flank; nb = 1; nb = 64
SHAPES = ((2000, 200), (100000, 2000), (1000, 300), (500, 500), (640, 10))


def rand_read(rng, n):
    """n bases of ACGT with some lower case and N, and CG planted across every multiple of 64 counted from either end."""
    s = rng.choice(list("ACGTacgtN"), size=n, p=[.2, .22, .22, .2, .04, .04, .04, .02, .02]).tolist() if n else []
    for e in range(64, n, 64):
        for at in (e - 1, n - 1 - e):
            if 0 <= at and at + 1 < n:
                s[at], s[at + 1] = ("C", "G") if (e // 64) % 3 else ("c", "g")
    return "".join(s)


def c_ranks(stored, rev):
    """(positions in O of its C, the ranks among them of the C of a CG pair of O)"""
    o = sequenced_strand(stored, rev)
    cs = [i for i, c in enumerate(o) if c == "C"]
    rank = {i: r for r, i in enumerate(cs)}
    return cs, [rank[i] for i in cs if i + 1 < len(o) and o[i + 1] == "G"]


def make_list(rng, stored, rev, kind):
    """(deltas int32, probs uint8) of one kind for the read."""
    cs, cpg = c_ranks(stored, rev)
    n_c = len(cs)
    if kind == "empty" or (n_c == 0 and kind in ("all", "cpg", "random", "last")):
        ranks = []
    elif kind == "all":
        ranks = list(range(n_c))                        # every C: zero deltas throughout
    elif kind == "cpg":
        ranks = cpg
    elif kind == "random":
        ranks = sorted(rng.choice(n_c, size=max(1, n_c // 3), replace=False).tolist())
    elif kind == "last":
        ranks = [n_c - 1]
    elif kind == "beyond":
        ranks = cpg[:3] + [n_c]                                                     # L_{m-1} = n_c exactly
    elif kind == "huge":
        ranks = [0, 1 << 30, 1 << 31, 3 << 30, (1 << 32) + 7]                       # the sum passes 2^31 and 2^32
    elif kind == "too_many":
        ranks = list(range(len(stored) + 1))                                        # m = n + 1
    else:
        raise ValueError(kind)
    deltas = np.diff(np.array([-1] + ranks, np.int64)) - 1
    probs = rng.choice(np.array(EDGE_BYTES * 40 + tuple(range(256)), np.uint8), size=len(ranks))    # half of them edge bytes
    return deltas.astype(np.int32), probs.astype(np.uint8)


def tract_for(rng, stored, which):
    """One of: empty at 0, empty inside, from index 0, to the end, the whole read, both edges inside a CG."""
    n = len(stored)
    up = stored.upper()
    sites = [s for s in range(n - 1) if up[s] == "C" and up[s + 1] == "G"]
    which %= 6
    if which == 0 or n == 0:
        return 0, 0
    if which == 1:
        return n // 2, n // 2
    if which == 2:
        return 0, max(1, n // 3)
    if which == 3:
        return 2 * n // 3, n
    if which == 4:
        return 0, n
    if len(sites) >= 2:
        a, b = sorted(rng.choice(len(sites), size=2, replace=False).tolist())
        return sites[a] + 1, sites[b] + 1
    return min(1, n), n


def edge_batch(seed=1, lengths=None):
    """Every length x (stored reversed, implicit) x a list kind and a tract that rotate: dict(reads, mods, flags, lo,
    hi), the arguments of _capi.read_methylation."""
    rng = np.random.default_rng(seed)
    reads, mods, flags, lo, hi = [], [], [], [], []
    k = 0
    for n in (EDGE_LENGTHS + [70001] if lengths is None else lengths):
        for bits in (0, 1, 2, 3):
            s = rand_read(rng, n)
            kind = LIST_KINDS[k % len(LIST_KINDS)]
            reads.append(s)
            mods.append(make_list(rng, s, bool(bits & 1), kind))
            flags.append(bits)
            a, b = tract_for(rng, s, k // 2)
            lo.append(a); hi.append(b)
            k += 3                                      # 3 is coprime to the 8 kinds and walks the tracts too
    return dict(reads=reads, mods=mods, flags=np.array(flags, np.uint8), lo=np.array(lo, np.int32),
                hi=np.array(hi, np.int32))


def kinds_batch(seed=2, n=777):
    """Every list kind x (stored reversed, implicit) on reads of one odd length, the tract in the middle."""
    rng = np.random.default_rng(seed)
    reads, mods, flags = [], [], []
    for kind in LIST_KINDS:
        for bits in (0, 1, 2, 3):
            s = rand_read(rng, n)
            reads.append(s); mods.append(make_list(rng, s, bool(bits & 1), kind)); flags.append(bits)
    # L_{m-1} = n_c - 1 (fine) next to n_c (BAD_TAG), on one read
    s = rand_read(rng, n)
    n_c = len(c_ranks(s, False)[0])
    for last in (n_c - 1, n_c):
        reads.append(s); flags.append(2)
        mods.append((np.array([3, last - 4], np.int32), np.array([HI_BYTE, LO_BYTE], np.uint8)))
    m = len(reads)
    return dict(reads=reads, mods=mods, flags=np.array(flags, np.uint8), lo=np.full(m, n // 3, np.int32),
                hi=np.full(m, 2 * n // 3, np.int32))


def take(batch, order):
    return dict(reads=[batch["reads"][i] for i in order], mods=[batch["mods"][i] for i in order],
                flags=batch["flags"][order], lo=batch["lo"][order], hi=batch["hi"][order])


def call(engine, batch, flank=2000, bin=200, **kw):
    return engine(batch["reads"], batch["mods"], batch["flags"], batch["lo"], batch["hi"], flank=flank, bin=bin,
                  lo_byte=LO_BYTE, hi_byte=HI_BYTE, **kw)


def mirrored(batch):
    """Every read as its reverse-complement record: the sequence reverse-complemented, bit 0 flipped, the tract
    mirrored, the same list."""
    comp = str.maketrans("ACGTacgt", "TGCAtgca")
    n = np.array([len(s) for s in batch["reads"]], np.int32)
    return dict(reads=[s.translate(comp)[::-1] for s in batch["reads"]], mods=batch["mods"], flags=batch["flags"] ^ 1,
                lo=n - batch["hi"], hi=n - batch["lo"])


def swap_sides(counts):
    """[reads][2 nb + 1][5] with before and after exchanged."""
    nb = (counts.shape[1] - 1) // 2
    return np.concatenate([counts[:, nb + 1:], counts[:, nb:nb + 1], counts[:, :nb]], axis=1)


# ---------------------------------------------------------------------------- tag text
def mm_text(deltas, code="m", flag="?", base="C"):
    return f"{base}+{code}{flag}" + "".join(f",{int(d)}" for d in deltas) + ";"


# ---------------------------------------------------------------------------- a BAM writer with tags
def _bgzf_block(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    bsize = 12 + 6 + len(data) + 8 - 1
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) +
            data + struct.pack("<II", zlib.crc32(payload), len(payload)))


def tag_bytes(key, typ, value):
    """One optional field.  typ: A c C s S i I f Z H, or ("B", subtype)."""
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
    head = key.encode()
    if isinstance(typ, tuple):
        sub = typ[1]
        return head + b"B" + sub.encode() + struct.pack("<i", len(value)) + b"".join(struct.pack(fmt[sub], v) for v in value)
    if typ == "A":
        return head + b"A" + value.encode()
    if typ in "ZH":
        return head + typ.encode() + value.encode() + b"\x00"
    return head + typ.encode() + struct.pack(fmt[typ], value)


def record(name, seq, tid, pos, ref_len, flag=0, tags=b"", hard_clip=0):
    cigar = ([(hard_clip << 4) | 5] if hard_clip else []) + [(ref_len << 4) | 0]
    codes = [B._SEQ_CODES.index(c) for c in seq.upper()] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 60, 0, len(cigar), flag, len(seq), -1, -1, 0)
    body += name.encode() + b"\x00" + b"".join(struct.pack("<I", c) for c in cigar) + packed + b"\xff" * len(seq) + tags
    return struct.pack("<i", len(body)) + body


def write_bam(path, refs, records, block=3000):
    """records: (name, seq, ref name, pos, end, flag, tag bytes, hard clip) sorted by (ref, pos); no index."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(f"@SQ\tSN:{n}\tLN:{l}\n".encode() for n, l in refs)
    raw = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in refs:
        raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", l)
    names = [n for n, _ in refs]
    for name, seq, ref, pos, end, flag, tags, clip in records:
        raw += record(name, seq, names.index(ref), pos, end - pos, flag, tags, clip)
    with open(path, "wb") as f:
        f.write(b"".join(_bgzf_block(raw[u:u + block]) for u in range(0, len(raw), block)) + _bgzf_block(b""))


# ---------------------------------------------------------------------------- the command case
def command_case(tmp_path, seed=5):
    """One CGG region with two alleles (10 and 30 units, 10 reads each, no read errors).  The reads of the long allele
    are methylated (byte 250) in the tract and the reference's left flank and not (byte 5) in the right flank; those of
    the short allele nowhere.  Records come in the four combinations of stored strand and sequenced strand; two reads in
    three list every CpG with `?`, the others list the methylated ones only with `.`, and every fifth carries a second
    modification (`C+mh`, m first).  Two more reads carry no tags and a hard clip.  Writes ref.fa, r.bed, in.bam and
    in.fastq (the reads as sequenced, tags in the header comments).  Returns {read name: allele units}."""
    from nanorepeat_amd import synth
    rng = np.random.default_rng(seed)
    left, right = synth.rand_seq(rng, 1500), synth.rand_seq(rng, 1500)
    chrom = left + "CGG" * 12 + right
    s1, e1 = len(left), len(left) + 36
    (tmp_path / "ref.fa").write_text(">chr7\n" + "\n".join(chrom[i:i + 80] for i in range(0, len(chrom), 80)) + "\n")
    (tmp_path / "r.bed").write_text(f"chr7\t{s1}\t{e1}\tCGG\n")
    recs, fastq, truth = [], [], {}
    for i in range(22):
        units = (10, 30)[i % 2]
        lo = s1 - 700 - 5 * i
        head = chrom[lo:s1]
        r = head + "CGG" * units + chrom[e1:e1 + 720]                   # the read in the reference's orientation
        tract_end = len(head) + 3 * units
        name = f"r{i:02d}"
        truth[name] = units
        stored_rc, sequenced_rc = bool(i & 2), bool(i & 4)
        stored = synth.revcomp(r) if stored_rc else r
        o = synth.revcomp(r) if sequenced_rc else r
        flag = 0x10 if stored_rc != sequenced_rc else 0
        explicit = i % 3 != 1
        # the CpG of O, by their position in r: methylated left of the tract's end on the long allele
        cs = [k for k, c in enumerate(o) if c == "C"]
        listed, probs = [], []
        for rank, k in enumerate(cs):
            if k + 1 < len(o) and o[k + 1] == "G":
                at = len(r) - 2 - k if sequenced_rc else k
                meth = units == 30 and at + 2 <= tract_end
                if meth or explicit:
                    listed.append(rank); probs.append(250 if meth else 5)
        deltas = np.diff(np.array([-1] + listed)) - 1
        two = i % 5 == 0
        text = mm_text(deltas, "mh" if two else "m", "?" if explicit else ".")
        ml = [b for p in probs for b in ((p, 1) if two else (p,))]
        if i == 20:
            tags, comment, clip = b"", "", 0                              # no tags at all
        else:
            clip = 7 if i == 21 else 0
            tags = (tag_bytes("NM", "i", 3) + tag_bytes("MM", "Z", text) + tag_bytes("ML", ("B", "C"), ml) +
                    tag_bytes("MN", "i", len(stored)))
            comment = f"\tMM:Z:{text}\tML:B:C,{','.join(map(str, ml))}\tMN:i:{len(o) + (3 if i == 21 else 0)}"
        recs.append((name, stored, "chr7", lo, e1 + 720, flag, tags, clip))
        fastq.append(f"@{name}{comment}\n{o}\n+\n{'5' * len(o)}\n")
    recs.sort(key=lambda t: t[3])
    write_bam(str(tmp_path / "in.bam"), [("chr7", len(chrom))], recs)
    (tmp_path / "in.fastq").write_text("".join(fastq))
    return truth
