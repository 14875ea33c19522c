"""Discovered tandem runs grouped into loci by their flanking sequence.

discover.scan_reads says which reads carry a run of which motif class; this module says which of those runs are one
locus.  Every run has up to two sides (the flank_len bases before and behind it); all sides of a class go through
nra_sketch_pairs as one group, and two sides match when they are a returned pair.  The rules on top of the matches
(linking, attachment, open loci, the representative) are the functions below.  It writes
`<out_prefix>.discovered_loci.tsv`, `<out_prefix>.discovered_locus_runs.tsv` and, for the core loci with enough spanned
runs, `<out_prefix>.discovered_loci.fa` / `.bed`: a pseudo-reference and a BED file that pipeline.quantify_from_reads
takes unchanged.  No counterpart in the reference.
"""
import statistics
import sys

from . import discover

MIN_SHARED = 8             # the default min_shared at sketch_k = 13, flank_len = 500: measured, DESIGN.md section 30.4
ANCHOR = 1000              # bases of the representative's read kept on either side of its run in the pseudo-reference
MAX_GROUP = 65536          # sides of one class in one call (NRA_SKETCH_MAX_GROUP)
MAX_SIDE = 2048            # bases of a side (NRA_SKETCH_MAX_N)

LOCUS_COLUMNS = ("Locus", "Class", "Unit", "Type", "Runs", "Reads", "Spanned", "Left_Open", "Right_Open", "Min_Copies",
                 "Median_Copies", "Max_Copies", "Max_Open_Copies", "Rep_Read", "Rep_Start", "Rep_End", "Ref", "Ref_Start",
                 "Catalogued_Regions")
LOCUS_RUN_COLUMNS = ("Read_Name", "Start", "End", "Class", "Locus", "Role", "Links")
_COMP = str.maketrans("ACGT", "TGCA")


def check_options(flank_len, sketch_k, min_shared, min_locus_reads):
    """ValueError for a value the grouping cannot take; returns min_shared (the default for None)."""
    if min_shared is None:
        min_shared = MIN_SHARED
    if not isinstance(sketch_k, int) or sketch_k % 2 == 0 or not 11 <= sketch_k <= 15:
        raise ValueError(f"sketch_k must be odd and in 11..15, not {sketch_k!r}")
    if not isinstance(flank_len, int) or not sketch_k <= flank_len <= MAX_SIDE:
        raise ValueError(f"flank_len must be in sketch_k..{MAX_SIDE}, not {flank_len!r}")
    if not isinstance(min_shared, int) or min_shared < 1:
        raise ValueError(f"min_shared must be at least 1, not {min_shared!r}")
    if not isinstance(min_locus_reads, int) or min_locus_reads < 1:
        raise ValueError(f"min_locus_reads must be at least 1, not {min_locus_reads!r}")
    return min_shared


def self_complementary(word):
    """A class whose reverse complement is a rotation of itself (AT, ACGT, ...): its strand call carries nothing."""
    rc = word.translate(_COMP)[::-1]
    return any(rc == word[i:] + word[:i] for i in range(len(word)))


def run_sides(row, k):
    """{'U': sequence, 'D': sequence} of a run, oriented to its class's strand: a + run's left flank is its side U and
    its right flank its side D, a - run's are swapped (canonical k-mers make complementing unnecessary).  A left-open
    run has its right flank only, a right-open run its left flank only, an in-repeat run none; a flank of fewer than k
    bases is no side."""
    flanks = {"spanned": ("left_flank", "right_flank"), "left_open": (None, "right_flank"),
              "right_open": ("left_flank", None), "in_repeat": (None, None)}[row["kind"]]
    kinds = ("U", "D") if row["strand"] == "+" else ("D", "U")
    return {kind: row[key] for kind, key in zip(kinds, flanks) if key is not None and len(row[key]) >= k}


class _Components:
    def __init__(self):
        self.parent = {}

    def find(self, x):
        self.parent.setdefault(x, x)
        while self.parent[x] != x:
            self.parent[x] = self.parent[self.parent[x]]
            x = self.parent[x]
        return x

    def join(self, x, y):
        x, y = self.find(x), self.find(y)
        if x != y:
            self.parent[max(x, y)] = min(x, y)


def group_runs(rows, k=13, min_shared=MIN_SHARED, engine=None, device=0, max_group=MAX_GROUP):
    """rows: discover.scan_reads(..., flank_len > 0) in file order.  One engine call (`engine`: a stand-in for
    _capi.sketch_pairs(seqs, groups, k, min_shared, device)) for the sides of all classes, then the rules:

    1. two spanned runs of a class are linked when their U sides match and their D sides match (for a self-complementary
       class: under one of the two pairings); the components of the spanned runs are the core loci;
    2. an open run is attached to the one core locus that has a run whose comparable side (same kind; any side for a
       self-complementary class) matches its side; matching two or more core loci makes it ambiguous;
    3. the open runs that match no spanned run form open loci: the components of the matches among comparable sides;
    4. locus ids are 1.. in the order of each locus's first run;
    5. the representative is the run with the largest sum of `shared` over its links, the earliest on a tie.

    Returns dict(runs=[dict(locus: id or None, role, links)] per row, loci=[dict] by id, ungrouped=[class words over
    max_group sides], counts=dict(core, open, ambiguous, unplaced))."""
    if engine is None:
        from . import _capi
        engine = _capi.sketch_pairs
    n = len(rows)
    side_of = [run_sides(row, k) for row in rows]
    per_class = {}
    for r, sides in enumerate(side_of):
        per_class[rows[r]["class_id"]] = per_class.get(rows[r]["class_id"], 0) + len(sides)
    ungrouped = sorted(cid for cid, count in per_class.items() if count > max_group)
    seqs, groups, owner, index = [], [], [], [{} for _ in rows]       # owner: (run, kind) of a side
    for r, sides in enumerate(side_of):
        for kind in sorted(sides, reverse=True):                       # U, then D
            index[r][kind] = len(seqs)
            seqs.append(sides[kind])
            groups.append(-1 if rows[r]["class_id"] in ungrouped else rows[r]["class_id"])
            owner.append((r, kind))
    shared_of, partners = {}, [[] for _ in seqs]
    if seqs:
        got = engine(seqs, groups, k, min_shared, device)
        for a, b, s in zip(*(got[key].tolist() if hasattr(got[key], "tolist") else list(got[key])
                             for key in ("a", "b", "shared"))):
            shared_of[(a, b)] = s
            partners[a].append(b)
            partners[b].append(a)

    def shared(x, kx, y, ky):
        a, b = index[x].get(kx), index[y].get(ky)
        return 0 if a is None or b is None else shared_of.get((min(a, b), max(a, b)), 0)

    free = [self_complementary(row["cls"]) for row in rows]
    placed = [row["class_id"] not in ungrouped for row in rows]
    spanned = [placed[r] and rows[r]["kind"] == "spanned" and len(side_of[r]) == 2 for r in range(n)]
    is_open = [placed[r] and rows[r]["kind"] in ("left_open", "right_open") and len(side_of[r]) == 1 for r in range(n)]

    # rule 1
    core = _Components()
    links, link_sum = [0] * n, [0] * n
    candidates = {(min(owner[a][0], owner[b][0]), max(owner[a][0], owner[b][0])) for a, b in shared_of}
    for x, y in sorted(candidates):
        if x == y or not (spanned[x] and spanned[y]):
            continue
        both = [(shared(x, "U", y, "U"), shared(x, "D", y, "D"))]
        if free[x]:
            both.append((shared(x, "U", y, "D"), shared(x, "D", y, "U")))
        weight = max((u + d for u, d in both if u and d), default=0)
        if weight:
            core.join(x, y)
            for r in (x, y):
                links[r] += 1
                link_sum[r] += weight
    locus_of = [core.find(r) if spanned[r] else None for r in range(n)]      # a key for now, an id below
    role = ["core" if spanned[r] else "unplaced" for r in range(n)]

    # rule 2
    pool = []
    for r in range(n):
        if not is_open[r]:
            continue
        (kind, side), = index[r].items()
        matched = [owner[p] for p in partners[side] if spanned[owner[p][0]] and (free[r] or owner[p][1] == kind)]
        found = {core.find(y) for y, _ in matched}
        if len(found) == 1:
            locus_of[r], role[r], links[r] = found.pop(), "attached", len({y for y, _ in matched})
        elif found:
            role[r] = "ambiguous"
        else:
            pool.append(r)

    # rule 3
    in_pool = set(pool)
    opens = _Components()
    for r in pool:
        (kind, side), = index[r].items()
        role[r] = "open"
        locus_of[r] = ("open", opens.find(r))
        for p in partners[side]:
            y, other = owner[p]
            if y != r and y in in_pool and (free[r] or other == kind):
                opens.join(r, y)
                links[r] += 1
                link_sum[r] += shared_of[(min(side, p), max(side, p))]
    for r in pool:
        locus_of[r] = ("open", opens.find(r))

    # rules 4 and 5
    ids, loci = {}, []
    for r in range(n):
        key = locus_of[r]
        if key is None:
            continue
        if key not in ids:
            ids[key] = len(loci) + 1
            kind = next(iter(index[r])) if role[r] == "open" else None
            loci.append(dict(id=ids[key], type="core" if kind is None else f"open_{kind}", runs=[],
                             class_id=rows[r]["class_id"], cls=rows[r]["cls"]))
        loci[ids[key] - 1]["runs"].append(r)
    for locus in loci:
        mine = [r for r in locus["runs"] if role[r] in ("core", "open")]
        locus["rep"] = max(mine, key=lambda r: (link_sum[r], -r))
    runs = [dict(locus=ids.get(locus_of[r]), role=role[r], links=links[r]) for r in range(n)]
    counts = dict(core=sum(l["type"] == "core" for l in loci), open=sum(l["type"] != "core" for l in loci),
                  ambiguous=role.count("ambiguous"), unplaced=role.count("unplaced"))
    return dict(runs=runs, loci=loci, ungrouped=[discover.class_word(c) for c in ungrouped], counts=counts)


def locus_rows(rows, grouped, catalogue=None):
    """One summary row (a dict keyed by LOCUS_COLUMNS) per locus, by Max_Copies descending (loci without a spanned run
    last), then Locus.  The copies columns are over the spanned runs; Max_Open_Copies, over the open ones, is a lower
    bound."""
    out = []
    for locus in grouped["loci"]:
        mine = [rows[r] for r in locus["runs"]]
        rep = rows[locus["rep"]]
        spanned = [r["copies"] for r in mine if r["kind"] == "spanned"]
        opened = [r["copies"] for r in mine if r["kind"] != "spanned"]
        out.append({"Locus": locus["id"], "Class": locus["cls"], "Unit": rep["unit"], "Type": locus["type"],
                    "Runs": len(mine), "Reads": len({r["name"] for r in mine}), "Spanned": len(spanned),
                    "Left_Open": sum(r["kind"] == "left_open" for r in mine),
                    "Right_Open": sum(r["kind"] == "right_open" for r in mine),
                    "Min_Copies": min(spanned) if spanned else "-",
                    "Median_Copies": f"{statistics.median(spanned):g}" if spanned else "-",
                    "Max_Copies": max(spanned) if spanned else "-",
                    "Max_Open_Copies": max(opened) if opened else "-",
                    "Rep_Read": rep["name"], "Rep_Start": rep["start"], "Rep_End": rep["end"], "Ref": rep["ref"],
                    "Ref_Start": rep["ref_start"],
                    "Catalogued_Regions": "-" if catalogue is None else catalogue.get(locus["class_id"], 0)})
    out.sort(key=lambda c: (-c["Max_Copies"] if c["Max_Copies"] != "-" else 1, c["Locus"]))
    return out


def write_loci(table, path):
    with open(path, "w") as f:
        f.write("\t".join(LOCUS_COLUMNS) + "\n")
        for c in table:
            f.write("\t".join(str(c[col]) for col in LOCUS_COLUMNS) + "\n")


def write_locus_runs(rows, grouped, path):
    with open(path, "w") as f:
        f.write("\t".join(LOCUS_RUN_COLUMNS) + "\n")
        for row, run in zip(rows, grouped["runs"]):
            f.write("\t".join(str(x) for x in (row["name"], row["start"], row["end"], row["cls"],
                                               "-" if run["locus"] is None else run["locus"], run["role"],
                                               run["links"])) + "\n")


def reference_loci(rows, grouped, min_locus_reads=3):
    """The core loci with at least min_locus_reads spanned runs."""
    return [l for l in grouped["loci"] if l["type"] == "core" and
            sum(rows[r]["kind"] == "spanned" for r in l["runs"]) >= min_locus_reads]


def write_reference(rows, chosen, reads, fasta_path, bed_path, anchor=ANCHOR, wrap=80):
    """The pseudo-reference of the loci `chosen`: contig locus_<id> = the representative's read, as read, from `anchor`
    bases before its run to `anchor` bases behind it (cut at the read's ends), and the BED row locus_<id>, the left
    anchor actually cut, that + the run's span, the representative's unit.  reads: {read_index: (name, sequence)}."""
    with open(fasta_path, "w") as fa, open(bed_path, "w") as bed:
        for locus in chosen:
            rep = rows[locus["rep"]]
            seq = reads[rep["read_index"]][1]
            left = min(anchor, rep["start"])
            contig = seq[rep["start"] - left:rep["end"] + anchor]
            fa.write(f">locus_{locus['id']}\n" + "".join(contig[i:i + wrap] + "\n" for i in range(0, len(contig), wrap)))
            bed.write(f"locus_{locus['id']}\t{left}\t{left + rep['span']}\t{rep['unit']}\n")


def loci_files(reads_path, out_prefix, rows, catalogue=None, k=13, min_shared=MIN_SHARED, min_locus_reads=3,
               no_details=False, device=0, chunk_bases=1 << 28, engine=None, stream=None, max_group=MAX_GROUP):
    """group_runs of the rows -> `<out_prefix>.discovered_loci.tsv`, `.discovered_locus_runs.tsv` (not with no_details),
    `.discovered_loci.fa` and `.discovered_loci.bed`, one NOTICE counting the loci and the runs without one, and one
    NOTICE naming the classes left ungrouped.  Returns (the locus rows, the grouping)."""
    stream = stream or sys.stderr
    grouped = group_runs(rows, k, min_shared, engine, device, max_group)
    table = locus_rows(rows, grouped, catalogue)
    write_loci(table, f"{out_prefix}.discovered_loci.tsv")
    if not no_details:
        write_locus_runs(rows, grouped, f"{out_prefix}.discovered_locus_runs.tsv")
    chosen = reference_loci(rows, grouped, min_locus_reads)
    reads = discover.fetch_reads(reads_path, {rows[l["rep"]]["read_index"] for l in chosen}, chunk_bases)
    write_reference(rows, chosen, reads, f"{out_prefix}.discovered_loci.fa", f"{out_prefix}.discovered_loci.bed")
    c = grouped["counts"]
    print(f"NOTICE: the discovered runs form {c['core']} core locus/loci ({len(chosen)} with at least "
          f"{min_locus_reads} spanned runs) and {c['open']} open locus/loci; {c['ambiguous']} ambiguous and "
          f"{c['unplaced']} unplaced run(s) have no locus", file=stream)
    if grouped["ungrouped"]:
        print(f"NOTICE: class(es) {', '.join(grouped['ungrouped'])} have more than {max_group} sides and are left "
              f"ungrouped", file=stream)
    return table, grouped
