"""Bootstrap confidence intervals for the allele sizes and the allele count of a region (`bootstrap=B`; DESIGN.md
section 24; no counterpart in the reference).  mixture.bootstrap runs the order search of B resamples of every
region's kept reads on the GPU; this module turns each replicate's model into its alleles the way
phasing.create_allele_list and remove_noisy_alleles do -- in numpy over all replicates of a region at once -- and writes
the statistics: per called allele the percentile interval of its size over the replicates that have the called number
of alleles, and per region how many replicates have that number.  Nothing is thresholded: the counts are printed.
1D problems only (the BAM and FASTQ commands); the joint command is not bootstrapped."""
import math

import numpy as np

from . import mixture as nr_mixture, phasing

HEADER = ("#Chrom\tStart\tEnd\tMotif\tAllele\tRepeat_Size\tNum_Reads\tCI_Low\tCI_High\tReplicates_Used\t"
          "Num_Replicates\tCount_Support\tCount_Distribution\n")
N_FIELDS = 13


def alleles_of_replicates(x, rep, ploidy, remove_noisy_reads):
    """x: the kept sizes [m] of a 1D problem, rep: its entry of mixture.bootstrap's result -> (count [B], sizes
    [B, C]): the number of alleles of every replicate (-1: not decided) and their sizes in the order of their
    component means, padded with -1.
    Per replicate this is phasing.create_allele_list on the resampled reads (labels by FittedMixture.predict's rule,
    empty components dropped, size = int(median + 0.5)), then with remove_noisy_reads phasing.remove_noisy_alleles:
    with more alleles than the ploidy, those whose reads times 1.5 do not exceed the reads of the ploidy-th largest go."""
    x = np.asarray(x, np.float64).reshape(-1)
    idx, order = rep["idx"], rep["order"]
    B, m = idx.shape
    C = max(1, rep["w"].shape[1])
    w, mu, var = (np.zeros((B, C)) for _ in range(3))
    w[:, :rep["w"].shape[1]] = rep["w"]
    mu[:, :rep["w"].shape[1]] = rep["mu"][:, :, 0]
    var[:, :rep["w"].shape[1]] = rep["var"][:, :, 0]
    decided = rep["status"] == nr_mixture.BOOT_DECIDED
    valid = np.arange(C)[None, :] < np.maximum(order, 1)[:, None]
    xs = x[idx]                                                          # [B, m]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.log(w) - 0.5 * (math.log(2 * math.pi) + np.log(var))
        e = xs[:, :, None] - mu[:, None, :]
        lj = a[:, None, :] - 0.5 * (e * e / var[:, None, :])
    lj = np.where(valid[:, None, :], lj, -np.inf)
    lab = lj.argmax(axis=2)
    lab[order <= 1] = 0                                                  # order 1 has no parameters
    cnt = (lab[:, :, None] == np.arange(C)[None, None, :]).sum(axis=1)   # [B, C]
    # the reads of a replicate by (label, size): component c's are cnt[c] neighbours from first[c] on
    by = np.lexsort((xs, lab), axis=1)
    v = np.take_along_axis(xs, by, axis=1)
    first = np.cumsum(cnt, axis=1) - cnt
    lo = np.minimum(first + (np.maximum(cnt, 1) - 1) // 2, m - 1)
    hi = np.minimum(first + np.maximum(cnt, 1) // 2, m - 1)
    median = (np.take_along_axis(v, lo, axis=1) + np.take_along_axis(v, hi, axis=1)) / 2
    size = (median + 0.5).astype(np.int64)
    keep = cnt > 0
    if remove_noisy_reads:
        n = keep.sum(axis=1)
        ranked = -np.sort(-cnt, axis=1)                                  # descending; the empty ones last
        bar = ranked[:, min(ploidy, C) - 1]
        keep &= ~((n > ploidy)[:, None] & (cnt * 1.5 <= bar[:, None]))
    by_mean = np.argsort(np.where(keep, mu, np.inf), axis=1, kind="stable")
    sizes = np.take_along_axis(np.where(keep, size, -1), by_mean, axis=1)
    count = np.where(decided, keep.sum(axis=1), -1)
    sizes[~decided] = -1
    return count, sizes


def percentile_interval(values, confidence=0.95):
    """The nearest-rank interval of r values: (v[floor(q (r - 1))], v[ceil((1 - q) (r - 1))]) of the sorted values,
    q = (1 - confidence) / 2.  (The 1e-9 keeps a product that is an integer but for its rounding on that integer.)"""
    v = np.sort(np.asarray(values))
    r = len(v)
    if r == 0:
        return None
    q = (1.0 - confidence) / 2.0
    return (v[int(math.floor(q * (r - 1) + 1e-9))], v[int(math.ceil((1.0 - q) * (r - 1) - 1e-9))])


class RegionBootstrap:
    """The bootstrap of one region: `count` and `sizes` of its replicates (alleles_of_replicates), and against the
    called alleles `rows`: per allele (size, reads, CI low, CI high, replicates used), `support` and `distribution`."""

    def __init__(self, seed, count, sizes, alleles, confidence):
        self.seed, self.count, self.sizes = seed, count, sizes
        decided = count >= 0
        self.n_replicates = len(count)
        called = len(alleles)
        same = count == called
        self.support = float(same.sum()) / max(1, int(decided.sum()))
        values, tally = np.unique(count[decided], return_counts=True)
        self.distribution = ",".join(f"{int(a)}:{int(b)}" for a, b in zip(values, tally)) or "-"
        self.rows = []
        for rank, allele in enumerate(alleles):
            ci = percentile_interval(sizes[same, rank], confidence) if rank < sizes.shape[1] else None
            self.rows.append((allele.repeat1_median_size, allele.num_reads, None if ci is None else int(ci[0]),
                              None if ci is None else int(ci[1]), int(same.sum())))


def bootstrap_regions(repeat_regions, problems, fitted, B, ploidy, remove_noisy_reads, confidence=0.95, engine=None,
                      device=0):
    """Sets region.bootstrap (a RegionBootstrap, or None for a region without a call) for every region: `problems`
    and `fitted` are mixture.phase_jobs' problems and results, region by region."""
    live = [k for k, (p, f) in enumerate(zip(problems, fitted)) if p is not None and f is not None]
    reps = nr_mixture.bootstrap([problems[k] for k in live], B, engine, device)
    for region in repeat_regions:
        region.bootstrap = None
    for k, rep in zip(live, reps):
        p = problems[k]
        count, sizes = alleles_of_replicates(p.x[:, 0], rep, ploidy, remove_noisy_reads)
        repeat_regions[k].bootstrap = RegionBootstrap(p.seed, count, sizes, fitted[k][0], confidence)


def write_region_bootstrap(region):
    """`<region>.bootstrap.tsv`: the alleles of every replicate."""
    boot = getattr(region, "bootstrap", None)
    if boot is None or region.no_details or not region.out_prefix:
        return None
    path = region.out_prefix + ".bootstrap.tsv"
    with open(path, "w") as f:
        f.write(f"##RepeatRegion={region.to_unique_id()}\n##Seed={boot.seed}\n#Replicate\tNum_Alleles\tAllele_Sizes\n")
        for b, (n, sizes) in enumerate(zip(boot.count, boot.sizes)):
            text = ",".join(str(int(s)) for s in sizes[:max(int(n), 0)]) or "-"
            f.write(f"{b}\t{int(n) if n >= 0 else '-'}\t{text}\n")
    return path


def summary_rows(region):
    head = f"{region.chrom}\t{max(0, region.start_pos)}\t{region.end_pos}\t{region.repeat_unit_seq}"
    boot = getattr(region, "bootstrap", None)
    if boot is None:
        return head + "\t-" * (N_FIELDS - 4) + "\n"
    out = []
    for rank, (size, reads, lo, hi, used) in enumerate(boot.rows):
        out.append(f"{head}\t{rank + 1}\t{size}\t{reads}\t{'-' if lo is None else lo}\t{'-' if hi is None else hi}\t"
                   f"{used}\t{boot.n_replicates}\t{boot.support:.4f}\t{boot.distribution}\n")
    return "".join(out)


def write_bootstrap_summary(regions, path):
    """`<out_prefix>.NanoRepeat_bootstrap.tsv`: one row per (region, called allele), in BED order; a region without
    a call gets one row of `-`."""
    with open(path, "w") as f:
        f.write(HEADER)
        f.write("".join(summary_rows(region) for region in regions))
    return path
