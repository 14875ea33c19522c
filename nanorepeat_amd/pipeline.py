"""Steps 1-4 of quantify1repeat_from_bam (nanoRepeat_bam.py:614-686) for one or many regions,
from reads already extracted for the region: anchors -> core -> rounds 1-2 -> round 3 -> the
`repeat_size.txt` text -> GMM phasing -> one row of `NanoRepeat_output.tsv` per region.
`quantify_from_bam`, `quantify_from_reads` (FASTQ / FASTA) and `quantify_joint` are the commands from files
to files."""
from . import upstream, round3, phasing, joint, io as nr_io


def quantify_regions(repeat_regions, reads_by_region, data_type="ont", fast_mode=False, num_cpu=1,
                     device=0, scoring=None, aligner=None, scorer=None, keep_candidates=False):
    """repeat_regions: RepeatRegion objects with anchors set (io.extract_ref_sequence);
    reads_by_region: one {read_name: sequence} dict per region.  Every step runs for all regions in
    one C-ABI call (per ~256 M bases): a call costs a few milliseconds however small it is.
    keep_candidates: round 3 also fetches every candidate's score (round3.round3_estimation_regions)."""
    upstream.find_anchor_locations_in_reads_many(data_type, repeat_regions, reads_by_region, num_cpu, device=device,
                                                 scoring=scoring, aligner=aligner)
    for region, reads in zip(repeat_regions, reads_by_region):
        upstream.make_core_seq(region, reads)
    upstream.round1_and_round2_estimation_many(data_type, repeat_regions, num_cpu, device=device, scoring=scoring,
                                               aligner=aligner)
    round3.round3_estimation_regions(data_type, fast_mode, repeat_regions, num_cpu, device, scoring, scorer,
                                     keep_candidates)
    report_unscored_reads(repeat_regions)
    return [round3.output_repeat_size_1d(region) for region in repeat_regions]


def report_unscored_reads(repeat_regions, stream=None):
    """Reads that did not get a round-3 size of their own must not blend in silently: reads beyond the C
    ABI's length limits (left out of steps 1-2, or kept at their round-2 size in step 3) are listed per
    region on `region.skipped_reads` and counted on stderr.  Returns the number of such reads."""
    import sys
    stream = stream or sys.stderr
    total = 0
    for region in repeat_regions:
        skipped = dict(getattr(region, "skipped_reads", None) or {})
        for name, read in region.read_dict.items():
            if getattr(read, "round3_status", None) == round3.READ_TOO_LONG:
                skipped[name] = "core or template beyond the scorer's limits: kept at its round-2 size"
        region.skipped_reads = skipped
        if skipped:
            total += len(skipped)
            some = ", ".join(list(skipped)[:5]) + (" ..." if len(skipped) > 5 else "")
            print(f"NOTICE: {region.to_unique_id()}: {len(skipped)} read(s) beyond the length limits were not "
                  f"scored in full ({some})", file=stream)
    return total


def _fit_in_worker_processes(jobs, n_jobs):
    """phasing.run_job over `jobs` in n_jobs fresh interpreters (`python -m
    nanorepeat_amd._phase_worker`): they get only the sizes, never import the caller's main module
    and never open the GPU."""
    import os, pickle, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    shares = [list(range(w, len(jobs), n_jobs)) for w in range(n_jobs)]
    # start every interpreter first (they import scikit-learn side by side), then hand out the work
    procs = [subprocess.Popen([sys.executable, "-m", "nanorepeat_amd._phase_worker"], stdin=subprocess.PIPE,
                              stdout=subprocess.PIPE, env=env) for _ in shares]
    for share, p in zip(shares, procs):
        p.stdin.write(pickle.dumps([jobs[i] for i in share]))
        p.stdin.close()
    fitted = [None] * len(jobs)
    for share, p in zip(shares, procs):
        data = p.stdout.read()
        if p.wait() != 0:
            raise RuntimeError("a phasing worker process failed")
        for i, res in zip(share, pickle.loads(data)):
            fitted[i] = res
    return fitted


def phase_regions(repeat_regions, data_type="ont", ploidy=2, max_mutual_overlap=0.15, max_num_components=-1,
                  remove_noisy_reads=False, seed=None, out_tsv_file=None, n_jobs=None, mixture="sklearn", device=0,
                  mixture_engine=None, bootstrap=0, bootstrap_confidence=0.95, bootstrap_engine=None,
                  bootstrap_tsv_file=None):
    """Step 4 for every region (nanoRepeat_bam.py:683-684) and the final table (:737-743); defaults
    are the CLI's (nanoRepeat.py:121-129,159-160).  With a seed, region i uses seed + i.  The mixture
    fits -- by far the longest step of the whole command -- run in up to 16 worker processes like
    the reference's region workers (nanoRepeat_bam.py:712-724); the workers are fresh interpreters
    that get only the sizes and never touch the GPU.  n_jobs=1 keeps everything in this process.
    mixture="gpu" fits every region's mixtures on the GPU instead, in this process, in one C-ABI call per
    window of model orders (mixture.py): no worker processes, no scikit-learn, and a
    run is a function of its seed (seed=None draws one).  `mixture_engine` stands in for that call (tests).
    bootstrap=B > 0 (mixture="gpu" only) adds bootstrap confidence intervals (bootstrap.py): the
    order search of B resamples of every region's kept reads in one more GPU call, `<region>.bootstrap.tsv` with every
    replicate's alleles, region.bootstrap with the intervals (bootstrap_confidence) and the allele-count support, and
    their table in bootstrap_tsv_file when given.  `bootstrap_engine` stands in for that call (tests)."""
    import os
    from . import mixture as nr_mixture
    nr_mixture.check_engine_name(mixture)
    _check_bootstrap(bootstrap, mixture)
    if mixture == "gpu" and seed is None:
        seed = nr_mixture.fresh_seed()
    if max_num_components == -1:
        max_num_components = ploidy + 20
    error_rate = phasing.data_type_error_rate(data_type)
    jobs = [(phasing.region_count_dict(region), ploidy, error_rate, max_mutual_overlap, max_num_components,
             remove_noisy_reads, None if seed is None else seed + i) for i, region in enumerate(repeat_regions)]
    problems = []
    if mixture == "gpu":
        fitted = nr_mixture.phase_jobs([("1d", j) for j in jobs], device, mixture_engine, problems)
    else:
        if n_jobs is None:
            n_jobs = min(16, os.cpu_count() or 1, max(1, sum(len(j[0]) >= 2 for j in jobs)))
        if n_jobs > 1:
            fitted = _fit_in_worker_processes([("1d", j) for j in jobs], n_jobs)
        else:
            fitted = [phasing.phase_1d_job(j) for j in jobs]
    rows = []
    for region, job, fit in zip(repeat_regions, jobs, fitted):
        if fit is not None:
            phasing.split_allele_using_gmm_1d(region, ploidy, error_rate, max_mutual_overlap, max_num_components,
                                              remove_noisy_reads, fitted=fit)
        rows.append(phasing.final_output_row(region))
    if bootstrap:
        from . import bootstrap as nr_bootstrap
        nr_bootstrap.bootstrap_regions(repeat_regions, problems, fitted, bootstrap, ploidy, remove_noisy_reads,
                                       bootstrap_confidence, bootstrap_engine, device)
        for region in repeat_regions:
            nr_bootstrap.write_region_bootstrap(region)
        if bootstrap_tsv_file:
            nr_bootstrap.write_bootstrap_summary(repeat_regions, bootstrap_tsv_file)
    if out_tsv_file:
        with open(out_tsv_file, "w") as f:
            f.write("".join(rows))
    return rows


def _check_bootstrap(bootstrap, mixture):
    if bootstrap < 0 or int(bootstrap) != bootstrap:
        raise ValueError(f"bootstrap must be a number of replicates >= 0, not {bootstrap!r}")
    if bootstrap and mixture != "gpu":
        raise ValueError('bootstrap > 0 needs mixture="gpu": only that fit is a function of (sizes, seed)')


def quantify_joint(in_fq, ref_fasta, repeat1_string, repeat2_string, out_prefix, data_type="ont", num_threads=1,
                   ploidy=2, error_rate=0.1, max_mutual_overlap=0.1, remove_noisy_reads=False,
                   max_num_components=-1, device=0, scoring=None, seed=None, phase_in_worker=True, mixture="sklearn",
                   **engines):
    """The joint (2D) command from files to files (nanoRepeat_joint.py:160-232): round 1 ->
    grid rounds 2/3 -> `<out_prefix>.repeat_size.txt` -> 2D GMM phasing -> `.phased_reads.txt`,
    `.summary.txt`, `.alleleN.fastq`.  `engines` may carry aligner / cigar_aligner / scorer /
    mixture_engine stand-ins (tests).  mixture="gpu": the 2D mixtures are fitted on the GPU in this process
    (see phase_regions).  Returns (RepeatSize, allele list or None)."""
    from . import mixture as nr_mixture
    nr_mixture.check_engine_name(mixture)
    if max_num_components == -1:
        max_num_components = ploidy + 20
    fastq_dict = nr_io.fastq_file_to_dict(in_fq)
    if len(fastq_dict) < ploidy:
        raise ValueError(f"not enough reads for analysis: ploidy {ploidy}, {len(fastq_dict)} reads in {in_fq}")
    repeat1 = joint.Repeat().init_from_string(repeat1_string)
    repeat2 = joint.Repeat().init_from_string(repeat2_string)
    if repeat1.chrom != repeat2.chrom:
        raise ValueError("joint quantification only works with two nearby repeats on one chromosome")
    if repeat1.start > repeat2.start:
        repeat1, repeat2 = repeat2, repeat1
    repeat1.max_size += 10
    repeat2.max_size += 10
    if repeat1.end + 100 < repeat2.start:
        raise ValueError("joint quantification only works with two nearby repeats (distance < 100 bp)")
    repeat_chrom_seq = nr_io.read_one_chr_from_fasta_file(ref_fasta, repeat1.chrom)
    if not repeat_chrom_seq:
        raise ValueError(f"ref_fasta file {ref_fasta} has no sequence named {repeat1.chrom}")
    initial_estimation = joint.initial_estimate_repeat_size(
        repeat_chrom_seq, fastq_dict, data_type, num_threads, repeat1, repeat2, 1000, device=device, scoring=scoring,
        aligner=engines.get("aligner"), cigar_aligner=engines.get("cigar_aligner"))
    final_estimation = joint.fine_tune_read_count(initial_estimation, fastq_dict, repeat_chrom_seq, repeat1, repeat2,
                                                  data_type, num_threads, None, device, scoring, engines.get("scorer"))
    joint_counts, _ = joint.output_repeat_size_2d(in_fq, repeat1.repeat_id, repeat2.repeat_id, out_prefix,
                                                  final_estimation.repeat1_count_dict,
                                                  final_estimation.repeat2_count_dict)
    # the fit runs in a fresh single-threaded interpreter: scikit-learn's small-matrix algebra is several
    # times slower with this process's BLAS/OpenMP thread pools (split_alleles.py:28-32 pins them to 1)
    if mixture == "gpu" and seed is None:
        seed = nr_mixture.fresh_seed()
    job = ("2d", (joint_counts, ploidy, error_rate, max_mutual_overlap, max_num_components, remove_noisy_reads, seed))
    if mixture == "gpu":
        fitted = nr_mixture.phase_jobs([job], device, engines.get("mixture_engine"))[0]
        if fitted is None:                  # too few reads: nothing to write, as when the default engine returns None
            return final_estimation, None
    else:
        fitted = _fit_in_worker_processes([job], 1)[0] if phase_in_worker else None
    alleles = phasing.split_alleles_using_gmm_2d(ploidy, error_rate, max_mutual_overlap, remove_noisy_reads,
                                                 max_num_components, repeat1, repeat2, joint_counts, 0, in_fq,
                                                 out_prefix, seed=seed, fitted=fitted)
    return final_estimation, alleles


def quantify_from_bam(in_bam_file, ref_fasta, repeat_region_bed, out_prefix, data_type="ont", anchor_len=1000,
                      fast_mode=False, ploidy=2, max_mutual_overlap=0.15, max_num_components=-1,
                      remove_noisy_reads=False, no_check_repeat_motif_in_ref=False, no_details=False,
                      num_cpu=1, device=0, scoring=None, seed=None, read_structure=False, discover_motifs=False,
                      min_motif_count=4, min_motif_share=0.1, partial_reads=False, mixture="sklearn",
                      allele_consensus=False, allele_split=False, motif_runs=False, segment_motifs=None,
                      switch_cost=None, read_alignments=False, discover_periods=False, in_repeat_reads=False,
                      bootstrap=0, bootstrap_confidence=0.95, flank_phase=False, flank_len=3000, flank_skip=20,
                      flank_min_sites=2, censored_fit=False, censored_error_rate=None, censored_max_alleles=6,
                      censored_bootstrap=0, methylation=False, meth_flank=2000, meth_bin=200, meth_hi=192, meth_lo=63,
                      meth_mod_code="m", **engines):
    """The BAM command from files to files (nanoRepeat_bam.py:614-751): for every region of the BED
    file, reads from the alignment file -> `<out_prefix>.details/<chr>/<region>.*` ->
    `<out_prefix>.NanoRepeat_output.tsv`.  The reference forks up to 16 workers, one region each;
    here steps 1-2 run region by region and step 3 for all regions in one GPU batch.  Regions
    without reads, or whose reference sequence fails the motif check, get their row with 0
    alleles like in the reference.  read_structure=True adds the repeat structure files
    (structure.py); discover_motifs=True adds the tandem motif files (motifs.py; min_motif_count and
    min_motif_share set the per-read call); partial_reads=True adds the one-anchor read files (partial.py): for
    every read with one anchor only, the repeat units it shows next to that anchor, and per region whether any such
    read shows more than the largest spanning read.  mixture="gpu" fits the phasing mixtures on the GPU (see
    phase_regions).  allele_consensus=True adds the consensus sequence of every allele's tract (consensus.py);
    allele_split=True adds the allele split files: alleles that hold two sequences of one size (split.py).
    motif_runs=True adds the motif run files (segments.py): every read's tract and every allele's consensus cut into
    runs of the motifs of the region's motif set (the BED motif, then segment_motifs[region key] when that dict names
    the region, else the motifs discovered in the reads); switch_cost is the price of changing motif (None: the
    default of segments.py).  read_alignments=True adds `<region>.round3.paf` (alignments.py): the alignment of every
    read with a round-3 size of its own to the template it was called at.  discover_periods=True adds the tandem
    period files (periods.py): the period (up to 64 bases) and the unit of every allele's consensus tract, every read's
    evidence for it, and the reads' sizes in that unit where it is not the BED motif.  in_repeat_reads=True adds the
    in-repeat read files (partial.py): for every read of the region's window without a hit of either anchor, the repeat
    units it shows, and per region whether any such read shows more than the largest spanning read.  bootstrap=B > 0
    (with mixture="gpu") adds the bootstrap files (bootstrap.py): `<region>.bootstrap.tsv` and
    `<out_prefix>.NanoRepeat_bootstrap.tsv` with a bootstrap_confidence interval for every allele size and the share
    of the B replicates that have the called number of alleles.  flank_phase=True adds the flank haplotype files
    (flank.py): the reads, one-anchor reads included when partial_reads is on, phased by the variants of the flank_len
    reference bases on either side of the repeat (no site within flank_skip bases of it; flank_min_sites supported sites
    for a verdict), the table size allele x haplotype, and per haplotype the most units its one-anchor reads show.
    censored_fit=True (with partial_reads and / or in_repeat_reads, else ValueError) adds the censored allele fit
    (censored.py): the spanning reads' sizes and the bounds of the one-anchor and in-repeat reads in one mixture
    likelihood, with an open allele where no read spans one; censored_error_rate is its sd in the log domain (None: the
    data type's error rate) and censored_max_alleles the largest number of closed alleles it tries.
    censored_bootstrap=B > 0 (with censored_fit=True, else ValueError; independent of `mixture`) adds the bootstrap of
    that fit: B resamples of every region's spanning reads and bounds, their model searches in
    one GPU call, `<region>.censored_bootstrap.tsv` and `<out_prefix>.NanoRepeat_censored_bootstrap.tsv` with the share
    of replicates that give the called model and an open allele and a bootstrap_confidence interval for every called
    allele's size and weight (censored_engine may carry `censored_bootstrap` as a stand-in for the call).
    methylation=True adds the CpG methylation files (methylation.py): the 5mC calls of the records' MM / ML tags
    (modification code meth_mod_code) counted per read and per allele over the repeat tract and over the meth_flank read
    bases on either side of it in bins of meth_bin; a call byte >= meth_hi counts as methylated, one <= meth_lo as
    unmethylated.
    `engines` may carry aligner / scorer / structure_engine / motif_engine / extension_engine / mixture_engine /
    consensus_engine / split_engine / segment_engine / path_aligner / period_engine / bootstrap_engine / flank_engine /
    censored_engine / methylation_engine stand-ins.  Returns the regions."""
    from . import bam as nr_bam, mixture as nr_mixture
    nr_mixture.check_engine_name(mixture)
    _check_bootstrap(bootstrap, mixture)
    meth = _methylation_options(methylation, meth_flank, meth_bin, meth_hi, meth_lo, meth_mod_code)
    censored = _censored_options(censored_fit, censored_error_rate, censored_max_alleles, partial_reads,
                                 in_repeat_reads)
    _check_censored_bootstrap(censored_bootstrap, censored_fit)
    regions = nr_io.read_repeat_region_file(repeat_region_bed, no_details)
    ref_fasta_dict = nr_io.fasta_file2dict(ref_fasta)
    live, reads_of, tags_of = [], [], []
    for i, region in enumerate(regions):
        _set_region_paths(region, i, out_prefix)
        tags = {} if meth is not None else None
        n = nr_bam.extract_fastq_from_bam(in_bam_file, region, anchor_len, region.region_fq_file, ref_fasta,
                                          **({} if tags is None else dict(mod_tags=tags)))
        if n == 0:
            continue
        nr_io.extract_ref_sequence(ref_fasta_dict, region, anchor_len)
        if not no_check_repeat_motif_in_ref and not nr_io.check_repeat_motif_in_ref(region):
            continue
        live.append(region)
        reads_of.append(nr_io.read_fastq(region.region_fq_file))
        tags_of.append(tags)
    if meth is not None:
        meth["tags_of"] = tags_of
    flank = _flank_options(flank_phase, flank_len, flank_skip, flank_min_sites, regions, ref_fasta_dict)
    _quantify_and_write(regions, live, reads_of, out_prefix, data_type, fast_mode, ploidy, max_mutual_overlap,
                        max_num_components, remove_noisy_reads, no_details, num_cpu, device, scoring, seed, engines,
                        read_structure, _motif_options(discover_motifs, min_motif_count, min_motif_share),
                        partial_reads, mixture, allele_consensus, allele_split,
                        _run_options(motif_runs, segment_motifs, switch_cost), read_alignments, discover_periods,
                        in_repeat_reads=in_repeat_reads, bootstrap=(bootstrap, bootstrap_confidence), flank=flank,
                        censored=censored, censored_bootstrap=censored_bootstrap, methylation=meth)
    return regions


def _set_region_paths(region, index, out_prefix):
    """`<out_prefix>.details/<chr>/<region>` (made here) and the region's `.reads.fastq` beside it."""
    import os
    region.index = index
    chrom_dir = region.chrom if region.chrom[0:3].lower() == "chr" else "chr" + region.chrom
    out_dir = f"{out_prefix}.details/{chrom_dir}"
    os.makedirs(out_dir, exist_ok=True)
    region.out_prefix = f"{out_dir}/{phasing.outfile_prefix(region)}"
    region.region_fq_file = f"{region.out_prefix}.reads.fastq"


def _motif_options(discover_motifs, min_motif_count, min_motif_share):
    return dict(min_motif_count=min_motif_count, min_motif_share=min_motif_share) if discover_motifs else None


def _run_options(motif_runs, segment_motifs, switch_cost):
    return dict(segment_motifs=segment_motifs, switch_cost=switch_cost) if motif_runs else None


def _flank_options(flank_phase, flank_len, flank_skip, flank_min_sites, regions, ref_fasta_dict):
    """None, or the keywords of flank.flank_regions; sets every region's reference flanks."""
    if not flank_phase:
        return None
    if flank_len < 1:
        raise ValueError(f"flank_len must be >= 1, not {flank_len!r}")
    from . import flank as nr_flank
    for region in regions:
        nr_flank.set_flank_sides(region, ref_fasta_dict, flank_len)
    return dict(flank_len=flank_len, skip=flank_skip, min_sites=flank_min_sites)


def _methylation_options(methylation, flank, bin_len, hi, lo, mod_code):
    """None, or the keywords of methylation.methylation_regions (the commands add `tags_of`)."""
    if not methylation:
        return None
    from . import methylation as nr_methylation
    nr_methylation.check_options(flank, bin_len, hi, lo, mod_code)
    return dict(flank=flank, bin_len=bin_len, hi=hi, lo=lo, mod_code=mod_code)


def _censored_options(censored_fit, error_rate, max_alleles, partial_reads, in_repeat_reads):
    """None, or the keywords of censored.censored_regions."""
    if not censored_fit:
        return None
    if not (partial_reads or in_repeat_reads):
        raise ValueError("censored_fit=True needs partial_reads=True and / or in_repeat_reads=True: they size the reads "
                         "it adds to the fit")
    if error_rate is not None and not (error_rate > 0 and error_rate < float("inf")):
        raise ValueError(f"censored_error_rate must be finite and > 0, not {error_rate!r}")
    if not 1 <= max_alleles <= 8:
        raise ValueError(f"censored_max_alleles must be in 1..8, not {max_alleles!r}")
    return dict(error_rate=error_rate, max_alleles=max_alleles, use_partial=bool(partial_reads),
                use_in_repeat=bool(in_repeat_reads))


def _check_censored_bootstrap(censored_bootstrap, censored_fit):
    if isinstance(censored_bootstrap, bool) or censored_bootstrap < 0 or int(censored_bootstrap) != censored_bootstrap:
        raise ValueError(f"censored_bootstrap must be a number of replicates >= 0, not {censored_bootstrap!r}")
    if censored_bootstrap and not censored_fit:
        raise ValueError("censored_bootstrap > 0 needs censored_fit=True: it resamples the reads of that fit")


def _quantify_and_write(regions, live, reads_of, out_prefix, data_type, fast_mode, ploidy, max_mutual_overlap,
                        max_num_components, remove_noisy_reads, no_details, num_cpu, device, scoring, seed, engines,
                        read_structure=False, motif_options=None, partial_reads=False, mixture="sklearn",
                        allele_consensus=False, allele_split=False, run_options=None, read_alignments=False,
                        discover_periods=False, in_repeat_reads=False, candidates=None, bootstrap=(0, 0.95), flank=None,
                        censored=None, censored_bootstrap=0, methylation=None):
    """The commands' common tail: steps 1-4 for the regions with reads, then one TSV row per BED region; with
    read_structure, the structure of every read with a size and the two structure files; with motif_options (a dict
    of motifs.motif_regions keywords), the tandem motifs of every read with a core and the two motif files; with
    partial_reads, the extension of every one-anchor read, the two partial-read files and a NOTICE per region where
    such reads show more repeat units than any spanning read; with allele_consensus, the consensus of every allele's
    tracts, the two consensus files and one NOTICE counting the alleles that did not converge or left reads out; with
    allele_split, the split of every allele by tract sequence, the three split files and one NOTICE counting the alleles
    split; with run_options (a dict of segments.segments_regions keywords), the motif runs of every read with a core and
    of every allele's consensus, the two run files and one NOTICE counting the alleles of more than one run; with
    read_alignments, the round-3 alignment of every read with a size of its own, one file per region and a NOTICE per
    region that left reads out; with discover_periods, the tandem period of every allele's consensus tract and every
    read's evidence for it, the two period files and one NOTICE counting the alleles whose unit is not the BED motif;
    with in_repeat_reads, the four extensions of every read without an anchor, the two in-repeat files and a NOTICE per
    region where such reads show more repeat units than any spanning read.  `candidates` (the FASTQ command, a dict of
    _place_candidates keywords): the one-anchor and in-repeat reads come from the screen's candidates too.  `bootstrap`
    (replicates, confidence): with replicates > 0, the bootstrap of every region's phasing and the two bootstrap files.
    With `flank` (a dict of flank.flank_regions keywords), the flank haplotypes of every region with reads (one-anchor
    reads too when partial_reads is on), the two flank files and a NOTICE per region with an unspanned haplotype.
    With `censored` (a dict of censored.censored_regions keywords), after the one-anchor and in-repeat reads: the
    censored allele fit of every region with reads or candidates, its three files and one NOTICE; with
    censored_bootstrap (replicates) > 0 then the bootstrap of that fit (confidence: bootstrap[1]; the streams are named
    by `seed`, a fresh one when it is None), its two files and one NOTICE.  With `methylation` (a dict of
    methylation.methylation_regions keywords and `tags_of`, the tags of every region with reads), the CpG counters of
    every read with a size, the three methylation files and one NOTICE counting the reads without usable calls."""
    if in_repeat_reads:
        for region in live:
            region.keep_no_anchor_reads = True
    flank_of, flank_reads = live, reads_of
    quantify_regions(live, reads_of, data_type, fast_mode, num_cpu, device, scoring,
                     engines.get("aligner"), engines.get("scorer"), keep_candidates=read_alignments and not no_details)
    phase_regions(live, data_type, ploidy, max_mutual_overlap, max_num_components, remove_noisy_reads, seed,
                  mixture=mixture, device=device, mixture_engine=engines.get("mixture_engine"),
                  bootstrap=bootstrap[0], bootstrap_confidence=bootstrap[1],
                  bootstrap_engine=engines.get("bootstrap_engine"))
    with open(f"{out_prefix}.NanoRepeat_output.tsv", "w") as f:
        for region in regions:
            f.write(phasing.final_output_row(region))
    if bootstrap[0]:
        from . import bootstrap as nr_bootstrap
        nr_bootstrap.write_bootstrap_summary(regions, f"{out_prefix}.NanoRepeat_bootstrap.tsv")
    if read_structure:
        from . import structure
        structure.structure_regions(live, device=device, engine=engines.get("structure_engine"))
        for region in live:
            structure.write_read_structure(region)
        structure.write_structure_summary(regions, out_prefix)
    if motif_options is not None:
        from . import motifs
        motifs.motif_regions(live, fast_mode, device=device, engine=engines.get("motif_engine"),
                             scorer=engines.get("scorer"), scoring=scoring, **motif_options)
        for region in live:
            motifs.write_read_motifs(region)
        motifs.write_motif_summary(regions, out_prefix)
    if partial_reads or in_repeat_reads:
        from . import partial
        of, of_reads, keep, shared, unscreened = live, reads_of, None, None, ()
        if candidates is not None:
            of, of_reads, keep, shared, unscreened = _place_candidates(
                regions, live, reads_of, data_type, num_cpu, device, scoring, engines.get("aligner"), in_repeat_reads,
                **candidates)
        if partial_reads:
            flank_of, flank_reads = of, of_reads
            partial.partial_regions(of, of_reads, device=device, scoring=scoring, engine=engines.get("extension_engine"))
            for region in of:
                partial.write_partial_reads(region)
            partial.write_partial_summary(regions, out_prefix)
            partial.report_exceeding_reads(of)
        if in_repeat_reads:
            partial.in_repeat_regions(of, of_reads, device=device, scoring=scoring,
                                      engine=engines.get("extension_engine"), keep=keep)
            for region in of:
                partial.write_in_repeat_reads(region)
            partial.write_in_repeat_summary(regions, out_prefix, shared, unscreened)
            partial.report_exceeding_in_repeat_reads(of)
        if censored is not None:
            from . import censored as nr_censored
            nr_censored.censored_regions(of, data_type, engine=engines.get("censored_engine"), device=device,
                                         **censored)
            for region in of:
                nr_censored.write_censored_fit(region)
                nr_censored.write_censored_reads(region)
            nr_censored.write_censored_summary(regions, out_prefix)
            nr_censored.report_censored_calls(of)
            if censored_bootstrap:
                from . import mixture as nr_mixture
                stand_in = engines.get("censored_engine")
                nr_censored.bootstrap_regions(
                    of, int(censored_bootstrap), nr_mixture.fresh_seed() if seed is None else seed, bootstrap[1],
                    censored["max_alleles"], stand_in if hasattr(stand_in, "censored_bootstrap") else None, device)
                for region in of:
                    nr_censored.write_censored_bootstrap(region)
                nr_censored.write_censored_bootstrap_summary(regions, out_prefix)
                nr_censored.report_censored_bootstrap(of)
    if allele_consensus:
        from . import consensus
        consensus.consensus_regions(live, device=device, engine=engines.get("consensus_engine"),
                                    structure_engine=engines.get("structure_engine"))
        for region in live:
            consensus.write_allele_consensus(region)
        consensus.write_consensus_summary(regions, out_prefix)
        consensus.report_unsettled_alleles(live)
    if allele_split:
        from . import split
        split.split_regions(live, device=device, engine=engines.get("split_engine"),
                            consensus_engine=engines.get("consensus_engine"),
                            structure_engine=engines.get("structure_engine"))
        for region in live:
            split.write_allele_split(region)
        split.write_split_summary(regions, out_prefix)
        split.report_split_alleles(live)
    if run_options is not None:
        from . import segments
        segments.segments_regions(live, device=device, engine=engines.get("segment_engine"),
                                  motif_engine=engines.get("motif_engine"),
                                  consensus_engine=engines.get("consensus_engine"),
                                  structure_engine=engines.get("structure_engine"), **run_options)
        for region in live:
            segments.write_read_runs(region)
        segments.write_runs_summary(regions, out_prefix)
        segments.report_multi_run_alleles(live)
    if read_alignments and not no_details:
        from . import alignments
        alignments.alignment_regions(live, device=device, scoring=scoring, engine=engines.get("path_aligner"))
        for region in live:
            alignments.write_read_alignments(region)
        alignments.report_left_out_reads(live)
    if discover_periods:
        from . import periods
        periods.period_regions(live, fast_mode, device=device, engine=engines.get("period_engine"),
                               scorer=engines.get("scorer"), scoring=scoring,
                               consensus_engine=engines.get("consensus_engine"),
                               structure_engine=engines.get("structure_engine"))
        for region in live:
            periods.write_read_periods(region)
        periods.write_period_summary(regions, out_prefix)
        periods.report_foreign_units(live)
    if flank is not None:
        from . import flank as nr_flank
        nr_flank.flank_regions(flank_of, flank_reads, device=device, engine=engines.get("flank_engine"), **flank)
        for region in flank_of:
            nr_flank.write_flank_phase(region)
        nr_flank.write_flank_summary(regions, out_prefix)
        nr_flank.report_unspanned_haplotypes(flank_of)
    if methylation is not None:
        from . import methylation as nr_methylation
        options = dict(methylation)
        nr_methylation.methylation_regions(live, reads_of, options.pop("tags_of"), device=device,
                                           engine=engines.get("methylation_engine"), **options)
        for region in live:
            nr_methylation.write_read_methylation(region)
            nr_methylation.write_allele_methylation(region)
        nr_methylation.write_methylation_summary(regions, out_prefix)
    if no_details:
        import shutil
        shutil.rmtree(f"{out_prefix}.details", ignore_errors=True)


def quantify_from_reads(in_reads, ref_fasta, repeat_region_bed, out_prefix, data_type="ont", anchor_len=1000,
                        fast_mode=False, ploidy=2, max_mutual_overlap=0.15, max_num_components=-1,
                        remove_noisy_reads=False, no_check_repeat_motif_in_ref=False, no_details=False,
                        num_cpu=1, device=0, scoring=None, seed=None, screen=True, k=15, min_hits=4, max_occ=16,
                        chunk_bases=1 << 28, read_structure=False, discover_motifs=False, min_motif_count=4,
                        min_motif_share=0.1, mixture="sklearn", allele_consensus=False, allele_split=False,
                        motif_runs=False, segment_motifs=None, switch_cost=None, read_alignments=False,
                        discover_periods=False, partial_reads=False, in_repeat_reads=False, motif_share_pct=5,
                        bootstrap=0, bootstrap_confidence=0.95, flank_phase=False, flank_len=3000, flank_skip=20,
                        flank_min_sites=2, censored_fit=False, censored_error_rate=None, censored_max_alleles=6,
                        censored_bootstrap=0, methylation=False, meth_flank=2000, meth_bin=200, meth_hi=192,
                        meth_lo=63, meth_mod_code="m", discover_repeats=False, group_loci=False, locus_flank_len=500,
                        sketch_k=13, min_shared=None, min_locus_reads=3, place_loci=False, place_k=15, place_bin=64,
                        place_min_votes=None, place_max_occ=16, place_max_target_occ=64, place_flank_len=1000,
                        max_ref_span=50000, **engines):
    """The FASTQ / FASTA command (nanoRepeat.py:109, `-t fastq|fasta`) from files to files, without a genome mapper:
    the reads each region sees are chosen by the anchor k-mer screen (screen.reads_by_region) instead of a
    genome-wide mapping and a BAM window, then the BAM command's steps run unchanged.  Every region's reference
    must extract (else the command fails, as the BAM command does); regions that fail the motif check are not
    screened and get their 0-allele row.  Each region's reads go to `<out_prefix>.details/<chr>/<region>.reads.fastq`
    (qualities `.` for FASTA input).  screen=False offers every read to every region: exact, and slow beyond small
    panels.  read_structure=True adds the repeat structure files (structure.py); discover_motifs=True adds the
    tandem motif files (motifs.py).  mixture="gpu" fits the phasing mixtures on the GPU (see phase_regions).
    allele_consensus=True adds the consensus sequence of every allele's tract (consensus.py); allele_split=True adds
    the allele split files (split.py); motif_runs=True adds the motif run files (segments.py; segment_motifs and
    switch_cost as for quantify_from_bam); read_alignments=True adds the round-3 alignment files (alignments.py);
    discover_periods=True adds the tandem period files (periods.py).  partial_reads=True adds the one-anchor read files
    and in_repeat_reads=True the in-repeat read files, as for quantify_from_bam: the motif screen (DESIGN.md section
    23) offers the reads with one anchor only and the reads made of a region's motif (at least motif_share_pct % of
    their k-mer windows) as candidates, written to `<region>.partial_candidates.fastq`; they go through the anchor step
    apart from the region's reads and never reach the sizes or the phasing.  bootstrap=B > 0 (with mixture="gpu")
    adds the bootstrap files, flank_phase=True the flank haplotype files, censored_fit=True the censored allele fit
    and censored_bootstrap=B > 0 its bootstrap files, as for quantify_from_bam.  methylation=True adds the CpG
    methylation files as for quantify_from_bam, from the MM / ML tags in the header comments of a FASTQ file
    (io.read_fastq_mod_tags); FASTA input has none.  discover_repeats=True adds the discovered-repeat files
    (discover.py) after everything else, from a second pass over the file that needs no region:
    the tandem runs of every read, and per motif class how many reads carry one and how many BED regions have it.
    group_loci=True beside it adds the four locus files (loci.py): the runs grouped into loci by
    their flanks (locus_flank_len bases a side -- discover_repeats()' flank_len, which is the flank haplotypes' keyword
    here --, sketch_k, min_shared: None is the measured default) and a pseudo-reference with a BED file for the core
    loci with at least min_locus_reads spanned runs; without discover_repeats=True it is a ValueError.
    place_loci=True beside group_loci=True adds the two placement files (place.py): every locus's
    representative placed on ref_fasta by the place_flank_len bases on either side of its run (place_k, place_bin,
    place_min_votes: None is the measured default, place_max_occ, place_max_target_occ, max_ref_span), and a BED file of
    the placed loci on ref_fasta; without group_loci=True it is a ValueError.
    `engines` may carry aligner / scorer / screener / structure_engine / motif_engine / extension_engine /
    mixture_engine / consensus_engine / split_engine / segment_engine / path_aligner / period_engine /
    bootstrap_engine / flank_engine / censored_engine / methylation_engine / scan_engine / sketch_engine /
    place_engine stand-ins.  Returns the regions."""
    from . import screen as nr_screen, mixture as nr_mixture
    place_options = None
    if place_loci:
        from . import place as nr_place
        if not group_loci:
            raise ValueError("place_loci=True needs group_loci=True")
        place_options = _place_options(place_k, place_bin, place_min_votes, place_max_occ, place_max_target_occ,
                                       place_flank_len, max_ref_span)
        nr_place.check_options(**place_options)
    if group_loci:
        from . import loci as nr_loci
        if not discover_repeats:
            raise ValueError("group_loci=True needs discover_repeats=True")
        nr_loci.check_options(locus_flank_len, sketch_k, min_shared, min_locus_reads)
    nr_mixture.check_engine_name(mixture)
    _check_bootstrap(bootstrap, mixture)
    meth = _methylation_options(methylation, meth_flank, meth_bin, meth_hi, meth_lo, meth_mod_code)
    censored = _censored_options(censored_fit, censored_error_rate, censored_max_alleles, partial_reads,
                                 in_repeat_reads)
    _check_censored_bootstrap(censored_bootstrap, censored_fit)
    regions = nr_io.read_repeat_region_file(repeat_region_bed, no_details)
    ref_fasta_dict = nr_io.fasta_file2dict(ref_fasta)
    screened = []
    for i, region in enumerate(regions):
        _set_region_paths(region, i, out_prefix)
        nr_io.extract_ref_sequence(ref_fasta_dict, region, anchor_len)
        if no_check_repeat_motif_in_ref or nr_io.check_repeat_motif_in_ref(region):
            screened.append(region)
    with_candidates = partial_reads or in_repeat_reads
    if screen:
        found = nr_screen.reads_by_region(in_reads, screened, k=k, max_occ=max_occ, min_hits=min_hits,
                                          chunk_bases=chunk_bases, device=device, screener=engines.get("screener"),
                                          **(dict(partial=True, motif_share_pct=motif_share_pct) if with_candidates
                                             else {}))
    else:
        found = nr_screen.all_reads_by_region(in_reads, len(screened), chunk_bases,
                                              **(dict(partial=True) if with_candidates else {}))
    candidates = None
    if with_candidates:
        found, offered = found
        candidates = dict(offered={id(region): {n: c for n, c in cand.items() if n not in reads}
                                   for region, reads, cand in zip(screened, found, offered)},
                          k=k, min_hits=min_hits, motif_share_pct=motif_share_pct)
    found_of = {id(region): reads for region, reads in zip(screened, found)}
    live, reads_of = [], []
    for region in regions:
        reads = found_of.get(id(region), {})
        _write_region_fastq(region.region_fq_file, reads)
        if reads:
            live.append(region)
            reads_of.append({name: seq for name, (seq, _) in reads.items()})
    flank = _flank_options(flank_phase, flank_len, flank_skip, flank_min_sites, regions, ref_fasta_dict)
    if meth is not None:
        tags = _fastq_mod_tags(in_reads)
        meth["tags_of"] = [{name: tags[name] for name in reads if name in tags} for reads in reads_of]
    _quantify_and_write(regions, live, reads_of, out_prefix, data_type, fast_mode, ploidy, max_mutual_overlap,
                        max_num_components, remove_noisy_reads, no_details, num_cpu, device, scoring, seed, engines,
                        read_structure, _motif_options(discover_motifs, min_motif_count, min_motif_share),
                        mixture=mixture, allele_consensus=allele_consensus, allele_split=allele_split,
                        run_options=_run_options(motif_runs, segment_motifs, switch_cost),
                        read_alignments=read_alignments, discover_periods=discover_periods,
                        partial_reads=partial_reads, in_repeat_reads=in_repeat_reads, candidates=candidates,
                        bootstrap=(bootstrap, bootstrap_confidence), flank=flank, censored=censored,
                        censored_bootstrap=censored_bootstrap, methylation=meth)
    if discover_repeats:
        from . import discover as nr_discover
        nr_discover.discover_file(in_reads, out_prefix, repeat_region_bed, no_details=no_details, device=device,
                                  chunk_bases=chunk_bases, engine=engines.get("scan_engine"), group_loci=group_loci,
                                  flank_len=locus_flank_len, sketch_k=sketch_k, min_shared=min_shared,
                                  min_locus_reads=min_locus_reads, sketch_engine=engines.get("sketch_engine"),
                                  place_ref=ref_fasta if place_loci else None, place_options=place_options,
                                  place_engine=engines.get("place_engine"), place_aligner=engines.get("aligner"))
    return regions


def _place_options(place_k, place_bin, place_min_votes, place_max_occ, place_max_target_occ, place_flank_len,
                   max_ref_span):
    """The placement switches under place.check_options' names."""
    return dict(k=place_k, bin=place_bin, min_votes=place_min_votes, max_occ=place_max_occ,
                max_target_occ=place_max_target_occ, flank_len=place_flank_len, max_ref_span=max_ref_span)


def discover_repeats(reads_path, out_prefix, repeat_region_bed=None, k=11, max_gap=100, min_span=200, no_details=False,
                     device=0, engine=None, group_loci=False, flank_len=500, sketch_k=13, min_shared=None,
                     min_locus_reads=3, sketch_engine=None, place_ref=None, place_k=15, place_bin=64,
                     place_min_votes=None, place_max_occ=16, place_max_target_occ=64, place_flank_len=1000,
                     max_ref_span=50000, place_engine=None, place_aligner=None):
    """The discovery command from files to files (no counterpart in the reference): every read of a FASTQ / FASTA / BAM
    file through the repeat scan (discover.py), with no region, anchor or motif given ->
    `<out_prefix>.discovered_runs.tsv` (one row per tandem run of at least min_span bases; not with no_details) and
    `<out_prefix>.NanoRepeat_discovered.tsv` (one row per motif class with a run; with a BED file, how many of its
    regions have that class).  `engine` stands in for _capi.scan_repeats (tests).  group_loci=True (loci.py; DESIGN.md
    section 30) groups the runs into loci by the flank_len bases on either side of them (canonical sketch_k-mers, two
    sides match at min_shared shared ones: None is the measured default) and adds `<out_prefix>.discovered_loci.tsv`,
    `.discovered_locus_runs.tsv` (not with no_details) and `.discovered_loci.fa` / `.bed`, a pseudo-reference of the
    core loci with at least min_locus_reads spanned runs that quantify_from_reads takes as its reference and BED file;
    `sketch_engine` stands in for _capi.sketch_pairs.  place_ref="ref.fa" beside group_loci=True (place.py; DESIGN.md
    section 31) places every locus's representative on that reference: the place_flank_len bases on either side of its
    run are looked for in the reference, streamed contig by contig (canonical place_k-mers; diagonal bins of place_bin
    bases; a side is placed at place_min_votes votes, None: the measured default, that beat the runner-up 1.5-fold;
    place_max_occ and place_max_target_occ mask the k-mers repeated in the sides and in the reference), and a locus whose
    two sides land on one contig and strand at most max_ref_span bases apart is placed.  It adds
    `<out_prefix>.discovered_loci_placed.tsv` and `.discovered_loci.ref.bed`, a BED file of the placed loci on ref.fa
    that quantify_from_bam and quantify_from_reads take; place_engine stands in for _capi's place_* functions and
    place_aligner for _capi.align_pairs.  A bad value, or place_ref without group_loci, is a ValueError.  Returns the
    class rows."""
    from . import discover as nr_discover
    place_options = None if place_ref is None else _place_options(place_k, place_bin, place_min_votes, place_max_occ,
                                                                  place_max_target_occ, place_flank_len, max_ref_span)
    return nr_discover.discover_file(reads_path, out_prefix, repeat_region_bed, k, max_gap, min_span, no_details, device,
                                     engine=engine, group_loci=group_loci, flank_len=flank_len, sketch_k=sketch_k,
                                     min_shared=min_shared, min_locus_reads=min_locus_reads,
                                     sketch_engine=sketch_engine, place_ref=place_ref, place_options=place_options,
                                     place_engine=place_engine, place_aligner=place_aligner)


def _fastq_mod_tags(in_reads):
    """io.read_fastq_mod_tags of a FASTQ file; {} for FASTA input, which has no place for tags."""
    with nr_io.gzopen(in_reads) as fp:
        first = fp.readline()
        while first and not first.strip():
            first = fp.readline()
    return nr_io.read_fastq_mod_tags(in_reads) if first[:1] == "@" else {}


def _place_candidates(regions, live, reads_of, data_type, num_cpu, device, scoring, aligner, in_repeat_reads, offered,
                      k, min_hits, motif_share_pct):
    """The FASTQ command's candidates (`offered[id(region)]` = {name: (seq, qual, kind)}, none of them among the
    region's own reads) through the anchor step, each region's against a shadow of the region: only the shadow's
    one_anchor_reads and no_anchor_reads are carried over, so read_dict, the sizes and the phasing never see a
    candidate.  A candidate the anchor step would place as spanning is ignored; one NOTICE counts them.  Writes
    `<region>.partial_candidates.fastq`.  Returns (regions with reads or candidates, their {name: sequence}, the
    in-repeat rule as partial.in_repeat_regions' `keep`, the regions per motif class in BED order, the ids of the
    regions whose motif has no class)."""
    import copy
    import sys
    from . import screen as nr_screen
    reads_by_id = {id(region): reads for region, reads in zip(live, reads_of)}
    shadows, shadow_reads, shadow_at = [], [], {}
    for region in regions:
        cand = offered.get(id(region))
        if cand is None:
            continue
        if not region.no_details:
            _write_region_fastq(f"{region.out_prefix}.partial_candidates.fastq",
                                {n: (seq, qual) for n, (seq, qual, _) in cand.items()})
        if cand:
            shadow = copy.copy(region)
            shadow.read_dict, shadow.read_core_seq_dict = {}, {}
            shadow.one_anchor_reads = shadow.no_anchor_reads = shadow.skipped_reads = None
            shadow.keep_no_anchor_reads = bool(in_repeat_reads)
            shadow_at[id(region)] = len(shadows)
            shadows.append(shadow)
            shadow_reads.append({n: seq for n, (seq, _, _) in cand.items()})
    upstream.find_anchor_locations_in_reads_many(data_type, shadows, shadow_reads, num_cpu, device=device,
                                                 scoring=scoring, aligner=aligner)
    n_spanning = 0
    of, of_reads = [], []
    for region in regions:
        if id(region) not in offered:
            continue
        reads = dict(reads_by_id.get(id(region), {}))
        if id(region) in shadow_at:
            shadow = shadows[shadow_at[id(region)]]
            n_spanning += len(shadow.read_dict)
            for attr in ("one_anchor_reads", "no_anchor_reads"):
                got = getattr(shadow, attr, None)
                if got:
                    setattr(region, attr, {**(getattr(region, attr, None) or {}), **got})
            reads.update(shadow_reads[shadow_at[id(region)]])
        if reads:
            of.append(region); of_reads.append(reads)
    if n_spanning:
        print(f"NOTICE: {n_spanning} candidate read(s) hold both anchors by the anchor step though not by the screen: "
              "they are no partial reads and are left out", file=sys.stderr)
    classes = [nr_screen.motif_class(region.repeat_unit_seq) for region in regions]
    shared = [0 if c is None else sum(c == d for d in classes) for c in classes]
    unscreened = {id(region) for region, c in zip(regions, classes) if c is None}
    if in_repeat_reads and unscreened:
        print(f"NOTICE: {len(unscreened)} region(s) have a motif without a class (a root longer than 6 bases, or not "
              "ACGT): the FASTQ / FASTA command does not look for their in-repeat reads", file=sys.stderr)

    def keep(region, seq):
        return nr_screen.in_repeat_rule(seq, region.repeat_unit_seq, k, min_hits, motif_share_pct)
    return of, of_reads, keep, shared, unscreened


def _write_region_fastq(path, reads):
    """{name: (seq, qual)} as extract_fastq_from_bam writes it: a missing quality becomes '.' (Phred 13)."""
    with open(path, "w") as f:
        for name, (seq, qual) in reads.items():
            f.write(f"@{name}\n{seq}\n+\n{qual if qual is not None else '.' * len(seq)}\n")
