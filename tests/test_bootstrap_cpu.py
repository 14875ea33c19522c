"""The bootstrap (`bootstrap=B`) without a device: the vectorised alleles-of-replicates against the
per-replicate restatement through phasing, the sample formula, the percentile rule, the degenerate regions, and
phase_regions' files.  The engine is bootstrap_ref.composed_engine over the numpy restatement of the fit."""
import os

import numpy as np
import pytest

from nanorepeat_amd import bootstrap, mixture, phasing, pipeline
from nanorepeat_amd.round3 import Read, RepeatRegion
import mixture_panel as MP
from bootstrap_ref import alleles_of_replicate, composed_engine, limit_cases, replicate_sample
from mixture_ref import ref_mixture_fit

B = 8
ENGINES = dict(mixture_engine=ref_mixture_fit, bootstrap_engine=composed_engine(ref_mixture_fit))


def _region(g, sizes, root=None):
    rr = RepeatRegion(f"chr1\t{1000 * g + 100}\t{1000 * g + 130}\tCAG")
    rr.out_prefix, rr.no_details = (os.path.join(str(root), f"c{g}") if root else None), root is None
    for i, v in enumerate(sizes):
        rd = Read(f"r{g}_{i}")
        rd.round3_repeat_size = float(v)
        rr.read_dict[f"r{g}_{i}"] = rd
    return rr


def _tree(root):
    return {fn: open(os.path.join(str(root), fn), "rb").read() for fn in sorted(os.listdir(str(root)))}


# ---------------------------------------------------------------------------- alleles of replicates
@pytest.fixture(scope="module")
def panel_bootstrap():
    """20 small 1D regions (two of them of two reads), solved and bootstrapped once: [(problem, replicates)]."""
    regions = MP.panel(19, 0)
    jobs = MP.jobs_of(regions, seed=50, max_num_components=6)
    jobs.append(("1d", ({"a": 33.0, "b": 33.5}, 2, 0.07, 0.15, 6, False, 77)))
    problems = []
    mixture.phase_jobs(jobs, engine=ref_mixture_fit, problems_out=problems)
    assert len(problems) == 20 and all(p is not None for p in problems)
    assert sum(len(p.x) == 2 for p in problems) >= 1
    return list(zip(problems, mixture.bootstrap(problems, B, ENGINES["bootstrap_engine"])))


def _per_replicate(x, rep, ploidy, noisy):
    return [alleles_of_replicate(x, rep["idx"][b], int(rep["order"][b]), rep["w"][b], rep["mu"][b], rep["var"][b],
                                 ploidy, noisy) for b in range(len(rep["idx"]))]


def _assert_same(x, rep, ploidy, noisy):
    count, sizes = bootstrap.alleles_of_replicates(x, rep, ploidy, noisy)
    want = _per_replicate(x, rep, ploidy, noisy)
    assert [int(c) for c in count] == [len(w) for w in want]
    assert [[int(s) for s in row[:c]] for row, c in zip(sizes, count)] == want
    assert all((row[c:] == -1).all() for row, c in zip(sizes, count))
    return want


@pytest.mark.parametrize("noisy", [False, True])
def test_vectorised_alleles_equal_the_per_replicate_restatement(panel_bootstrap, noisy):
    orders = set()
    for p, rep in panel_bootstrap:
        assert (rep["status"] == mixture.BOOT_DECIDED).all()
        _assert_same(p.x[:, 0], rep, 2, noisy)
        orders.update(int(o) for o in rep["order"])
    assert {1, 2} <= orders


@pytest.mark.parametrize("noisy", [False, True])
def test_empty_components_and_noisy_alleles_by_hand(noisy):
    """Replicates made by hand: a component without reads, three alleles of which the count rule removes one, a tie
    of counts, and a median between two reads."""
    x = np.array([20.0, 20.5, 21.0, 19.5, 20.0, 40.0, 41.0, 60.5, 61.0, 59.5])
    idx = np.array([[0, 1, 2, 3, 4, 0, 1, 2, 3, 4],            # nobody in components 1 and 2
                    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9],            # 5, 2, 3 reads
                    [0, 1, 2, 3, 5, 5, 6, 7, 8, 9],            # 4, 3, 3
                    [0, 1, 2, 3, 4, 0, 1, 5, 7, 8],            # 7, 1, 2: the count rule drops the middle one
                    [5, 6, 5, 6, 5, 6, 7, 7, 8, 9]])           # 0, 6, 4
    n = len(idx)
    rep = dict(idx=idx, status=np.zeros(n, np.int32), order=np.full(n, 3, np.int32),
               w=np.tile([0.5, 0.2, 0.3], (n, 1)), mu=np.tile([20.2, 40.5, 60.3], (n, 1))[:, :, None],
               var=np.tile([0.4, 0.5, 0.6], (n, 1))[:, :, None])
    want = _assert_same(x, rep, 2, noisy)
    assert want[0] == [20] and want[1] == ([20, 61] if noisy else [20, 41, 61])
    assert want[3] == ([20, 61] if noisy else [20, 40, 61]) and want[4] == [41, 61]
    assert want[2] == [20, 40, 61]                             # 3 * 1.5 > 3: nothing goes
    # the means out of order, an order-1 replicate and one that is not decided
    rep2 = dict(idx=idx[1:4], status=np.array([0, 0, 1], np.int32), order=np.array([3, 1, 0], np.int32),
                w=np.array([[0.3, 0.5, 0.2], [0, 0, 0], [0, 0, 0]]),
                mu=np.array([[60.3, 20.2, 40.5], [0, 0, 0], [0, 0, 0]])[:, :, None],
                var=np.array([[0.6, 0.4, 0.5], [0, 0, 0], [0, 0, 0]])[:, :, None])
    count, sizes = bootstrap.alleles_of_replicates(x, rep2, 2, noisy)
    assert list(count) == [2 if noisy else 3, 1, -1]
    assert list(sizes[0]) == ([20, 61, -1] if noisy else [20, 41, 61])
    assert list(sizes[1]) == [int(np.median(x[idx[2]]) + 0.5), -1, -1] and (sizes[2] == -1).all()


def test_identity_resample_is_the_problems_own_sample():
    rng = np.random.default_rng(5)
    for d, m in ((1, 2), (1, 37), (2, 11), (2, 52)):
        x = np.round(rng.uniform(5, 90, size=(m, d)), 1)
        p = mixture.Problem(x, 0.07, 0.15, 6, seed=90 + m)
        got = replicate_sample(p.x, p.z, p.error_rate, np.arange(m))
        assert got.shape == p.X.shape and got.tobytes() == p.X.tobytes()
        assert np.array_equal(mixture.sample(x, 0.07, 90 + m), p.X)
    # the noise belongs to the position: a read drawn twice gets two different sets of copies
    twice = replicate_sample(p.x, p.z, p.error_rate, np.zeros(m, np.int64))
    assert len(np.unique(twice[:, 0])) == len(twice)
    assert np.array_equal(mixture.resample_indices(7, 5, 3),
                          np.random.default_rng([7, 0x626F6F74]).integers(0, 5, size=(3, 5)))


def test_percentiles_follow_the_nearest_rank_rule():
    """q = 0.025: (floor(q (r - 1)), ceil((1 - q) (r - 1))) by hand."""
    table = {1: (0, 0), 2: (0, 1), 40: (0, 39), 200: (4, 195)}     # 0.025 * 199 = 4.975, 0.975 * 199 = 194.025
    for r, (lo, hi) in table.items():
        v = np.random.default_rng(r).permutation(r) * 3 + 7
        assert bootstrap.percentile_interval(v) == (3 * lo + 7, 3 * hi + 7), r
    assert bootstrap.percentile_interval(np.arange(200), 0.5) == (49, 150)    # 0.25 * 199 = 49.75, 149.25
    assert bootstrap.percentile_interval([]) is None


# ---------------------------------------------------------------------------- degenerate regions
def test_all_reads_equal_gives_one_allele_of_that_size():
    rr = _region(0, [30.0] * 12)
    pipeline.phase_regions([rr], seed=11, mixture="gpu", bootstrap=B, **ENGINES)
    boot = rr.bootstrap
    assert (boot.count == 1).all() and (boot.sizes[:, 0] == 30).all() and (boot.sizes[:, 1:] == -1).all()
    assert boot.rows == [(30, 12, 30, 30, B)] and boot.support == 1.0 and boot.distribution == f"1:{B}"


def test_two_alleles_of_20_and_60():
    rr = _region(0, [20.0] * 10 + [60.0] * 10)
    pipeline.phase_regions([rr], "hifi", seed=12, mixture="gpu", bootstrap=B, **ENGINES)
    boot = rr.bootstrap
    assert [a.repeat_size1 for a in rr.results.quantified_allele_list] == [20, 60]
    assert boot.rows == [(20, 10, 20, 20, B), (60, 10, 60, 60, B)]
    assert boot.support == 1.0 and boot.n_replicates == B


# ---------------------------------------------------------------------------- the command's files
SIZES = ([20.0] * 9 + [20.5] * 6 + [41.0] * 8 + [40.5] * 7, [33.0, 33.5], [12.0],
         [15.0, 15.5, 16.0, 15.0, 14.5, 15.0, 15.5, 15.0])


def _run(root, name, **kw):
    out = root / name
    out.mkdir()
    regions = [_region(g, sizes, out) for g, sizes in enumerate(SIZES)]
    pipeline.phase_regions(regions, seed=3, out_tsv_file=str(out / "out.tsv"), **kw)
    return regions, _tree(out)


def test_off_is_the_default_and_needs_the_gpu_engine(tmp_path):
    _, absent = _run(tmp_path, "absent", mixture="gpu", mixture_engine=ref_mixture_fit)
    _, zero = _run(tmp_path, "zero", mixture="gpu", mixture_engine=ref_mixture_fit, bootstrap=0,
                   bootstrap_tsv_file=str(tmp_path / "zero" / "boot.tsv"))
    assert absent == zero and not any("boot" in fn for fn in zero)
    with pytest.raises(ValueError, match="bootstrap"):
        pipeline.phase_regions([_region(0, SIZES[0])], seed=3, mixture="sklearn", bootstrap=8)
    with pytest.raises(ValueError, match="bootstrap"):
        pipeline.phase_regions([], mixture="gpu", bootstrap=-1)
    for command in (pipeline.quantify_from_reads, pipeline.quantify_from_bam):
        with pytest.raises(ValueError, match="bootstrap"):
            command(str(tmp_path / "none"), str(tmp_path / "none.fa"), str(tmp_path / "none.bed"), str(tmp_path / "o"),
                    bootstrap=8)


def test_files_end_to_end_and_the_same_seed_gives_the_same_bytes(tmp_path):
    _, plain = _run(tmp_path, "plain", mixture="gpu", mixture_engine=ref_mixture_fit)
    regions, boot = _run(tmp_path, "boot", mixture="gpu", bootstrap=B,
                         bootstrap_tsv_file=str(tmp_path / "boot" / "boot.tsv"), **ENGINES)
    new = sorted(set(boot) - set(plain))
    assert new == ["boot.tsv", "c0.bootstrap.tsv", "c1.bootstrap.tsv", "c3.bootstrap.tsv"]
    assert {fn: boot[fn] for fn in plain} == plain
    lines = boot["c0.bootstrap.tsv"].decode().split("\n")
    assert lines[0] == "##RepeatRegion=" + regions[0].to_unique_id() and lines[1] == "##Seed=3"
    assert lines[2].split("\t") == ["#Replicate", "Num_Alleles", "Allele_Sizes"]
    rows = [l.split("\t") for l in lines[3:] if l]
    assert [r[0] for r in rows] == [str(b) for b in range(B)]
    assert all(len(r[2].split(",")) == int(r[1]) for r in rows)
    assert boot["c1.bootstrap.tsv"].decode().split("\n")[1] == "##Seed=4"
    table = [l.split("\t") for l in boot["boot.tsv"].decode().split("\n") if l]
    assert table[0] == ["#Chrom", "Start", "End", "Motif", "Allele", "Repeat_Size", "Num_Reads", "CI_Low", "CI_High",
                        "Replicates_Used", "Num_Replicates", "Count_Support", "Count_Distribution"]
    assert all(len(r) == 13 for r in table)
    by_region = {}
    for r in table[1:]:
        by_region.setdefault(r[1], []).append(r)
    assert [len(v) for v in by_region.values()] == [len(rg.results.quantified_allele_list) or 1 for rg in regions]
    assert by_region["2100"] == [["chr1", "2100", "2130", "CAG"] + ["-"] * 9]          # one read: no call
    for r in by_region["100"]:
        assert r[5] in ("20", "41") and int(r[7]) <= int(r[5]) <= int(r[8]) and r[10] == str(B)
        assert sum(int(kv.split(":")[1]) for kv in r[12].split(",")) == B
        assert float(r[11]) == int(r[9]) / B
    _, again = _run(tmp_path, "again", mixture="gpu", bootstrap=B,
                    bootstrap_tsv_file=str(tmp_path / "again" / "boot.tsv"), **ENGINES)
    assert again == boot


# ---------------------------------------------------------------------------- the C ABI
def test_symbol_is_exported_and_arguments_are_checked_before_the_device(capi):
    """Every refusal comes before the device is touched, so it is the same with and without one; good arguments
    succeed on a GPU and return NRA_E_DEVICE without."""
    assert "nra_mixture_bootstrap" in capi.EXPORTS and capi.load().nra_abi_version() == 4
    good, cases = limit_cases(capi.boot_start_rows)
    for change, code in cases:
        with pytest.raises(capi.NraError) as e:
            capi.mixture_bootstrap(**{**good, **change})
        assert e.value.code == code, change
    if capi.load().nra_device_count() > 0:
        assert capi.mixture_bootstrap(**good)["status"].shape == (1, 2)
    else:
        with pytest.raises(capi.NraError) as e:
            capi.mixture_bootstrap(**good)
        assert e.value.code == -2 and "no HIP device" in str(e.value)
        with pytest.raises(capi.NraError) as e:                  # the product has no CPU path
            pipeline.phase_regions([_region(0, SIZES[0])], seed=1, mixture="gpu", mixture_engine=ref_mixture_fit,
                                   bootstrap=B)
        assert e.value.code == -2
