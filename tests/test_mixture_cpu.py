"""The GPU mixture engine without a GPU: the procedure of nanorepeat_amd/mixture.py with the numpy restatement of the
fit contract (tests/mixture_ref.py) as `mixture_engine`, against scikit-learn's procedure; windows, order and seeds;
the FASTQ command; the untouched default path; and the argument checks of nra_mixture_fit."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nanorepeat_amd import mixture, phasing, pipeline, synth
from nanorepeat_amd.round3 import Read, RepeatRegion, output_repeat_size_1d
import mixture_panel as MP
from mixture_ref import ref_mixture_fit, fit_one

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def single_thread():
    """scikit-learn's small-matrix algebra is several times slower with BLAS thread pools (pipeline.quantify_joint)."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=1):
        yield


# ---------------------------------------------------------------------------- against scikit-learn
N_1D, N_2D = 300, 30
SEED_A, SEED_B = 100, 50_000


def test_procedure_agrees_with_scikit_learn_as_scikit_learn_with_itself(single_thread):
    """D_ref: regions whose allele median sizes differ between two scikit-learn seeds; D_new: between the new
    procedure and the first of them.  Required: D_new <= max(2 D_ref, D_ref + 1 % of the regions).
    Measured (330 regions, panel seed 2024): see DESIGN.md section 17."""
    regions = MP.panel(N_1D, N_2D)
    assert sum(t[1] - t[0] in MP.EDGE_GAPS for k, _, t in regions if k == "1d") >= N_1D // 8
    assert min(len(c) for _, c, _ in regions) == 2
    ref_a = [MP.medians(phasing.run_job(j)) for j in MP.jobs_of(regions, SEED_A)]
    ref_b = [MP.medians(phasing.run_job(j)) for j in MP.jobs_of(regions, SEED_B)]
    new = [MP.medians(r) for r in mixture.phase_jobs(MP.jobs_of(regions, SEED_A), engine=ref_mixture_fit)]
    d_ref = sum(a != b for a, b in zip(ref_a, ref_b))
    d_new = sum(a != b for a, b in zip(ref_a, new))
    print(f"mixture panel: {len(regions)} regions, D_ref = {d_ref}, D_new = {d_new}")
    assert d_new <= max(2 * d_ref, d_ref + 0.01 * len(regions)), (d_ref, d_new)


def test_well_separated_alleles_get_scikit_learns_labels(single_thread):
    rng = np.random.default_rng(77)
    n = 0
    for i in range(24):
        a1 = int(rng.integers(8, 121))
        a2 = a1 + int(np.ceil(0.4 * a1 / 0.6)) + int(rng.integers(0, 20))        # gap >= 40 % of the larger size
        assert a2 - a1 >= 0.4 * a2
        sizes = np.concatenate([MP._sizes(rng, a1, int(rng.integers(6, 30))), MP._sizes(rng, a2, int(rng.integers(6, 30)))])
        counts = {f"w{i}_{j}": float(v) for j, v in enumerate(sizes)}
        job = (counts, 2, 0.07, 0.15, 22, False, 900 + i)
        want = phasing.phase_1d_job(job)
        got = mixture.phase_jobs([("1d", job)], engine=ref_mixture_fit)[0]
        assert len(got[0]) == len(want[0]) == 2
        for g, w in zip(got[0], want[0]):
            assert g.readname_list == w.readname_list and g.repeat1_median_size == w.repeat1_median_size
            assert g.confidence_list == w.confidence_list
            n += len(g.readname_list)
    assert n > 400


# ---------------------------------------------------------------------------- windows, order, seeds
def _plain(results):
    return [None if r is None else ([(a.readname_list, a.confidence_list, a.gmm_mean1, a.gmm_sd1, a.gmm_mean2, a.gmm_sd2,
                                      a.probability_list) for a in r[0]], r[1]) for r in results]


def test_windows_job_order_and_seeds(monkeypatch):
    regions = MP.panel(8, 2, seed=5)
    jobs = MP.jobs_of(regions, 300, max_num_components=6)
    calls = []

    def engine(*a, **k):
        calls.append(sorted(set(np.asarray(a[5]).tolist())))
        return ref_mixture_fit(*a, **k)

    base = _plain(mixture.phase_jobs(jobs, engine=engine))
    assert calls[0] == [2, 3] and all(len(c) <= 2 for c in calls)
    # one order per call, and every order up to the stop in one call
    for window in (1, 22):
        monkeypatch.setattr(mixture, "WINDOW", window)
        del calls[:]
        assert _plain(mixture.phase_jobs(jobs, engine=engine)) == base
        assert calls[0] == ([2] if window == 1 else [2, 3, 4, 5, 6])
    monkeypatch.undo()
    # the jobs in another order: the same result per region
    order = np.random.default_rng(1).permutation(len(jobs))
    shuffled = _plain(mixture.phase_jobs([jobs[i] for i in order], engine=ref_mixture_fit))
    assert [shuffled[list(order).index(i)] for i in range(len(jobs))] == base
    # the same seed twice: identical; another seed: another sample
    assert _plain(mixture.phase_jobs(jobs, engine=ref_mixture_fit)) == base
    x = np.array([[20.0], [21.0], [40.0]])
    assert np.array_equal(mixture.sample(x, 0.07, 5), mixture.sample(x, 0.07, 5))
    assert not np.array_equal(mixture.sample(x, 0.07, 5), mixture.sample(x, 0.07, 6))
    assert not np.array_equal(mixture.sample(x, 0.07, 5), mixture.sample(x, 0.07, 5, restart=1))


def test_sample_and_starts_follow_the_contract():
    x = np.array([[20.0, 7.0], [21.5, 8.0], [40.0, 9.0]])
    m, d, e, s = 3, 2, 0.1, 11
    z = np.random.default_rng(s).standard_normal(100 * m * d)
    flat = x.ravel()
    want = np.array([flat[k % (m * d)] + z[k] * e * (10 + flat[k % (m * d)]) for k in range(100 * m * d)]).reshape(-1, d)
    assert np.array_equal(mixture.sample(x, e, s), want)
    rows = mixture.start_rows(s, 4, 7, 300)
    assert np.array_equal(rows, np.random.default_rng([s, 4, 7]).choice(300, size=4, replace=False))
    assert len(set(rows.tolist())) == 4
    one = mixture.one_component(want)
    assert np.allclose(one.means_[0], want.mean(axis=0)) and np.allclose(one.covariances_[0], want.var(axis=0) + 1e-6)
    # the order rule: touching intervals overlap (sd floored at 1)
    import statistics
    zo = statistics.NormalDist().inv_cdf(0.85)
    touching = mixture.FittedMixture([0.5, 0.5], [[10.0], [10.0 + 2 * zo]], [[0.25], [1.0]])
    assert mixture.components_overlap(touching, 0.15)
    apart = mixture.FittedMixture([0.5, 0.5], [[10.0], [10.0 + 2 * zo + 1e-9]], [[0.25], [1.0]])
    assert not mixture.components_overlap(apart, 0.15)


def test_restatement_has_no_knife_edge_on_the_gpu_tests_problems():
    """tests/test_mixture_gpu.py compares discrete outputs fit by fit; the panel's seed is chosen so that no fit of the
    restatement comes within 1e-9 of the stop test's tolerance.  Two starts of a (problem, order) within 1e-12 of each
    other's lb cannot be avoided by a seed: starts that reach the same Lloyd labels are the same fit with its
    components in another order.  Such starts must then be the same mixture, so that it does not matter which of them
    is called the best; the GPU test accepts any start of the restatement's tie set and nothing else."""
    args = MP.fit_problems(200)
    ref = ref_mixture_fit(*args, detail=True)
    assert len(ref["lb"]) == 2000
    assert (ref["margin"] >= 1e-9).all(), int((ref["margin"] < 1e-9).sum())
    assert set(args[3].tolist()) == {1, 2} and set(args[5].tolist()) == {2, 3, 4, 5, 6}
    assert args[2].min() >= 200 and args[2].max() <= 4000
    n_tied = 0
    for g in range(0, 2000, mixture.N_STARTS):
        lb = ref["lb"][g:g + mixture.N_STARTS]
        tied = [g + t for t in np.flatnonzero(lb.max() - lb <= 1e-12)]
        n_tied += len(tied) > 1
        first = np.sort(ref["w"][ref["off"][tied[0]]:ref["off"][tied[0] + 1]])
        for f in tied[1:]:
            assert np.allclose(np.sort(ref["w"][ref["off"][f]:ref["off"][f + 1]]), first, rtol=0, atol=1e-9)
    print(f"(problem, order) pairs whose best lb is shared by several starts: {n_tied} of 200")


def test_fit_one_hand_cases():
    # two tight groups from starts in each: means and weights come out, EM stops at its second step
    X = np.array([[0.0], [0.1], [-0.1], [10.0], [10.1], [9.9], [10.0], [10.0]])
    got = fit_one(X, [0, 3])
    assert got["converged"] == 1 and got["n_iter"] == 2
    assert np.allclose(got["mu"][:, 0], [0.0, 10.0]) and np.allclose(got["w"], [3 / 8, 5 / 8])
    assert np.allclose(got["var"][:, 0], [0.02 / 3 + 1e-6, 0.02 / 5 + 1e-6])
    # both starts in one group: Lloyd moves one of them over
    got = fit_one(X, [3, 4])
    assert sorted(np.round(got["mu"][:, 0], 6)) == [0.0, 10.0]
    # as many components as points
    got = fit_one(X[:4], [0, 1, 2, 3])
    assert np.allclose(got["var"], 1e-6) and np.allclose(got["w"], 0.25)


# ---------------------------------------------------------------------------- the command
def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _rows(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l]


def test_fastq_command_with_the_restatement_as_engine(oracle, tmp_path, single_thread):
    from screen_ref import RefScreen
    p = synth.panel(6, anchor_len=400, reads_per_region=14, n_decoys=6, seed=3)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont_q20", anchor_len=400, seed=1, aligner=oracle.align_pairs, scorer=oracle.round3_1d,
                  screener=RefScreen)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "sk"), **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "new"), mixture="gpu", mixture_engine=ref_mixture_fit,
                                 **common)
    want, got = _tree(tmp_path / "sk.details"), _tree(tmp_path / "new.details")
    assert sorted(want) == sorted(got)                            # every existing file is written
    assert any(n.endswith(".phased_reads.txt") for n in got) and any(n.endswith(".summary.txt") for n in got)
    alleles = {}
    for name, (g, k) in p["truth"].items():
        alleles.setdefault(g, set()).add(k)
    n_checked = 0
    for g, (a, b) in enumerate(zip(_rows(tmp_path / "sk.NanoRepeat_output.tsv"), _rows(tmp_path / "new.NanoRepeat_output.tsv"))):
        assert a[:4] == b[:4]
        lo, hi = min(alleles[g]), max(alleles[g])
        if hi - lo >= 0.4 * hi:                                   # well separated
            assert a[4] == b[4] == "2" and a[7] == b[7], g        # Num_Alleles, allele sizes and read counts
            n_checked += 1
    assert n_checked >= 2
    # a run is a function of its seed
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "again"), mixture="gpu",
                                 mixture_engine=ref_mixture_fit, **common)
    assert _tree(tmp_path / "again.details") == got
    assert (tmp_path / "again.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "new.NanoRepeat_output.tsv").read_bytes()


# ---------------------------------------------------------------------------- the default path
def _golden_region(case, tmp_path, stem):
    rr = RepeatRegion("chr4\t3074876\t3074933\tCAG")
    rr.out_prefix = str(tmp_path / stem)
    rr.region_fq_file = str(tmp_path / (stem + ".fastq"))
    with open(rr.region_fq_file, "w") as f:
        for name, size in case["reads"]:
            rd = Read(name)
            rd.round3_repeat_size = size
            rr.read_dict[name] = rd
            f.write(f"@{name} len=8\nACGTACGT\n+\nIIIIIIII\n")
    output_repeat_size_1d(rr)
    return rr


@pytest.mark.parametrize("keyword", [{}, {"mixture": "sklearn"}])
def test_default_engine_gives_the_golden_files(tmp_path, keyword, single_thread):
    from test_phasing import _files
    from nanorepeat_amd import joint
    fx = json.load(open(os.path.join(HERE, "golden", "ref_phasing.json")))
    n = 0
    for ci, case in enumerate(fx["cases_1d"]):
        par = case["params"]
        if par["error_rate"] != 0.07:                             # phase_regions takes the data type's rate
            continue
        stem = f"ph1_{ci}"
        rr = _golden_region(case, tmp_path, stem)
        rows = pipeline.phase_regions([rr], "ont", par["ploidy"], par["max_mutual_overlap"], par["max_num_components"],
                                      par["remove_noisy_reads"], seed=case["seed"], n_jobs=1 + ci % 2, **keyword)
        assert _files(tmp_path, stem) == case["files"], case["label"]
        assert rows == [case["final_output"]], case["label"]
        n += 1
    assert n >= 5
    r1 = joint.Repeat().init_from_string("chr4:3074876:3074933:CAG:200")
    r2 = joint.Repeat().init_from_string("chr4:3074946:3074966:CCG:20")
    for ci, case in enumerate(fx["cases_2d"]):                   # quantify_joint's fit: the job it builds, in a worker
        stem = f"ph2_{ci}"
        fq = str(tmp_path / (stem + ".fastq"))
        with open(fq, "w") as f:
            for name, a, b in case["reads"]:
                f.write(f"@{name}\nACGTACGTAC\n+\nIIIIIIIIII\n")
        counts = {name: (a, b) for name, a, b in case["reads"]}
        par = case["params"]
        job = ("2d", (counts, par["ploidy"], par["error_rate"], par["max_mutual_overlap"], par["max_num_components"],
                      par["remove_noisy_reads"], case["seed"]))
        fitted = pipeline._fit_in_worker_processes([job], 1)[0]
        phasing.split_alleles_using_gmm_2d(par["ploidy"], par["error_rate"], par["max_mutual_overlap"],
                                           par["remove_noisy_reads"], par["max_num_components"], r1, r2, counts, 0,
                                           fq, str(tmp_path / stem), seed=case["seed"], fitted=fitted)
        assert _files(tmp_path, stem, (fq, "IN.fastq")) == case["files"], case["label"]


def test_gpu_engine_imports_neither_scikit_learn_nor_scipy(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(f"""
import sys
sys.path[:0] = [{ROOT!r}, {HERE!r}]
from nanorepeat_amd import pipeline, phasing
from nanorepeat_amd.round3 import Read, RepeatRegion
from mixture_ref import ref_mixture_fit
regions = []
for g, sizes in enumerate(([20.0] * 9 + [20.5] * 6 + [41.0] * 8 + [40.5] * 7, [33.0, 33.5], [12.0])):
    rr = RepeatRegion(f"chr1\\t{{1000 * g + 100}}\\t{{1000 * g + 130}}\\tCAG")
    rr.out_prefix, rr.no_details = {str(tmp_path)!r} + f"/c{{g}}", False
    for i, v in enumerate(sizes):
        rd = Read(f"r{{g}}_{{i}}")
        rd.round3_repeat_size = v
        rr.read_dict[f"r{{g}}_{{i}}"] = rd
    regions.append(rr)
rows = pipeline.phase_regions(regions, seed=3, mixture="gpu", mixture_engine=ref_mixture_fit)
assert [r.split("\\t")[4] for r in rows][::2] == ["2", "0"], rows
bad = sorted(m for m in sys.modules if m.split(".")[0] in ("sklearn", "scipy"))
assert not bad, bad
print("ok")
""")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_unknown_engine_is_a_value_error(tmp_path):
    with pytest.raises(ValueError):
        pipeline.phase_regions([], mixture="tpu")
    for command in (pipeline.quantify_from_reads, pipeline.quantify_from_bam):
        with pytest.raises(ValueError, match="mixture"):
            command(str(tmp_path / "none"), str(tmp_path / "none.fa"), str(tmp_path / "none.bed"), str(tmp_path / "o"),
                    mixture="tpu")
    with pytest.raises(ValueError, match="mixture"):
        pipeline.quantify_joint(str(tmp_path / "none.fq"), str(tmp_path / "none.fa"), "chr4:1:2:CAG:20", "chr4:5:9:CCG:20",
                                str(tmp_path / "o"), mixture="tpu")


# ---------------------------------------------------------------------------- the C ABI
def _good():
    X = np.arange(24, dtype=np.float64)
    return dict(samples=X, prob_off=[0, 4], prob_n=[12, 10], prob_d=[2, 1], fit_problem=[0, 1], fit_n=[2, 3],
                starts=[0, 5, 1, 2, 9])


def test_symbol_is_exported_and_listed(capi):
    assert "nra_mixture_fit" in capi.EXPORTS
    assert hasattr(C.CDLL(capi.LIB_PATH), "nra_mixture_fit")
    assert capi.load().nra_abi_version() == 4


def test_mixture_fit_checks_arguments_and_needs_a_device(capi):
    """Arguments are checked before the device is touched; with good arguments and no device the call returns
    NRA_E_DEVICE.  Skipped where a GPU is present: the GPU suite covers the call there."""
    if capi.load().nra_device_count() > 0:
        pytest.skip("a HIP device is present")
    cases = [(dict(prob_d=[3, 1]), -1), (dict(prob_d=[2, 0]), -1), (dict(fit_n=[0, 3], starts=[1, 2, 9]), -1),
             (dict(fit_n=[2, 11], starts=[0, 5] + list(range(10)) + [0]), -1),              # n > N
             (dict(starts=[0, 12, 1, 2, 9]), -1), (dict(starts=[0, 5, 1, 2, 10]), -1),          # a start row >= N
             (dict(starts=[0, -1, 1, 2, 9]), -1), (dict(fit_problem=[0, 2]), -1),
             (dict(prob_off=[0, 15]), -1),                                                   # rows outside the samples
             (dict(samples=np.where(np.arange(24) == 7, np.nan, np.arange(24.0))), -1),
             (dict(samples=np.where(np.arange(24) == 23, np.inf, np.arange(24.0))), -1),
             (dict(flags=4), -1)]
    for change, code in cases:
        with pytest.raises(capi.NraError) as e:
            capi.mixture_fit(**{**_good(), **change})
        assert e.value.code == code, change
    big = np.zeros(40)
    with pytest.raises(capi.NraError) as e:                      # n = 33
        capi.mixture_fit(big, [0], [40], [1], [0], [33], list(range(33)))
    assert e.value.code == -3
    lib = capi.load()
    one = np.zeros(1)
    po, pn, pd = np.zeros(1, np.int64), np.array([(1 << 22) + 1], np.int32), np.ones(1, np.int32)
    # N beyond the limit is refused before a single row is read
    assert lib.nra_mixture_fit(0, 1 << 23, capi._ptr(one, C.c_double), 1, capi._ptr(po, C.c_int64),
                               capi._ptr(pn, C.c_int32), capi._ptr(pd, C.c_int32), 0, *(None,) * 3, 0, *(None,) * 6) == -3
    assert lib.nra_mixture_fit(0, -1, None, 0, None, None, None, 0, *(None,) * 3, 0, *(None,) * 6) == -1
    with pytest.raises(capi.NraError) as e:
        capi.mixture_fit(**_good())
    assert e.value.code == -2 and "no HIP device" in str(e.value)
    with pytest.raises(capi.NraError) as e:                      # the product has no CPU path
        pipeline.phase_regions([_two_allele_region()], seed=1, mixture="gpu")
    assert e.value.code == -2


def _two_allele_region():
    rr = RepeatRegion("chr1\t100\t130\tCAG")
    rr.out_prefix = None
    for i, v in enumerate([20.0] * 9 + [41.0] * 8):
        rd = Read(f"r{i}")
        rd.round3_repeat_size = v
        rr.read_dict[f"r{i}"] = rd
    return rr
