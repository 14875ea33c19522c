"""The mixture fits on the MI355X, through the C ABI only: nra_mixture_fit against the numpy restatement of its
contract fit by fit, bit-level determinism across runs, batch orders and kernel paths, the limits, and the commands
end to end with mixture="gpu".

Continuous outputs (lb, w, mu, var): the largest relative difference from the restatement measured on this file's
problem set on one MI355X is recorded in DESIGN.md section 17; TOLERANCE is 100 times it, capped at 1e-6."""
import os
import sys

import numpy as np
import pytest

from nanorepeat_amd import mixture, synth
import mixture_panel as MP
from mixture_ref import ref_mixture_fit

pytestmark = pytest.mark.gpu

MEASURED = 2.657e-9                         # largest relative difference on this file's problems, one MI355X
TOLERANCE = min(100 * MEASURED, 1e-6)
REG_MAX = 256 * 20                           # the largest N the register path takes (NRA_MIX_THREADS * NRA_MIX_KREG)
FIELDS = ("lb", "w", "mu", "var")


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


def _compare(got, ref, what):
    """Discrete outputs equal on every fit whose stop test is not a knife edge in the restatement (at most 1 % may be);
    the best start equal, or one of the restatement's starts that share the best lb to 1e-12 (the same fit with its
    components in another order: tests/test_mixture_cpu.py); continuous outputs within TOLERANCE.  Returns the
    largest relative difference."""
    edge = ref["margin"] < 1e-9
    assert edge.sum() <= 0.01 * len(edge), (what, int(edge.sum()))
    ok = ~edge
    assert np.array_equal(got["n_iter"][ok], ref["n_iter"][ok]), what
    assert np.array_equal(got["converged"][ok], ref["converged"][ok]), what
    same = ok & (got["n_iter"] == ref["n_iter"])
    worst = 0.0
    for f in np.flatnonzero(same):
        o = slice(int(ref["off"][f]), int(ref["off"][f + 1]))
        worst = max(worst, _rel(got["lb"][f], ref["lb"][f]), _rel(got["w"][o], ref["w"][o]))
        for key in ("mu", "var"):
            keep = ref[key][o] != 0                               # the unused second axis of a 1D fit is 0 in both
            assert np.array_equal(got[key][o] != 0, keep), (what, f, key)
            worst = max(worst, _rel(got[key][o][keep], ref[key][o][keep]))
    print(f"{what}: {int(same.sum())} fits, largest relative difference {worst:.3e}")
    for g in range(0, len(edge) - len(edge) % mixture.N_STARTS, mixture.N_STARTS):
        sl = slice(g, g + mixture.N_STARTS)
        if edge[sl].any():
            continue
        tied = np.flatnonzero(ref["lb"][sl].max() - ref["lb"][sl] <= 1e-12)
        assert int(np.argmax(got["lb"][sl])) in tied, (what, g)
        if len(tied) == 1:
            assert int(np.argmax(got["lb"][sl])) == int(np.argmax(ref["lb"][sl]))
    assert worst <= TOLERANCE, (what, worst)
    return worst


def _bits(out, f):
    o = slice(int(out["off"][f]), int(out["off"][f + 1]))
    return (out["lb"][f].tobytes(), int(out["n_iter"][f]), int(out["converged"][f]), out["w"][o].tobytes(),
            out["mu"][o].tobytes(), out["var"][o].tobytes())


@pytest.fixture(scope="module")
def problems200():
    return MP.fit_problems(200)


def test_device_equals_restatement_fit_by_fit(capi, problems200):
    got = capi.mixture_fit(*problems200)
    ref = ref_mixture_fit(*problems200, detail=True)
    assert len(got["lb"]) == 2000 and got["converged"].sum() > 1500
    _compare(got, ref, "200 problems")


def _large(N, d, n, seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(10, 120, size=(n, d)) + 40 * np.arange(n)[:, None]
    which = rng.integers(0, n, N)
    X = centres[which] + rng.standard_normal((N, d)) * (0.07 * (10 + centres[which]))
    starts = np.concatenate([np.random.default_rng([seed, n, t]).choice(N, size=n, replace=False)
                             for t in range(mixture.N_STARTS)])
    return X.ravel(), [0], [N], [d], [0] * mixture.N_STARTS, [n] * mixture.N_STARTS, starts


@pytest.mark.parametrize("N,d,n", [(100_000, 1, 3), (100_000, 2, 4), (REG_MAX - 1, 1, 3), (REG_MAX, 2, 2),
                                   (REG_MAX + 1, 1, 4), (REG_MAX + 1, 2, 3), (1024, 1, 2), (1025, 2, 3)])
def test_large_problems_and_the_border_of_the_register_path(capi, N, d, n):
    args = _large(N, d, n, seed=N + d)
    got = capi.mixture_fit(*args)
    _compare(got, ref_mixture_fit(*args, detail=True), f"N = {N}, d = {d}, n = {n}")
    # the same bits whichever kernel runs the problem
    for flags in (capi.MIX_STREAM, capi.MIX_ONE_CLASS):
        other = capi.mixture_fit(*args, flags=flags)
        assert all(_bits(other, f) == _bits(got, f) for f in range(len(got["lb"]))), flags


def test_identical_bits_twice_reversed_alone_and_streamed(capi, problems200):
    samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts = problems200
    nf = 600                                                      # the first 60 problems
    off = np.concatenate([[0], np.cumsum(fit_n)])
    cut = (samples, prob_off, prob_n, prob_d, fit_problem[:nf], fit_n[:nf], starts[:off[nf]])
    a = capi.mixture_fit(*cut)
    b = capi.mixture_fit(*cut)
    assert all(_bits(a, f) == _bits(b, f) for f in range(nf))
    order = np.arange(nf)[::-1]
    rev_starts = np.concatenate([starts[off[f]:off[f + 1]] for f in order])
    r = capi.mixture_fit(samples, prob_off, prob_n, prob_d, fit_problem[order], fit_n[order], rev_starts)
    assert all(_bits(r, nf - 1 - f) == _bits(a, f) for f in range(nf))
    s = capi.mixture_fit(*cut, flags=capi.MIX_STREAM)
    assert all(_bits(s, f) == _bits(a, f) for f in range(nf))
    for p in range(0, 60, 3):                                     # a problem alone, from a buffer of its own
        N, d = int(prob_n[p]), int(prob_d[p])
        fs = np.flatnonzero(fit_problem[:nf] == p)
        alone = capi.mixture_fit(samples[prob_off[p]:prob_off[p] + N * d].copy(), [0], [N], [d], [0] * len(fs),
                                 fit_n[fs], np.concatenate([starts[off[f]:off[f + 1]] for f in fs]))
        assert all(_bits(alone, i) == _bits(a, f) for i, f in enumerate(fs)), p


def test_limits(capi):
    with pytest.raises(capi.NraError) as e:
        capi.mixture_fit(np.zeros(40), [0], [40], [1], [0], [33], list(range(33)))
    assert e.value.code == -3
    import ctypes as C
    one = np.zeros(1)
    po, pn, pd = np.zeros(1, np.int64), np.array([(1 << 22) + 1], np.int32), np.ones(1, np.int32)
    assert capi.load().nra_mixture_fit(0, 1 << 23, capi._ptr(one, C.c_double), 1, capi._ptr(po, C.c_int64),
                                       capi._ptr(pn, C.c_int32), capi._ptr(pd, C.c_int32), 0, *(None,) * 3, 0,
                                       *(None,) * 6) == -3
    for bad in (dict(prob_d=[3]), dict(fit_n=[0], starts=[]), dict(starts=[0, 200])):
        args = dict(samples=np.arange(200.0), prob_off=[0], prob_n=[200], prob_d=[1], fit_problem=[0], fit_n=[2],
                    starts=[0, 1])
        with pytest.raises(capi.NraError) as e:
            capi.mixture_fit(**{**args, **bad})
        assert e.value.code == -1, bad
    # a problem of two reads (N = 200), and as many components as points
    X = mixture.sample(np.array([[20.0], [31.0]]), 0.07, 4)
    args = (X.ravel(), [0], [200], [1], [0, 0], [2, 3], [5, 150, 0, 1, 2])
    _compare(capi.mixture_fit(*args), ref_mixture_fit(*args, detail=True), "two reads")
    pts = np.array([3.0, 9.5, 20.0, 20.5, 41.0, 77.0, 78.0, 120.0])
    for n_pts in (1, 2, 8):
        args = (pts[:n_pts], [0], [n_pts], [1], [0], [n_pts], list(range(n_pts))[::-1])
        got = capi.mixture_fit(*args)
        ref = ref_mixture_fit(*args, detail=True)
        assert got["n_iter"][0] == ref["n_iter"][0] and np.allclose(np.sort(got["mu"][:, 0]), pts[:n_pts])
        assert np.allclose(got["var"][:, 0], 1e-6) and np.allclose(got["w"], 1.0 / n_pts)
    assert len(capi.mixture_fit(pts, [0], [8], [1], [], [], [])["lb"]) == 0


# ---------------------------------------------------------------------------- end to end
def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _rows(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l]


def test_fastq_command_gpu_engine_equals_restatement_and_default(capi, tmp_path):
    from nanorepeat_amd import pipeline
    p = synth.panel(12, anchor_len=1000, reads_per_region=24, edge_overlaps=(300, 1000), n_decoys=24, seed=21)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="ont", anchor_len=1000)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "gpu"), seed=3, mixture="gpu", **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), seed=3, mixture="gpu",
                                 mixture_engine=ref_mixture_fit, **common)
    assert (tmp_path / "gpu.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_output.tsv").read_bytes()
    got = _tree(tmp_path / "gpu.details")
    assert got == _tree(tmp_path / "ref.details")
    assert sum(n.endswith(".summary.txt") for n in got) == 12 and any(n.endswith(".allele2.fastq") for n in got)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "sk3"), seed=3, **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "sk9"), seed=900, **common)
    n = 0
    for a, b, g in zip(*(_rows(tmp_path / f"{x}.NanoRepeat_output.tsv") for x in ("sk3", "sk9", "gpu"))):
        if (a[4], a[7]) == (b[4], b[7]):                          # two scikit-learn seeds agree on this region
            assert (g[4], g[7]) == (a[4], a[7]), a[:4]
            n += 1
    assert n >= 6


@pytest.mark.parametrize("remove_noisy_reads", [False, True])
def test_joint_command_gpu_engine_equals_restatement_and_default(capi, tmp_path, remove_noisy_reads):
    from nanorepeat_amd import pipeline
    from test_joint_round1 import _joint_files
    truth, rs1, rs2 = _joint_files(tmp_path, n=24)
    args = (str(tmp_path / "reads.fastq"), str(tmp_path / "ref.fa"), rs1, rs2)
    trees = {}
    for name, kw in (("gpu", dict(mixture="gpu")), ("ref", dict(mixture="gpu", mixture_engine=ref_mixture_fit)),
                     ("sk", {}), ("sk2", dict(seed=77))):
        (tmp_path / name).mkdir()
        kw = {"seed": 9, **kw}
        _, alleles = pipeline.quantify_joint(*args, str(tmp_path / name / "out"), remove_noisy_reads=remove_noisy_reads, **kw)
        trees[name] = (_tree(tmp_path / name), [(a.repeat1_median_size, a.repeat2_median_size, a.num_reads) for a in alleles])
    assert trees["gpu"][0] == trees["ref"][0]
    assert sorted(trees["gpu"][0]) == sorted(trees["sk"][0])
    if trees["sk"][1] == trees["sk2"][1]:
        assert trees["gpu"][1] == trees["sk"][1]
    assert len(trees["gpu"][1]) == 2
