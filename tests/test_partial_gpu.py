"""One-anchor reads on the GPU: k_extend (nra_extend_tracts) against the numpy restatement bit for bit -- score, end,
end phase and motif bases -- over motif lengths 1..64, tract kinds and lengths up to 200 kb, several score triples, a
config-4-scale call, the argument errors, and the BAM command end to end on the panel with an allele no read spans."""
import ctypes as C
import sys

import numpy as np
import pytest

from nanorepeat_amd import synth
from extend_ref import ref_extend_tracts
from test_structure_gpu import P_LIST, _motif, _tract, _case

pytestmark = pytest.mark.gpu

SCORES = ((2, 4, 6), (1, 0, 1), (3, 2, 127), (127, 127, 5), (5, 0, 3))       # among them b = 0 and g = 127


def _same(got, want):
    for k in ("score", "end", "end_phase", "motif_bases"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert got[k].dtype == np.int32 and len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[:5]}"


def _with_tails(seed, tracts):
    """Every third tract runs into sequence that is not repeat."""
    rng = np.random.default_rng(seed)
    return [t + synth.rand_seq(rng, int(rng.integers(0, 200))) if i % 3 == 0 else t for i, t in enumerate(tracts)]


@pytest.mark.parametrize("p", P_LIST)
def test_kernel_equals_restatement_per_motif_length(capi, p):
    motifs, tracts, rm = _case(100 + p, (p,), 157, long_every=60)
    tracts = _with_tails(p, tracts)
    assert len(tracts) % 64 != 0
    sc = SCORES[p % len(SCORES)]
    for a, b, g in {(2, 4, 6), sc}:
        _same(capi.extend_tracts(motifs, tracts, rm, match=a, mismatch=b, gap=g),
              ref_extend_tracts(motifs, tracts, rm, match=a, mismatch=b, gap=g))


@pytest.mark.parametrize("scores", SCORES)
def test_many_motifs_in_one_call(capi, scores):
    motifs, tracts, rm = _case(7, P_LIST, 45)
    tracts = _with_tails(8, tracts)
    a, b, g = scores
    got = capi.extend_tracts(motifs, tracts, rm, match=a, mismatch=b, gap=g)
    _same(got, ref_extend_tracts(motifs, tracts, rm, match=a, mismatch=b, gap=g))
    assert (got["score"] > 0).any() and (got["score"] == 0).any()
    assert (got["end"][got["score"] == 0] == 0).all() and (got["motif_bases"][got["score"] == 0] == 0).all()


def test_pure_prefixes_show_every_base(capi):
    motifs = ["CAG", "TATTG", "A", "GGCCCC", synth.rand_unit(np.random.default_rng(1), 33)]
    tracts, rm, want = [], [], []
    for m, u in enumerate(motifs):
        p = len(u)
        for phase in range(p):
            for L in (p, 4 * p + 2, 997):
                tracts.append((u * (L // p + 3))[phase:phase + L])
                rm.append(m)
                want.append((2 * L, L, (phase + L) % p, L))
    got = capi.extend_tracts(motifs, tracts, rm)
    assert [tuple(int(got[k][i]) for k in ("score", "end", "end_phase", "motif_bases")) for i in range(len(tracts))] == want


def test_200kb_tracts(capi):
    rng = np.random.default_rng(3)
    for p, kind, scores in ((5, "ont", (2, 4, 6)), (33, "interrupted", (3, 0, 127))):
        u = _motif(rng, p)
        t = _tract(rng, u, kind, 200000 // p)[:200000]
        short = _tract(rng, u, "hifi", 40)
        a, b, g = scores
        got = capi.extend_tracts([u], [t, short], [0, 0], match=a, mismatch=b, gap=g)
        _same(got, ref_extend_tracts([u], [t, short], [0, 0], match=a, mismatch=b, gap=g))
        assert got["end"][0] > 150000
    # the largest values the contract allows stay inside int32: 200 000 matches of 127
    got = capi.extend_tracts(["A"], ["A" * 200000], [0], match=127, mismatch=127, gap=127)
    assert (int(got["score"][0]), int(got["end"][0]), int(got["motif_bases"][0])) == (127 * 200000, 200000, 200000)


def test_config4_scale_call_matches_on_a_sample(capi):
    d = synth.config4(1000, 1000)
    motifs = [u for _, u, _ in d["regions"]]
    tracts = [s[100:] for s in d["reads"]]                   # what follows the left anchor: the tract, then the flank
    rr = d["read_region"]
    got = capi.extend_tracts(motifs, tracts, rr)
    rng = np.random.default_rng(9)
    sample = np.sort(np.concatenate([rng.choice(np.nonzero(rr == g)[0], 3, replace=False) for g in range(len(motifs))]))
    want = ref_extend_tracts(motifs, [tracts[i] for i in sample], rr[sample])
    _same({k: v[sample] for k, v in got.items()}, want)
    # the units shown follow the planted allele (errors and the flank's first bases move it by a few)
    units = got["motif_bases"] // np.array([len(motifs[g]) for g in rr])
    assert np.mean(np.abs(units - d["k_true"]) <= 3) > 0.95


def test_argument_errors_come_before_the_device(capi):
    lib = capi.load()
    for motif, code in (("", -1), ("A" * 65, -3), ("CAN", -1), ("cag", -1)):
        with pytest.raises(capi.NraError) as e:
            capi.extend_tracts([motif], ["CAGCAG"], [0], device=99)
        assert e.value.code == code, motif
    for kw in (dict(match=0), dict(match=128), dict(mismatch=-1), dict(mismatch=128), dict(gap=0), dict(gap=128)):
        with pytest.raises(capi.NraError) as e:
            capi.extend_tracts(["CAG"], ["CAGCAG"], [0], device=99, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(capi.NraError) as e:
        capi.extend_tracts(["CAG"], ["CAG"], [1], device=99)
    assert e.value.code == -1
    with pytest.raises(capi.NraError) as e:
        capi.extend_tracts(["CAG"], ["CAG" * 66667], [0], device=99)
    assert e.value.code == capi.E_RANGE
    data, off = capi.pack_reads(["CAG"])
    none4 = (None,) * 4
    assert lib.nra_extend_tracts(0, 0, data, capi._ptr(off, C.c_int64), 0, None, None, None, 2, 4, 6, *none4) == -1
    assert lib.nra_extend_tracts(0, 1, data, None, 0, None, None, None, 2, 4, 6, *none4) == -1
    with pytest.raises(capi.NraError) as e:                  # good arguments: the device index is looked at last
        capi.extend_tracts(["CAG"], ["CAGCAG"], [0], device=99)
    assert e.value.code == -1 and "device index" in str(e.value)
    out = capi.extend_tracts(["CAG"], [], [])
    assert all(len(v) == 0 for v in out.values())
    out = capi.extend_tracts(["CAG", "A" * 64], ["CAGCAG", ""], [0, 1], mismatch=0, gap=127)
    assert [int(out[k][0]) for k in ("score", "end", "end_phase", "motif_bases")] == [12, 6, 0, 6]
    assert [int(out[k][1]) for k in ("score", "end", "end_phase", "motif_bases")] == [0, 0, 0, 0]


def test_bam_command_on_the_gpu_equals_the_cpu_path(capi, oracle, tmp_path, monkeypatch, capsys):
    from test_partial_cpu import run_panel, check_panel_outputs
    monkeypatch.setitem(sys.modules, "pysam", None)
    (tmp_path / "gpu").mkdir()
    (tmp_path / "cpu").mkdir()
    regions, tree, summary, planted, err = run_panel(tmp_path / "gpu", capsys)
    check_panel_outputs(regions, tree, summary, planted, err)
    _, cpu_tree, cpu_summary, _, _ = run_panel(tmp_path / "cpu", capsys, aligner=oracle.align_pairs,
                                               scorer=oracle.round3_1d, extension_engine=ref_extend_tracts)
    assert tree == cpu_tree and summary == cpu_summary
    for name in ("on.NanoRepeat_output.tsv", "on.NanoRepeat_partial.tsv"):
        assert (tmp_path / "gpu" / name).read_bytes() == (tmp_path / "cpu" / name).read_bytes()
