"""Tandem periods on the GPU: k_tract_periods (nra_tract_periods) against the numpy restatement bit for bit -- at the
edges of the kernel's 32-base words, for every max_period class, with bytes other than ACGT, lower case, 200 kb tracts,
many short tracts in one call against each alone and permuted, forced small chunks -- and the FASTQ command end to end
on synth.period_panel."""
import numpy as np
import pytest

from nanorepeat_amd import periods, synth
import period_cases as cases
from period_ref import ref_tract_periods

pytestmark = pytest.mark.gpu


def _same(got, want):
    for k in ("match", "valid"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.int32, k
        bad = np.nonzero((got[k] != want[k]).any(axis=1))[0]
        assert len(bad) == 0, f"{k}: {len(bad)} tracts differ, first {bad[:5]}"


def test_word_edges_non_acgt_and_lower_case_every_max_period(capi):
    tracts = cases.edge_tracts() + cases.p_and_p_plus_one() + cases.non_acgt_tracts() + cases.lower_case_tracts()
    want = ref_tract_periods(tracts, 64)
    for max_period in cases.MAX_PERIODS:
        got = capi.tract_periods(tracts, max_period)
        _same(got, {k: v[:, :max_period] for k, v in want.items()})
    got = capi.tract_periods(cases.p_and_p_plus_one())
    assert got["valid"][:, 0].tolist() == [0, 1, 1, 63, 64, 64] and got["match"][:3, 0].tolist() == [0, 1, 0]
    assert got["valid"][:, 63].tolist() == [0, 0, 0, 0, 1, 1] and got["match"][:, 63].tolist() == [0, 0, 0, 0, 1, 0]


def test_200kb_homopolymer_and_64mer(capi):
    tracts = cases.long_tracts()
    got = capi.tract_periods(tracts)
    _same(got, ref_tract_periods(tracts))
    lags = np.arange(1, 65)
    assert (got["match"][0] == 200000 - lags).all() and (got["valid"][0] == 200000 - lags).all()
    assert got["match"][1, 63] == 200000 - 64 and periods.call_period(got["match"][1], got["valid"][1])[0] == 64
    with pytest.raises(capi.NraError) as e:
        capi.tract_periods(["CAG", "A" * 200001])
    assert e.value.code == capi.E_RANGE


def test_a_tract_does_not_depend_on_the_others_or_their_order(capi):
    tracts = cases.short_mixed()
    want = ref_tract_periods(tracts)
    one = capi.tract_periods(tracts)
    _same(one, want)
    for t, s in enumerate(tracts):
        alone = capi.tract_periods([s])
        assert (alone["match"][0] == want["match"][t]).all() and (alone["valid"][0] == want["valid"][t]).all(), t
    perm = np.random.default_rng(5).permutation(len(tracts))
    shuffled = capi.tract_periods([tracts[i] for i in perm])
    _same(shuffled, {k: v[perm] for k, v in want.items()})
    assert capi.tract_periods([])["match"].shape == (0, 64)


def _chunks(capfd):
    """The tract counts of the chunks the library traced on stderr since the last call (NRA_DEBUG)."""
    return [int(l.split()[3]) for l in capfd.readouterr().err.split("\n") if l.startswith("nra_tract_periods: chunk of")]


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch, capfd):
    """A tract costs its 16-byte-rounded codes and 512 bytes of results of a chunk's budget."""
    tracts = cases.short_mixed(seed=36) + cases.edge_tracts(seed=37)
    monkeypatch.setenv("NRA_DEBUG", "1")                           # the call traces its chunks on stderr
    monkeypatch.delenv("NRA_TEST_PERIOD_CHUNK_BYTES", raising=False)
    capfd.readouterr()
    one = capi.tract_periods(tracts)
    assert _chunks(capfd) == [len(tracts)]
    monkeypatch.setenv("NRA_TEST_PERIOD_CHUNK_BYTES", "4096")      # read at every call
    many = capi.tract_periods(tracts)
    counts = _chunks(capfd)
    cost = sum((len(t) + 15) // 16 * 16 + 512 for t in tracts)
    assert sum(counts) == len(tracts) and cost // 4096 <= len(counts) <= len(tracts) and max(counts) <= 8
    assert any(c % 4 for c in counts[:-1])                         # chunks that end inside a workgroup's four tracts
    _same(many, one)
    _same(one, ref_tract_periods(tracts))
    monkeypatch.setenv("NRA_TEST_PERIOD_CHUNK_BYTES", "1")         # a tract beyond the budget goes alone
    alone = capi.tract_periods(tracts[:60])
    assert _chunks(capfd) == [1] * 60
    _same(alone, {k: v[:60] for k, v in one.items()})


def test_fastq_command_finds_planted_periods(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_periods_cpu import check_panel
    from test_screen_cpu import _tree
    p = synth.period_panel(model="hifi", seed=5)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3, no_check_repeat_motif_in_ref=True)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), discover_periods=True, **common)
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_periods.tsv")} == off
    assert sum(k.endswith(".read_periods.tsv") for k in on) == 7
    assert not (tmp_path / "off.NanoRepeat_periods.tsv").exists()
    check_panel(p, regions, (tmp_path / "on.NanoRepeat_periods.tsv").read_text())
