"""Repeat structure on the GPU: k_structure (nra_read_structure) against the numpy restatement bit for bit -- edits,
start phase and every path byte -- over motif lengths 1..64, tract kinds and lengths up to 200 kb, forced small
chunks, a config-4-scale call, and the FASTQ command end to end on a panel with planted interruptions."""

import numpy as np
import pytest

from nanorepeat_amd import synth
from structure_ref import ref_read_structure

pytestmark = pytest.mark.gpu

P_LIST = (1, 2, 3, 5, 6, 7, 12, 16, 17, 31, 32, 33, 64)


def _motif(rng, p):
    return synth.rand_unit(rng, p) if p > 1 else "ACGT"[int(rng.integers(0, 4))]


def _tract(rng, u, kind, n_units):
    p = len(u)
    phase = int(rng.integers(0, p))
    pure = (u * (n_units + 2))[phase:phase + n_units * p + int(rng.integers(0, p))]
    if kind == "pure":
        return pure
    if kind == "interrupted":
        s = pure
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + synth.rand_seq(rng, int(rng.integers(1, p + 3))) + s[at:]
        return s
    if kind in ("ont", "hifi"):
        return synth.apply_errors(rng, pure, kind)
    if kind == "random":
        return synth.rand_seq(rng, len(pure))
    if kind == "n":
        s = list(synth.apply_errors(rng, pure, "ont"))
        for _ in range(max(1, len(s) // 50)):
            if s:
                s[int(rng.integers(0, len(s)))] = "NRY-"[int(rng.integers(0, 4))]
        return "".join(s)
    if kind == "lower":
        s = synth.apply_errors(rng, pure, "hifi")
        return s.lower() if rng.random() < 0.5 else s[:len(s) // 2].lower() + s[len(s) // 2:]
    raise ValueError(kind)


KINDS = ("pure", "interrupted", "ont", "hifi", "random", "n", "lower")


def _case(seed, p_list, n_per_p, long_every=0):
    rng = np.random.default_rng(seed)
    motifs, tracts, rm = [], [], []
    for p in p_list:
        for _ in range(2):                                   # two motifs of each length in the call
            motifs.append(_motif(rng, p))
        for i in range(n_per_p):
            m = len(motifs) - 1 - (i % 2)
            u = motifs[m]
            kind = KINDS[i % len(KINDS)]
            if i % 17 == 0:
                n_units = 0
            elif long_every and i % long_every == long_every - 1:
                n_units = int(rng.integers(2000, 20001)) // p
            else:
                n_units = int(rng.integers(1, max(2, 600 // p)))
            t = _tract(rng, u, kind, n_units)
            if i % 23 == 5:
                t = t[:int(rng.integers(0, 3))]              # 0..2 bases
            tracts.append(t)
            rm.append(m)
    order = rng.permutation(len(tracts))
    return motifs, [tracts[i] for i in order], np.array(rm, np.int32)[order]


def _same(got, want):
    assert np.array_equal(got["edits"], want["edits"])
    assert np.array_equal(got["start_phase"], want["start_phase"])
    assert np.array_equal(got["path_off"], want["path_off"])
    bad = np.nonzero(got["path"] != want["path"])[0]
    assert len(bad) == 0, f"{len(bad)} path bytes differ, first at {bad[:5]}"


@pytest.mark.parametrize("p", P_LIST)
def test_kernel_equals_restatement_per_motif_length(capi, p):
    motifs, tracts, rm = _case(100 + p, (p,), 157, long_every=60)
    assert len(tracts) % 64 != 0
    _same(capi.read_structure(motifs, tracts, rm), ref_read_structure(motifs, tracts, rm))


def test_many_motifs_in_one_call(capi):
    motifs, tracts, rm = _case(7, P_LIST, 45)
    got = capi.read_structure(motifs, tracts, rm)
    _same(got, ref_read_structure(motifs, tracts, rm))
    assert (got["edits"] > 0).any() and (got["edits"] == 0).any()


def test_one_200kb_tract(capi):
    rng = np.random.default_rng(3)
    for p, kind in ((5, "ont"), (33, "interrupted")):
        u = _motif(rng, p)
        t = _tract(rng, u, kind, 200000 // p)[:200000]
        short = _tract(rng, u, "hifi", 40)
        got = capi.read_structure([u], [t, short], [0, 0])
        _same(got, ref_read_structure([u], [t, short], [0, 0]))
    with pytest.raises(capi.NraError) as e:
        capi.read_structure(["CAG"], ["CAG" * 66667 + "CA"], [0])
    assert e.value.code == capi.E_RANGE


def test_forced_small_chunks_equal_one_chunk(capi, monkeypatch):
    motifs, tracts, rm = _case(11, (3, 6, 16, 64), 200, long_every=150)
    monkeypatch.delenv("NRA_TEST_STRUCT_PTR_BYTES", raising=False)
    one = capi.read_structure(motifs, tracts, rm)
    monkeypatch.setenv("NRA_TEST_STRUCT_PTR_BYTES", "4096")
    many = capi.read_structure(motifs, tracts, rm)
    _same(many, one)
    _same(one, ref_read_structure(motifs, tracts, rm))


def test_chunks_of_single_waves_and_tracts_around_one_block(capi, monkeypatch):
    """130 tracts of 0, 1, 15, 16, 17 and 33 bases (both sides of the 16-byte block), 129 of capacity 3 (two waves and
    one lane more: an empty tract that is the first lane of its wave) and one of capacity 64; in one chunk per capacity
    and with every wave in a chunk of its own."""
    rng = np.random.default_rng(21)
    motifs = ["CAG", _motif(rng, 40)]
    lengths = [(0, 1, 15, 16, 17, 33)[i % 6] for i in range(129)] + [17]
    rm = np.array([0] * 129 + [1], np.int32)
    tracts = [(motifs[m] * 12)[i % 3:][:n] if i % 2 else synth.rand_seq(rng, n) for i, (n, m) in enumerate(zip(lengths, rm))]
    assert [len(t) for t in tracts] == lengths and min(lengths[:129]) == 0
    order = rng.permutation(130)
    tracts, rm = [tracts[i] for i in order], rm[order]
    want = ref_read_structure(motifs, tracts, rm)
    monkeypatch.delenv("NRA_TEST_STRUCT_PTR_BYTES", raising=False)
    one = capi.read_structure(motifs, tracts, rm)
    monkeypatch.setenv("NRA_TEST_STRUCT_PTR_BYTES", "1")
    many = capi.read_structure(motifs, tracts, rm)
    _same(many, one)
    _same(one, want)


def test_config4_scale_call_matches_on_a_sample(capi):
    d = synth.config4(1000, 1000)
    motifs = [u for _, u, _ in d["regions"]]
    tracts = [s[100:max(100, len(s) - 100)] for s in d["reads"]]
    got = capi.read_structure(motifs, tracts, d["read_region"])
    rng = np.random.default_rng(9)
    rr = d["read_region"]
    sample = np.sort(np.concatenate([rng.choice(np.nonzero(rr == g)[0], 3, replace=False) for g in range(len(motifs))]))
    want = ref_read_structure(motifs, [tracts[i] for i in sample], rr[sample])
    off = got["path_off"]
    sub = dict(edits=got["edits"][sample], start_phase=got["start_phase"][sample],
               path=np.concatenate([got["path"][off[i]:off[i + 1]] for i in sample]), path_off=want["path_off"])
    _same(sub, want)


def test_fastq_command_recovers_planted_interruptions(capi, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    p = synth.structure_panel(model="hifi", seed=5)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), read_structure=True, **common)
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".read_structure.tsv")} == off
    assert sum(k.endswith(".read_structure.tsv") for k in on) == 3
    rows = [l.split("\t") for l in (tmp_path / "on.NanoRepeat_structure.tsv").read_text().split("\n")[1:] if l]
    assert len(rows) == 3
    from nanorepeat_amd import structure
    for g, (row, region) in enumerate(zip(rows, regions)):
        alleles = structure.allele_structures(region)
        assert int(row[4]) == len(alleles) == 2, row
        # alleles come in phasing order (ascending size), like the planted ones
        for (label, n, purity, pure, longest, recurrent), planted in zip(alleles, p["planted"][g]):
            assert n >= 6
            # every planted interruption is recurrent at its slot (an error that many reads share by chance, such as a
            # lost base somewhere in the tract, may be recurrent too: the key is the bases and their rank in the read)
            got = [(b, round(k)) for b, k in recurrent]
            assert all(x in got for x in planted), (g, label, recurrent)
            assert purity > 0.95
