"""Motif runs on the GPU: k_segment (nra_tract_segments) against the numpy restatement bit for bit -- edits, start phase,
start motif, every path byte and every motif byte -- over the corner cases of the contract, the template edges, seeded
sets in all three state classes, a 20 kb tract, forced small chunks and shuffled tracts; against nra_read_structure with
one motif and with a switch that never pays; and the FASTQ command end to end on the motif panel."""
import numpy as np
import pytest

from nanorepeat_amd import synth
import segment_ref as R
from segment_cases import rand_set, rand_tract, seeded_case, KINDS

pytestmark = pytest.mark.gpu


def _same(got, want):
    for k in ("edits", "start_phase", "start_motif", "path_off"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][:5])
    for k in ("path", "motif_of"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{len(bad)} {k} bytes differ, first at {bad[:5]}"


def _check(capi, sets, tracts, ts, W):
    got = capi.tract_segments(sets, tracts, ts, W)
    _same(got, R.ref_tract_segments(sets, tracts, ts, W))
    return got


def test_corner_cases(capi):
    rng = np.random.default_rng(1)
    two = ["ATTTT", "ATTTC"]
    # n = 0, 1 and n below every p; lowercase and other bytes; one tract
    _check(capi, [two], [""], [0], 3)
    _check(capi, [two], ["A"], [0], 3)
    _check(capi, [two, ["ACGTACGA", "CCGTTGCA"]], ["", "T", "ATT", "ATTC", "ACG", "GTTG"], [0, 0, 0, 0, 1, 1], 2)
    _check(capi, [two], ["atttt" * 5 + "ATTTC" * 8 + "atTTt" * 5, "ATTTTNNATTTC-ATTTCRATTTCATTTC", "NNNN", "nnnnnnn"],
           [0] * 4, 3)
    got = _check(capi, [two], ["ATTTT" * 5 + "ATTTC" * 8 + "ATTTT" * 5], [0], 3)
    assert got["edits"][0] == 6 and bytes(got["motif_of"]) == b"\0" * 25 + b"\1" * 40 + b"\0" * 25
    # 65 tracts: two waves; mixed sets and lengths inside one wave
    sets = [rand_set(rng, n_states=s) for s in (3, 8, 5, 7)]
    ts = rng.integers(0, 4, 65).astype(np.int32)
    tracts = [rand_tract(rng, sets[q], int(rng.integers(0, 200)), KINDS[i % len(KINDS)]) for i, q in enumerate(ts)]
    _check(capi, sets, tracts, ts, 3)
    # W = 1
    _check(capi, sets, tracts, ts, 1)


@pytest.mark.parametrize("S", (8, 9, 16, 17, 32))
def test_template_edges(capi, S):
    rng = np.random.default_rng(40 + S)
    sets = [rand_set(rng, n_states=S, n_motifs=m) for m in (1, 2, 3, min(8, S))]
    ts = np.arange(70, dtype=np.int32) % len(sets)
    tracts = [rand_tract(rng, sets[q], int(rng.integers(0, 300)), KINDS[i % len(KINDS)]) for i, q in enumerate(ts)]
    _check(capi, sets, tracts, ts, 3)


def test_eight_motifs_of_four_bases_and_shared_prefixes(capi):
    rng = np.random.default_rng(5)
    eight = []
    while len(eight) < 8:
        u = synth.rand_unit(rng, 4)
        if u not in eight:
            eight.append(u)
    prefixes = ["ACGTACGA", "ACGTACGT", "ACGTACG", "ACGTAC", "ACG"]            # the tie rules decide between them
    twins = ["CAGCAG", "CAG", "CAGCAGCAG", "AGC"]                                # the same sequence, four ways
    sets = [eight, prefixes, twins]
    ts = np.arange(90, dtype=np.int32) % 3
    tracts = [rand_tract(rng, sets[q], int(rng.integers(1, 250)), KINDS[i % len(KINDS)]) for i, q in enumerate(ts)]
    tracts[1] = "ACGTACG" * 12 + "ACGTACGT" * 9 + "ACG" * 11
    tracts[2] = "CAG" * 40
    for W in (1, 2, 5):
        _check(capi, sets, tracts, ts, W)


def test_one_motif_is_the_repeat_structure(capi):
    rng = np.random.default_rng(7)
    motifs = [synth.rand_unit(rng, p) if p > 1 else "ACGT"[p % 4] for p in range(1, 33)]
    rm = np.arange(96, dtype=np.int32) % 32
    tracts = [rand_tract(rng, [motifs[m]], int(rng.integers(0, 300)), KINDS[i % len(KINDS)]) for i, m in enumerate(rm)]
    st = capi.read_structure(motifs, tracts, rm)
    got = capi.tract_segments([[u] for u in motifs], tracts, rm, 3)
    for k in ("edits", "start_phase", "path", "path_off"):
        assert np.array_equal(got[k], st[k]), k
    assert not got["start_motif"].any() and not got["motif_of"].any()


def test_a_switch_that_never_pays(capi):
    """W = 1000 on tracts under 500 bases: no path can afford a switch (n <= 499 edits align anything), so the edits are
    the best of the set's motifs alone and every base of a tract has one motif index."""
    sets, tracts, ts = seeded_case(60, seed=11, max_len=499, n_sets=6)
    got = _check(capi, sets, tracts, ts, 1000)
    flat = [u for s in sets for u in s]
    first = np.cumsum([0] + [len(s) for s in sets])
    each = [capi.read_structure(flat, tracts, np.array([first[q] + k if k < len(sets[q]) else first[q] for q in ts], np.int32))
            ["edits"] for k in range(8)]
    best = np.array([min(each[k][i] for k in range(len(sets[ts[i]]))) for i in range(len(tracts))])
    assert np.array_equal(got["edits"], best)
    off = got["path_off"]
    assert all(len(set(got["motif_of"][off[i]:off[i + 1]].tolist())) <= 1 for i in range(len(tracts)))


@pytest.fixture(scope="module")
def seeded():
    """200 seeded tracts of 0..600 bases over random sets, a third in each state class, and their restatement."""
    parts = [seeded_case(67, seed=20 + S, max_len=600, n_states=S) for S in (6, 13, 29)]
    sets, tracts, ts = [], [], []
    for s, t, q in parts:
        ts += (q + len(sets)).tolist()
        sets += s
        tracts += t
    ts = np.array(ts, np.int32)
    assert {8, 16, 32} == {8 if sum(map(len, s)) <= 8 else 16 if sum(map(len, s)) <= 16 else 32 for s in sets}
    return sets, tracts, ts, R.ref_tract_segments(sets, tracts, ts, 3)


def test_seeded_tracts_in_all_state_classes(capi, seeded):
    sets, tracts, ts, want = seeded
    assert len(tracts) == 201
    got = capi.tract_segments(sets, tracts, ts, 3)
    _same(got, want)
    off = got["path_off"]
    assert sum(len(set(got["motif_of"][off[i]:off[i + 1]].tolist())) > 1 for i in range(len(tracts))) > 20


def test_forced_small_chunks_equal_one_chunk(capi, seeded, monkeypatch):
    sets, tracts, ts, want = seeded
    monkeypatch.setenv("NRA_TEST_SEG_PTR_BYTES", "4096")
    _same(capi.tract_segments(sets, tracts, ts, 3), want)


def test_chunks_of_single_waves_and_tracts_around_one_block(capi, monkeypatch):
    """130 tracts of 0, 1, 15, 16, 17 and 33 bases (both sides of the 16-byte block), 129 on a set of 6 states (two waves
    and one lane more: an empty tract that is the first lane of its wave) and one on a set of 20; in one chunk per state
    class and with every wave in a chunk of its own."""
    rng = np.random.default_rng(22)
    sets = [rand_set(rng, n_states=6, n_motifs=2), rand_set(rng, n_states=20, n_motifs=4)]
    lengths = [(0, 1, 15, 16, 17, 33)[i % 6] for i in range(129)] + [17]
    ts = np.array([0] * 129 + [1], np.int32)
    tracts = [rand_tract(rng, sets[q], n, "runs" if i % 2 else "random") for i, (n, q) in enumerate(zip(lengths, ts))]
    assert [len(t) for t in tracts] == lengths and min(lengths[:129]) == 0
    order = rng.permutation(130)
    tracts, ts = [tracts[i] for i in order], ts[order]
    want = R.ref_tract_segments(sets, tracts, ts, 3)
    monkeypatch.delenv("NRA_TEST_SEG_PTR_BYTES", raising=False)
    one = capi.tract_segments(sets, tracts, ts, 3)
    monkeypatch.setenv("NRA_TEST_SEG_PTR_BYTES", "1")
    many = capi.tract_segments(sets, tracts, ts, 3)
    _same(many, one)
    _same(one, want)


def test_shuffled_tracts_permute_the_outputs(capi, seeded):
    sets, tracts, ts, want = seeded
    perm = np.random.default_rng(3).permutation(len(tracts))
    got = capi.tract_segments(sets, [tracts[i] for i in perm], ts[perm], 3)
    off, woff = got["path_off"], want["path_off"]
    for k, i in enumerate(perm):
        for f in ("edits", "start_phase", "start_motif"):
            assert got[f][k] == want[f][i], (f, k)
        for f in ("path", "motif_of"):
            assert np.array_equal(got[f][off[k]:off[k + 1]], want[f][woff[i]:woff[i + 1]]), (f, k)


def test_one_20kb_tract(capi):
    rng = np.random.default_rng(9)
    sets = [["ATTTT", "ATTTC"], ["AAAAG", "AAGGG", "AAAGG", "ACGTACGTTT"]]
    long = synth.apply_errors(rng, "ATTTT" * 1800 + "ATTTC" * 1200 + "ATTTT" * 1000, "ont")[:20000]
    short = rand_tract(rng, sets[1], 300)
    got = _check(capi, sets, [long, short], [0, 1], 3)
    assert set(got["motif_of"][:len(long)].tolist()) == {0, 1}
    with pytest.raises(capi.NraError) as e:
        capi.tract_segments([["CAG"]], ["CAG" * 66667], [0], 3)
    assert e.value.code == capi.E_RANGE


def test_fastq_command_on_the_motif_panel(capi, tmp_path):
    """The device's files equal the files written with the restatement as engine; the DAB1-like allele comes back as
    ATTTT, ATTTC, ATTTT with its ATTTC units within the tolerance of DESIGN.md section 20.3 (the largest error of a read
    in the restatement's hifi table, 2.0 units, plus 1 unit for the consensus's one-base lean: 3.0); the TATTG control
    and the (ATTTT)15 allele show a single run."""
    from nanorepeat_amd import pipeline, segments
    from test_screen_cpu import _tree
    p = synth.motif_panel()
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=1000, seed=3)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), motif_runs=True, **common)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "ref"), motif_runs=True,
                                 segment_engine=R.ref_tract_segments, **common)
    on, off, want = (_tree(tmp_path / f"{n}.details") for n in ("on", "off", "ref"))
    assert on == want and sum(k.endswith(".read_runs.tsv") for k in on) == 4
    assert {k: v for k, v in on.items() if not k.endswith(".read_runs.tsv")} == off
    assert (tmp_path / "on.NanoRepeat_runs.tsv").read_bytes() == (tmp_path / "ref.NanoRepeat_runs.tsv").read_bytes()
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    assert sorted(q.name for q in tmp_path.glob("on.*")) == ["on.NanoRepeat_output.tsv", "on.NanoRepeat_runs.tsv",
                                                             "on.details"]
    dab, control = regions[2], regions[3]
    assert dab.motif_set[:2] == ["ATTTT", "ATTTC"]
    (_, short), (_, long) = dab.allele_runs
    assert [dab.motif_set[r.motif] for r in long.runs] == ["ATTTT", "ATTTC", "ATTTT"]
    assert len(short.runs) == 1 and dab.motif_set[short.runs[0].motif] == "ATTTT"
    units = segments.allele_units(dab)
    attc = units[1][2][1]
    print("ATTTC median units", attc, "consensus", segments.runs_text(long.runs, dab.motif_set))
    assert abs(attc - 40) <= 3.0 and abs(long.runs[1].consumed / 5 - 40) <= 3.0
    assert all(len(tr.runs) == 1 for _, tr in control.allele_runs)
