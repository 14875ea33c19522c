"""nra_align_paths on the device: the trace fill in chained row blocks against the oracle's traceback, bit for bit
(DESIGN.md section 21), and the round-3 alignment file end to end."""
import numpy as np
import pytest

from nanorepeat_amd import synth
from paths_cases import paths_panel, paf_rows, spans_fit_cigar

pytestmark = pytest.mark.gpu

KEYS = ("score", "tstart", "tend", "qstart", "qend")
OVERRIDES = ({}, {"min_dp_score": 0})


def _against_oracle(capi, oracle, seqs, pq, pt, over, call=None):
    g = (call or capi.align_paths)(seqs, pq, pt, sc=capi.default_scoring(**over))
    lo = max(1, over.get("min_dp_score", 80))
    n_records = 0
    for i, (a, b) in enumerate(zip(pq, pt)):
        o = oracle.align_cigar(seqs[a], seqs[b], sc=oracle.default_scoring(**over)) if seqs[a] and seqs[b] else dict(score=0)
        if o["score"] < lo:
            assert g["score"][i] == -1 and g["cigar"][i] == "", (i, len(seqs[a]), len(seqs[b]))
            continue
        n_records += 1
        got = (int(g["score"][i]), g["cigar"][i], *[int(g[k][i]) for k in KEYS[1:]])
        want = (o["score"], o["cigar"], o["tstart"], o["tend"], o["qstart"], o["qend"])
        assert got == want, (i, len(seqs[a]), len(seqs[b]), got[0], want[0], got[2:], want[2:])
    return g, n_records


def _seam_pairs():
    rng = np.random.default_rng(41)
    seqs, pq, pt = [], [], []

    def pair(q, t):
        seqs.extend([q, t]); pq.append(len(seqs) - 2); pt.append(len(seqs) - 1)

    for ql in (63, 64, 65, 128, 129, 191, 300):
        for tl in (1, 50, 400):
            q = synth.rand_seq(rng, ql)
            for model in ("ont", "hifi"):                          # related: the query's errors inside random flanks
                e = synth.apply_errors(rng, q, model)
                lead = int(rng.integers(0, max(1, tl - len(e)))) if tl > len(e) else 0
                pair(q, (synth.rand_seq(rng, lead) + e + synth.rand_seq(rng, tl))[:tl] if tl > 1 else q[ql // 2])
            pair(q, synth.rand_seq(rng, tl))                       # random
    t = synth.rand_seq(rng, 260)                                   # N runs across the seams at rows 64 and 128
    q = list(synth.apply_errors(rng, t[20:240], "hifi"))
    q[61:67] = "NNNNNN"; q[127:130] = "NNN"
    pair("".join(q), t)
    t = synth.rand_seq(rng, 200)                                   # a gap that opens in one block and extends through the next
    pair(t[:60] + synth.rand_seq(rng, 70) + t[60:], t)
    seqs.extend(["", synth.rand_seq(rng, 50)])                     # an empty sequence on either side
    pq.extend([len(seqs) - 2, len(seqs) - 1, len(seqs) - 2]); pt.extend([len(seqs) - 1, len(seqs) - 2, len(seqs) - 2])
    return seqs, pq, pt


@pytest.mark.parametrize("over", OVERRIDES, ids=("default", "min0"))
def test_block_seams_at_tiny_shapes(capi, oracle, monkeypatch, over):
    monkeypatch.setenv("NRA_TEST_TRACE_BLOCK_ROWS", "64")
    seqs, pq, pt = _seam_pairs()
    g, n = _against_oracle(capi, oracle, seqs, pq, pt, over)
    assert n >= (20 if not over else 40)
    ins = [i for i in range(len(pq)) if len(seqs[pq[i]]) == 270 and len(seqs[pt[i]]) == 200]
    assert len(ins) == 1 and "70I" in g["cigar"][ins[0]] and g["qstart"][ins[0]] < 60     # rows 60..129: two seams


def test_block_seams_in_64_bit_cells(capi, oracle, monkeypatch):
    """match 64: a 600-base pair scores beyond what an int32 cell holds above its 16-bit origin column."""
    monkeypatch.setenv("NRA_TEST_TRACE_BLOCK_ROWS", "128")
    rng = np.random.default_rng(43)
    t = synth.rand_seq(rng, 700)
    seqs = [synth.apply_errors(rng, t[40:650], "hifi"), t, synth.apply_errors(rng, t[300:500], "ont"),
            t[:100] + synth.rand_seq(rng, 150) + t[100:]]
    over = {"match": 64, "min_dp_score": 0}
    g, n = _against_oracle(capi, oracle, seqs, [0, 2, 3], [1, 1, 1], over)
    assert n == 3 and g["score"][0] > 32767


@pytest.fixture(scope="module")
def long_pairs():
    rng = np.random.default_rng(45)
    seqs, pq, pt = [], [], []
    for ql, tl in ((3072, 300), (3073, 450), (6144, 700), (6145, 520)):
        q = synth.rand_seq(rng, ql)
        mid = ql // 2
        seqs += [q, synth.apply_errors(rng, q[mid - tl // 2:mid + tl // 2], "ont")]
        pq.append(len(seqs) - 2); pt.append(len(seqs) - 1)
    t = synth.rand_seq(rng, 3600)
    seqs += [(synth.apply_errors(rng, t[30:3560], "hifi") + synth.rand_seq(rng, 100))[:3500], t]
    pq.append(len(seqs) - 2); pt.append(len(seqs) - 1)
    assert len(seqs[-2]) == 3500
    return seqs, pq, pt


def test_real_block_height(capi, oracle, long_pairs):
    seqs, pq, pt = long_pairs
    g, n = _against_oracle(capi, oracle, seqs, pq, pt, {})
    assert n == len(pq)
    assert g["qend"][2] > 1536 * 2 and g["qend"][4] > 3072            # best cells beyond the first blocks


def test_3073_bases_need_the_new_call(capi, oracle, long_pairs):
    seqs, pq, pt = long_pairs
    assert len(seqs[pq[1]]) == 3073
    with pytest.raises(capi.NraError) as e:
        capi.align_pairs_cigar(seqs, pq[1:2], pt[1:2])
    assert e.value.code == capi.E_RANGE
    _, n = _against_oracle(capi, oracle, seqs, pq[1:2], pt[1:2], {})
    assert n == 1
    assert capi.align_pairs_cigar(seqs, pq[:1], pt[:1])["cigar"][0] == capi.align_paths(seqs, pq[:1], pt[:1])["cigar"][0]


def test_equal_on_short_queries(capi):
    """The pairs of test_paf_cigar.test_cigar_emission_matches_oracle_traceback."""
    rng = np.random.default_rng(21)
    seqs, pq, pt = [], [], []
    for i in range(14):
        L, R = synth.rand_seq(rng, int(rng.integers(30, 300))), synth.rand_seq(rng, int(rng.integers(30, 300)))
        u = ["TATTG", "CAG", "AT", "GGCCCC"][i % 4]; k = int(rng.integers(0, 40))
        t = L + u * k + R
        q = synth.apply_errors(rng, L[-60:] + u * int(rng.integers(0, 40)) + R[:60], "ont" if i % 2 else "hifi")
        if i == 5:
            q = q[:30] + "NNN" + q[33:]
        seqs += [q, t]; pq.append(2 * i); pt.append(2 * i + 1)
    seqs += ["", synth.rand_seq(rng, 50)]
    pq += [28, 29, 0]; pt += [1, 3, 29]
    for over in OVERRIDES:
        a = capi.align_pairs_cigar(seqs, pq, pt, sc=capi.default_scoring(**over))
        for call in (capi.align_paths, capi.align_paths_chunked):
            b = call(seqs, pq, pt, sc=capi.default_scoring(**over))
            assert a["cigar"] == b["cigar"] and any(a["cigar"])
            for k in KEYS:
                assert np.array_equal(a[k], b[k]), k


def test_range_checks(capi):
    """Checked on the host: nothing is launched."""
    for q, t in ((200001, 10), (10, 65001), (200000, 65000)):
        with pytest.raises(capi.NraError) as e:
            capi.align_paths(["A" * q, "C" * t], [0], [1])
        assert e.value.code == capi.E_RANGE, (q, t)


def test_fastq_command_writes_the_round3_alignments(capi, oracle, tmp_path):
    from nanorepeat_amd import pipeline
    from test_screen_cpu import _tree
    p = paths_panel(long_units=1100)
    ref, bed, reads = synth.write_panel(p, str(tmp_path))
    common = dict(data_type="hifi", anchor_len=500, seed=3)
    pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "off"), **common)
    regions = pipeline.quantify_from_reads(reads, ref, bed, str(tmp_path / "on"), read_alignments=True, **common)
    on, off = _tree(tmp_path / "on.details"), _tree(tmp_path / "off.details")
    assert {k: v for k, v in on.items() if not k.endswith(".round3.paf")} == off
    assert sum(k.endswith(".round3.paf") for k in on) == 3
    assert (tmp_path / "on.NanoRepeat_output.tsv").read_bytes() == (tmp_path / "off.NanoRepeat_output.tsv").read_bytes()
    n_long = 0
    for region in regions:
        rows = paf_rows(f"{region.out_prefix}.round3.paf")
        ok = [n for n, r in region.read_dict.items() if r.round3_status == capi.READ_OK]
        assert sorted(p_.qname for p_, _ in rows) == sorted(ok) and len(ok) >= 5
        for row, rs in rows:
            read = region.read_dict[row.qname]
            core = region.read_core_seq_dict[row.qname].strip()
            k = int(row.tname.rsplit("|k=", 1)[1])
            assert row.tname == f"{region.to_unique_id()}|k={k}" and rs == f"{read.round3_repeat_size:.1f}"
            assert row.align_score == read.round3_best_score and row.strand == "+" and spans_fit_cigar(row)
            template = region.left_anchor_seq + region.repeat_unit_seq * k + region.right_anchor_seq
            assert (row.qlen, row.tlen) == (len(core), len(template))
            o = oracle.align_cigar(core, template)
            assert (row.cigar, row.tstart, row.tend, row.qstart, row.qend) == \
                   (o["cigar"], o["tstart"], o["tend"], o["qstart"], o["qend"])
            n_long += len(core) > 3072
    assert n_long >= 2
