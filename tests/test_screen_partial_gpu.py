"""The motif screen on the MI355X: nra_screen_set_motifs / nra_screen_reads_partial against the numpy restatement of
their contract (tests/screen_partial_ref.py) -- everything is integers, so the device equals it exactly -- and the
FASTQ command with partial_reads / in_repeat_reads end to end."""
import ctypes as C

import numpy as np
import pytest

import screen_partial_cases as cases
from screen_partial_ref import RefScreenPartial, class_windows, classes_of

pytestmark = pytest.mark.gpu

KEYS = ("read", "region", "hits_left", "hits_right", "motif_windows", "kind")


def _ref(case):
    ref = RefScreenPartial(case["anchors"], k=case["k"], max_occ=case["max_occ"], motifs=case["motifs"])
    return ref.screen_reads_partial(case["reads"], case["min_hits"], case["pct"])


def _gpu(case):
    from nanorepeat_amd.screen import Screen
    with Screen(case["anchors"], k=case["k"], max_occ=case["max_occ"], motifs=case["motifs"]) as scr:
        return scr.screen_reads_partial(case["reads"], case["min_hits"], case["pct"]), scr.stats()


def _same(got, want, keys=KEYS):
    for key in keys:
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("k", [11, 15])
def test_kernel_edges(capi, k):
    case = cases.edge_case(k)
    assert 35 <= len(case["reads"]) <= 50
    got, st = _gpu(case)
    want = _ref(case)
    _same(got, want)
    assert st["n_classes"] == len(classes_of(case["motifs"])[1]) == 7
    assert (got["kind"] == 3).sum() >= 20 and (got["kind"] == 1).sum() >= 1


def test_tiles(capi):
    case = cases.tile_case()
    got, _ = _gpu(case)
    _same(got, _ref(case))
    # the long read: its class windows are the sum over its tiles' own windows
    long_read, k = case["reads"][2], case["k"]
    members = classes_of(case["motifs"])[1]
    n_win = len(long_read) - k + 1
    assert n_win > 4 * cases.TILE
    pieces = [long_read[w:w + cases.TILE + k - 1] for w in range(0, n_win, cases.TILE)]
    by_tile = class_windows(pieces, k, members).sum(0)
    assert (by_tile == class_windows([long_read], k, members)[0]).all() and by_tile.min() > 0
    rows = got["read"] == 2
    assert rows.sum() == 3 and (got["kind"][rows] == 3).all()
    assert got["motif_windows"][rows].tolist() == [int(by_tile[c]) for c in classes_of(case["motifs"])[0]]
    # 4096 and 4097 windows: the run's last window is position 4095, then 4096 (a tile of its own)
    assert got["motif_windows"][got["read"] == 0].tolist() == [46]
    assert got["motif_windows"][got["read"] == 1].tolist() == [47]


def test_full_lds_map_and_read_order(capi):
    case = cases.full_map_case()
    members = classes_of(case["motifs"])[1]
    assert len(members) == 150
    assert (class_windows([case["reads"][1]], 15, members)[0] > 0).sum() > cases.LDS_MAP   # one tile, > 128 classes
    got, _ = _gpu(case)
    want = _ref(case)
    _same(got, want)
    assert len(got["read"]) == 7 * 150 and (got["kind"] == 0).all()
    perm = cases.full_map_case(permute=True)
    got_p, _ = _gpu(perm)
    for new, old in enumerate(cases.FULL_MAP_PERMUTATION):
        for key in KEYS[1:]:
            assert np.array_equal(got_p[key][got_p["read"] == new], got[key][got["read"] == old]), (key, new)


def test_kinds_on_a_panel(capi):
    from nanorepeat_amd.screen import Screen
    case = cases.kinds_case()
    want = _ref(case)
    with Screen(case["anchors"], k=case["k"], max_occ=case["max_occ"], motifs=case["motifs"]) as scr:
        got = scr.screen_reads_partial(case["reads"], case["min_hits"], case["pct"])
        plain = scr.screen_reads(case["reads"], case["min_hits"])
        assert scr.stats()["n_empty_regions"] == 1
    _same(got, want)
    for kd in (0, 1, 2, 3):
        assert (got["kind"] == kd).sum() >= 3, kd
    zero = got["kind"] == 0
    for key in ("read", "region", "hits_left", "hits_right"):
        assert np.array_equal(got[key][zero], plain[key]), key


def test_two_calls_capacity_and_set_motifs_twice(capi):
    from nanorepeat_amd.screen import Screen
    case = cases.kinds_case()
    reads, half = case["reads"], len(case["reads"]) // 2
    ref = RefScreenPartial(case["anchors"], motifs=case["motifs"])
    with Screen(case["anchors"], motifs=case["motifs"]) as scr:
        _same(scr.screen_reads_partial(reads[:half], 4, 5), ref.screen_reads_partial(reads[:half], 4, 5))
        _same(scr.screen_reads_partial(reads[half:], 4, 5), ref.screen_reads_partial(reads[half:], 4, 5))
        st = scr.stats()
        assert st["n_calls"] == 2 and st["sum_motif_kernel_ms"] >= st["motif_kernel_ms"] > 0
        want = ref.screen_reads_partial(reads, 4, 5)
        n_want = len(want["read"])
        lib = capi.load()
        seqs, off = capi.pack_reads(reads)
        out = [np.full(n_want, -7, np.int32) for _ in range(5)]
        kind = np.full(n_want, 77, np.uint8)

        def call(cap):
            n = C.c_int64(cap)
            rc = lib.nra_screen_reads_partial(scr._h, len(reads), seqs, capi._ptr(off, C.c_int64), 4, 5, C.byref(n),
                                              *(capi._ptr(x, C.c_int32) for x in out), capi._ptr(kind, C.c_uint8))
            return rc, n.value
        assert call(n_want - 1) == (capi.E_RANGE, n_want)
        assert all((x == -7).all() for x in out) and (kind == 77).all()             # nothing written
        assert call(n_want) == (0, n_want)
        for x, key in zip(out + [kind], KEYS):
            assert np.array_equal(x, want[key]), key
        _same(capi.screen_reads_partial(scr._h, reads, 4, 5, capacity=3), want)      # the binding's retry
        # other motifs replace the first: every region of the class of CAG
        scr.set_motifs(["CAG"] * 6 + ["CTGCTG"] * 6)
        ref.set_motifs(["CAG"] * 6 + ["CTGCTG"] * 6)
        assert scr.stats()["n_classes"] == 1
        _same(scr.screen_reads_partial(reads, 4, 5), ref.screen_reads_partial(reads, 4, 5))


def test_without_motifs_no_pair_is_in_repeat(capi):
    from nanorepeat_amd.screen import Screen
    case = cases.kinds_case()
    with Screen(case["anchors"]) as scr:
        got = scr.screen_reads_partial(case["reads"], 4, 5)
        assert scr.stats()["motif_kernel_ms"] == 0
    _same(got, RefScreenPartial(case["anchors"]).screen_reads_partial(case["reads"], 4, 5))
    assert not (got["kind"] == 3).any() and (got["kind"] == 1).any() and (got["motif_windows"] == 0).all()


def test_bad_arguments_on_a_device(capi):
    from nanorepeat_amd.screen import Screen
    anchors = [("ACGTTGCAAGTCCATGACTTGA", "TTGACCATGACCAGTACAGGAT")] * 2

    def code(fn, *a, **kw):
        with pytest.raises(capi.NraError) as e:
            fn(*a, **kw)
        return e.value.code
    with Screen(anchors) as scr:
        assert code(scr.set_motifs, ["CAG"]) == -1                   # one motif, two regions
        assert code(scr.set_motifs, ["CAG", ""]) == -1
        assert code(scr.set_motifs, ["CAG", "CANG"]) == -1
        assert code(scr.set_motifs, ["CAG", "ACGTC" * 13]) == capi.E_RANGE
        scr.set_motifs(["cag", "ACGTC" * 12 + "ACGT"])               # lower case and 64 bases are fine
        assert scr.stats()["n_classes"] == 1
        assert code(scr.screen_reads_partial, ["ACGT"], min_hits=0) == -1
        assert code(scr.screen_reads_partial, ["ACGT"], motif_share_pct=0) == -1
        assert code(scr.screen_reads_partial, ["ACGT"], motif_share_pct=101) == -1
        got = scr.screen_reads_partial(["", "ACG"], 4, 100)
        assert len(got["read"]) == 0


# ---------------------------------------------------------------------------- end to end
def test_fastq_command_finds_the_allele_no_read_spans(capi, tmp_path, capsys):
    """quantify_from_reads(partial_reads=True, in_repeat_reads=True) on the device: the panel's checks (the long allele
    shows in region 0 only, every other file unchanged, the same files without the screen), and the one-anchor and
    in-repeat reads the CPU engines find."""
    import in_repeat_panel
    regions, names, _ = in_repeat_panel.run_and_check(tmp_path, capsys)
    assert sorted(regions[0].one_anchor_reads) == sorted(names["left"] + names["right"])
    assert sorted(regions[0].in_repeat_reads) == sorted(names["inside"])
