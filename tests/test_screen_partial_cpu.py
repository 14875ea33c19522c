"""The motif screen's contract on the CPU: the two restatements of tests/screen_partial_ref.py against each other on
the GPU tests' inputs, the class rules, kind 0 against tests/screen_ref.py, and the measurement behind the default
motif_share_pct."""
import ctypes as C

import numpy as np
import pytest

import screen_partial_cases as cases
from nanorepeat_amd import synth
from screen_partial_ref import (RefScreenPartial, as_tuples, class_windows, classes_of, motif_root,
                                plain_screen_partial)
from screen_ref import RefScreen, plain_screen
from screen_ref import as_tuples as as_tuples4

CASES = {"edges11": lambda: cases.edge_case(11), "edges15": lambda: cases.edge_case(15), "tiles": cases.tile_case,
         "full_map": cases.full_map_case, "kinds": cases.kinds_case}


def _numpy(case, motifs=True):
    ref = RefScreenPartial(case["anchors"], k=case["k"], max_occ=case["max_occ"],
                           motifs=case["motifs"] if motifs else None)
    return ref.screen_reads_partial(case["reads"], case["min_hits"], case["pct"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_restatement_equals_plain_python(name):
    case = CASES[name]()
    got = _numpy(case)
    want = plain_screen_partial(case["anchors"], case["motifs"], case["reads"], case["k"], case["max_occ"],
                                case["min_hits"], case["pct"])
    assert as_tuples(got) == want
    assert len(want) > 0


def test_the_cases_hold_what_they_are_for():
    for k in (11, 15):
        got = _numpy(cases.edge_case(k))
        assert (got["kind"] == 3).sum() >= 20 and (got["kind"] == 1).sum() >= 1
    got = _numpy(cases.kinds_case())
    assert all((got["kind"] == kd).sum() >= 3 for kd in (0, 1, 2, 3))
    got = _numpy(cases.tile_case())
    assert got["motif_windows"][got["read"] == 0].tolist() == [46]
    assert got["motif_windows"][got["read"] == 1].tolist() == [47]
    assert (got["read"] == 2).sum() == 3 and (got["kind"] == 3).all()
    case = cases.full_map_case()
    members = classes_of(case["motifs"])[1]
    assert (class_windows([case["reads"][1]], 15, members)[0] > 0).sum() > cases.LDS_MAP


def test_class_rules():
    assert motif_root("CAGCAG") == "CAG" and motif_root("cag") == "CAG" and motif_root("ACACACAT") == "ACACACAT"
    class_of, members = classes_of(["CAG", "CAGCAG", "CTG", "GCA", "AAAAAAC", "AAAG", "CTTT", "GGCCTCAGGCCTCA", "A", "T"])
    assert class_of == [0, 0, 0, 0, -1, 1, 1, -1, 2, 2]
    assert len(members) == 3 and members[0] == {"CAG", "AGC", "GCA", "CTG", "TGC", "GCT"}


def test_kind0_pairs_equal_the_anchor_screen():
    case = cases.kinds_case()
    for motifs in (True, False):
        got = _numpy(case, motifs)
        zero = got["kind"] == 0
        ref = RefScreen(case["anchors"], k=case["k"], max_occ=case["max_occ"]).screen_reads(case["reads"], case["min_hits"])
        assert [t[:4] for t, z in zip(as_tuples(got), zero) if z] == as_tuples4(ref)
        if not motifs:
            assert not (got["kind"] == 3).any() and (got["motif_windows"] == 0).all()
    small = dict(case, reads=case["reads"][:12])
    got = _numpy(small)
    want = plain_screen(small["anchors"], small["reads"], small["k"], small["max_occ"], small["min_hits"])
    assert [t[:4] for t in as_tuples(got) if t[5] == 0] == want


# ----------------------------------------------------------------------------------- the default motif_share_pct
SHARE_MOTIFS = ("A", "AC", "GAA", "CAG", "AAAG", "AAGGG", "GGCCCC")     # every period 1..6
N_SHARE_READS = 200


def share_table(n_reads=N_SHARE_READS, seed=2):
    """[(k, model or 'decoy', motif, lowest share %, median share %)]: the share of class windows m / W of wholly
    in-repeat reads (lengths 300..3000, both strands), and of decoys (5 kb random reads holding (motif)20); for a
    decoy 'lowest' holds the highest share."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in (11, 15):
        for model in ("ont", "hifi", "decoy"):
            for motif in SHARE_MOTIFS:
                members = classes_of([motif])[1]
                reads = []
                for i in range(n_reads):
                    if model == "decoy":
                        run = motif * 20
                        at = int(rng.integers(0, 5000 - len(run)))
                        s = synth.rand_seq(rng, at) + run + synth.rand_seq(rng, 5000 - len(run) - at)
                    else:
                        n = int(rng.integers(300, 3001))
                        s = synth.apply_errors(rng, (motif * (n // len(motif) + 2))[i % len(motif):][:n], model)
                    reads.append(synth.revcomp(s) if i % 2 else s)
                w = np.array([len(s) - k + 1 for s in reads])
                share = 100.0 * class_windows(reads, k, members)[:, 0] / w
                rows.append((k, model, motif, float(share.max() if model == "decoy" else share.min()),
                             float(np.median(share))))
    return rows


def test_share_table_and_the_default_motif_share_pct():
    import inspect
    from nanorepeat_amd import pipeline
    default = inspect.signature(pipeline.quantify_from_reads).parameters["motif_share_pct"].default
    rows = share_table()
    print("\nk  reads  motif   lowest% (decoy: highest%)  median%")          # shown with pytest -s
    for k, model, motif, edge, med in rows:
        print(f"{k:<3}{model:<7}{motif:<8}{edge:8.2f}{med:10.2f}")
    lowest_planted = min(e for k, model, _, e, _ in rows if k == 15 and model == "ont")
    highest_decoy = max(e for _, model, _, e, _ in rows if model == "decoy")
    assert min(e for _, model, _, e, _ in rows if model == "hifi") > lowest_planted
    assert default <= lowest_planted / 2, (default, lowest_planted)
    assert default > 2 * highest_decoy, (default, highest_decoy)


def test_null_handle_is_an_argument_error(capi):
    lib = capi.load()
    data, off = capi.pack_reads(["CAG"])
    assert lib.nra_screen_set_motifs(None, 1, data, capi._ptr(off, C.c_int64)) == -1
    n = C.c_int64(0)
    assert lib.nra_screen_reads_partial(None, 0, None, None, 4, 5, C.byref(n), *(None,) * 6) == -1
    assert {"nra_screen_set_motifs", "nra_screen_reads_partial"} <= set(capi.EXPORTS)
