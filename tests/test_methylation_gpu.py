"""nra_read_methylation on the device equals the restatement (tests/methylation_ref.py) exactly: counts, n_c and status,
at the smallest shapes at which the kernel can go wrong, through several chunks, in either read order and either
orientation, on one read of the largest length, and through both commands."""
import sys
import time

import numpy as np
import pytest

import methylation_cases as K
import methylation_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("counts", "n_c", "status")


def same(got, want, note=""):
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (key, note)


@pytest.fixture(scope="module")
def edges():
    """The edge batch (every length x both flag bits, lists and tracts of every kind) and its reference per shape."""
    batch = K.edge_batch()
    return batch, {shape: K.call(R.ref_read_methylation, batch, *shape) for shape in K.SHAPES}


def test_hand_counted_case(capi):
    from test_methylation_cpu import HAND_WANT, hand_call
    out, bits = hand_call(capi.read_methylation)
    for i, b in enumerate(bits):
        assert out["counts"][i].tolist() == HAND_WANT[b], b
    assert out["n_c"].tolist() == [7] * 4 and out["status"].tolist() == [0] * 4


@pytest.mark.parametrize("shape", K.SHAPES)
def test_edge_lengths_lists_and_tracts(capi, edges, shape):
    batch, want = edges
    same(K.call(capi.read_methylation, batch, *shape), want[shape], shape)
    assert want[shape]["counts"][:, :, 1].sum() > 0 and set(want[shape]["status"].tolist()) == {0, 1}


def test_every_list_kind(capi):
    batch = K.kinds_batch()
    want = K.call(R.ref_read_methylation, batch)
    same(K.call(capi.read_methylation, batch), want)
    assert want["status"][-2:].tolist() == [0, 1]                       # L_{m-1} = n_c - 1 next to n_c
    assert want["status"].reshape(-1)[:32].reshape(8, 4).all(axis=1).tolist() == [False] * 5 + [True] * 3


def test_read_order_does_not_matter(capi, edges):
    batch, want = edges
    order = np.random.default_rng(3).permutation(len(batch["reads"]))
    got = K.call(capi.read_methylation, K.take(batch, order))
    for key in KEYS:
        assert np.array_equal(got[key], want[K.SHAPES[0]][key][order]), key


def test_small_chunks_and_a_read_that_goes_alone(capi, edges, monkeypatch, capfd):
    """A budget of 40 000 bytes: the 70 001-base reads go alone, the others in several chunks."""
    batch, want = edges
    monkeypatch.setenv("NRA_TEST_METH_BYTES", "40000")
    monkeypatch.setenv("NRA_DEBUG", "1")
    capfd.readouterr()
    got = K.call(capi.read_methylation, batch)
    lines = [l for l in capfd.readouterr().err.split("\n") if l.startswith("nra_read_methylation: chunk of")]
    same(got, want[K.SHAPES[0]])
    assert len(lines) > 8 and sum("chunk of 1 read(s), 70001 base(s)" in l for l in lines) == 4
    assert sum(int(l.split()[3]) for l in lines) == len(batch["reads"])


def test_orientation_invariance_on_the_device(capi, edges):
    batch, _ = edges
    for shape in K.SHAPES[:3]:
        a, b = K.call(capi.read_methylation, batch, *shape), K.call(capi.read_methylation, K.mirrored(batch), *shape)
        assert np.array_equal(a["counts"], K.swap_sides(b["counts"])), shape
        assert np.array_equal(a["n_c"], b["n_c"]) and np.array_equal(a["status"], b["status"])


# One workgroup walks the 4 000 000 bases in 15 625 tiles and the list of about 250 000 entries in about 1 000.  Measured
# on an MI355X: the kernel 11.2 ms, the call from host arrays to host arrays 12.2 ms.  The limit
# is a hundred times the call: a run beyond it has gone wrong, not slow.
LONGEST_READ_LIMIT_S = 1.25


def test_the_longest_read(capi):
    from test_methylation_cpu import hand_call
    hand_call(capi.read_methylation)                 # the device and the code object are loaded outside the timed call
    rng = np.random.default_rng(9)
    n = 4000000
    s = rng.choice(np.frombuffer(b"ACGTacgN", np.uint8), size=n, p=[.22, .25, .25, .22, .02, .02, .01, .01])
    stored = s.tobytes().decode()
    for bits in (1, 2):
        up = s & 0xDF
        is_c = (up[::-1] == ord("G")) if bits & 1 else (up == ord("C"))
        ranks = np.flatnonzero(is_c)
        listed = np.sort(rng.choice(len(ranks), size=len(ranks) // 4, replace=False))
        deltas = np.diff(np.concatenate([[-1], listed])) - 1
        mods = [(deltas.astype(np.int32), rng.integers(0, 256, len(listed)).astype(np.uint8))]
        args = ([stored], mods, np.array([bits], np.uint8), np.array([1999000], np.int32), np.array([2001001], np.int32))
        kw = dict(flank=100000, bin=2000, lo_byte=K.LO_BYTE, hi_byte=K.HI_BYTE)
        t0 = time.perf_counter()
        got = capi.read_methylation(*args, **kw)
        took = time.perf_counter() - t0
        print(f"4 000 000 bases, flags {bits}: {took:.3f} s")
        same(got, R.np_read_methylation(*args, **kw), bits)
        assert got["status"][0] == 0 and got["counts"][0, :, 1].min() > 0
        assert took < LONGEST_READ_LIMIT_S


def test_commands_give_the_same_files_as_through_the_restatement(capi, oracle, tmp_path, monkeypatch, capsys):
    from test_methylation_cpu import check_command_files, run_commands
    from test_screen_cpu import _tree
    monkeypatch.setitem(sys.modules, "pysam", None)
    truth = K.command_case(tmp_path)
    capsys.readouterr()
    dev_bam, dev_fq, _ = run_commands(tmp_path, oracle, None, "dev")
    err = capsys.readouterr().err
    run_commands(tmp_path, oracle, R.ref_read_methylation, "ref")
    check_command_files(str(tmp_path / "bam_dev"), dev_bam, truth, err)
    check_command_files(str(tmp_path / "fq_dev"), dev_fq, truth, err)
    for kind in ("bam", "fq"):
        assert _tree(tmp_path / f"{kind}_dev.details") == _tree(tmp_path / f"{kind}_ref.details")
        assert ((tmp_path / f"{kind}_dev.NanoRepeat_methylation.tsv").read_bytes() ==
                (tmp_path / f"{kind}_ref.NanoRepeat_methylation.tsv").read_bytes())
