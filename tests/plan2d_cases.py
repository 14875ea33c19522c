"""Inputs of the 2D plan test (tests/test_plan2d_cpu.py): name -> the arguments of nanorepeat_amd._capi.plan2d_digest.  The
step sequences are those of the GPU tests that drive the same paths (tests/test_gpu_parity.py: resident reads across cell
lists, a routed grid against its cell list, a finer grid from kept column states, the refinement), so that the CPU pin and
the GPU parity cover the same ground.  Everything is seeded; 10 - 20 reads of about 500 bases unless a case says otherwise."""
import functools

import numpy as np

from nanorepeat_amd import _capi as A, synth

# bytes of column states the coarse grid of `finer_grid` keeps for its 17 reads (keep_bytes in the digest; the test checks it)
COARSE_KEEP_BYTES = 4294144


def joint(n, seed, **kw):
    kw = dict(dict(alleles=((9, 5), (14, 3)), read_len=520, read_sd=30, anchor=300), **kw)
    return synth.make_joint(n, seed=seed, **kw)


def case(j, steps, flags=0, sc=None, region=None, reads=None):
    return dict(region=region or j["region"], reads=reads if reads is not None else j["reads"], steps=steps, flags=flags,
                sc=sc or {})


def cells_step(cells, strand=None, **kw):
    return dict(kind="cells", cells=cells, strand=strand, **kw)


def grid_step(grid, strand=None, **kw):
    return dict(kind="grid", grid=grid, strand=strand, **kw)


def window_cells(j, step=1, shift=0, sit_out=True):
    """the cell lists of test_joint_resident_reads_across_cell_lists"""
    cr, k1, k2 = [], [], []
    for r in range(len(j["reads"])):
        if sit_out and (r + shift) % 4 == 3:
            continue                                   # some reads sit a list out
        for a in range(max(0, int(j["truth"][r][0]) - 4 + shift), int(j["truth"][r][0]) + 5, step):
            for b in range(max(0, int(j["truth"][r][1]) - 2), int(j["truth"][r][1]) + 3, step):
                cr.append(r); k1.append(a); k2.append(b)
    return cr, k1, k2


def truth_grid(j, a1=(2, 3, 7), a2=(0, 2, 6)):
    t1, t2 = j["truth"][:, 0].astype(np.float64), j["truth"][:, 1].astype(np.float64)
    return A.Grid(a1, t1 - 5, t1 + 6, a2, t2 - 3, t2 + 4)


def finer_grid_parts(n=17, seed=75):
    """the grids of test_joint_finer_grid_from_kept_column_states"""
    j = joint(n, seed, alleles=((11, 6), (21, 4)), read_len=640, read_sd=60, anchor=330)
    t1, t2 = j["truth"][:, 0].astype(np.float64), j["truth"][:, 1].astype(np.float64)
    strands = j["strand"].astype(np.int8)
    flipped = strands.copy(); flipped[3] = -flipped[3]
    lo1, hi1, lo2, hi2 = t1 - 9, t1 + 8, np.maximum(t2 - 5, 0), t2 + 5
    coarse = A.Grid((1, 4, 9), lo1, hi1, (0, 3, 5), lo2, hi2)
    size1, size2 = t1 + np.arange(n) % 3 - 1 + 0.5 * (np.arange(n) % 2), t2 + np.arange(n) % 2
    fine = A.Grid((0, 1, 40), np.maximum(size1 - 4, lo1), np.minimum(size1 + 4, hi1),
                  (0, 1, 16), np.maximum(size2 - 3, lo2), np.minimum(size2 + 3, hi2))
    wider = A.Grid((0, 1, 40), lo1 - 3, hi1 + 3, (0, 1, 16), lo2, hi2 + 2)      # beyond what was kept
    return j, strands, flipped, coarse, fine, wider, (lo1, hi1, lo2, hi2)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    # the five cell lists of test_joint_resident_reads_across_cell_lists
    j = joint(10, 73)
    true_strand = j["strand"].astype(np.int8)
    flipped = true_strand.copy(); flipped[[1, 4]] *= -1
    lists = [cells_step(window_cells(j, step, shift), st) for step, shift, st in
             ((2, 0, true_strand), (1, 1, true_strand), (1, 0, flipped), (1, 2, None), (2, 1, true_strand))]
    out["cell_lists"] = case(j, lists)

    # the four rounds and the empty grid of test_joint_routed_grid_equals_its_cell_list
    j = joint(14, 74)
    n = len(j["reads"])
    t1, t2 = j["truth"][:, 0].astype(np.float64), j["truth"][:, 1].astype(np.float64)
    strands = j["strand"].astype(np.int8)
    rounds = [((2, 3, 7), t1 - 5, t1 + 6, (0, 2, 6), t2 - 3, t2 + 4, strands),
              ((5, 1, 14), t1 - 1.5, t1 + 1.5, (1, 1, 8), t2 - 1 / 3, t2 + 2.5, strands),
              ((0, 4, 6), t1 - 8, t1 + 3, (0, 1, 9), np.where(np.arange(n) % 5 == 2, 99.0, t2 - 2), t2 + 2, None),
              ((3, 1, 20), t1 - 2, t1 + 2.5, (2, 1, 2), t2 - 9, t2 + 9, strands)]
    steps = [grid_step(A.Grid(a1, lo1, hi1, a2, lo2, hi2), st) for a1, lo1, hi1, a2, lo2, hi2, st in rounds]
    steps.append(grid_step(A.Grid((0, 1, 4), t1 + 50, t1 + 60, (0, 1, 4), t2, t2 + 1), strands))
    out["routed_grid"] = case(j, steps)
    out["routed_grid_no_chain"] = case(j, steps, flags=A.F_JOINT_NO_CHAIN)
    out["routed_grid_tails"] = case(j, steps, flags=A.F_JOINT_TAILS)

    # the ten steps of test_joint_finer_grid_from_kept_column_states
    j, strands, flipped, coarse, fine, wider, bounds = finer_grid_parts()
    steps = [grid_step(coarse, strands), grid_step(fine, strands), grid_step(fine, strands), grid_step(fine, flipped),
             grid_step(fine, flipped), grid_step(wider, flipped), grid_step(coarse, strands), dict(kind="invalidate"),
             grid_step(fine, strands), grid_step(fine, None)]
    out["finer_grid"] = case(j, steps)
    out["finer_grid_no_keep"] = case(j, steps, flags=A.F_JOINT_NO_KEEP)

    # the keep budget: none, one byte below the need, the need; then an arena that already holds enough (other strands, so
    # that the states are made again: the device is not asked although it has nothing free)
    need = COARSE_KEEP_BYTES
    out["keep_budget"] = case(j, [grid_step(coarse, strands, budget=0), grid_step(coarse, strands, budget=need - 1),
                                  grid_step(coarse, strands, budget=need), grid_step(coarse, flipped, free=0)])
    # free memory below twice the need, and at it
    out["keep_free"] = case(j, [grid_step(coarse, strands, free=2 * need - 1), grid_step(coarse, strands, free=2 * need)])

    # sweep-flanks before a grid: every strand given (and a second time, nothing stale), some strands 0
    some = strands.copy(); some[[2, 5, 6]] = 0
    out["flanks_then_grid"] = case(j, [dict(kind="sweep_flanks", strand=strands), dict(kind="sweep_flanks", strand=strands),
                                       grid_step(coarse, strands)])
    out["flanks_some_strands"] = case(j, [dict(kind="sweep_flanks", strand=some), grid_step(coarse, some),
                                          grid_step(coarse, strands)])

    # a refinement behind a keeping grid with buf = its steps (and a second one: not in this state), and the other exits
    refine = dict(kind="refine", bounds=bounds, buf=(4, 3))
    out["refine"] = case(j, [grid_step(coarse, strands), refine, refine, grid_step(fine, strands), refine])
    out["refine_no_kept_states"] = case(j, [grid_step(coarse, strands), refine], flags=A.F_JOINT_NO_KEEP)
    wide = (bounds[0] - 10, bounds[1] + 10, bounds[2], bounds[3] + 10)
    out["refine_leaves_kept_range"] = case(j, [grid_step(coarse, strands), dict(kind="refine", bounds=wide, buf=(9, 7))])
    out["refine_not_a_routed_grid"] = case(j, [cells_step(A.joint_grid_cells(coarse), strands), refine])
    rng = np.random.default_rng(9201)
    long_reads = list(j["reads"]); long_reads[4] = synth.rand_seq(rng, 3200)       # above NRA_MAX_QLEN_1BLOCK = 3072
    out["refine_chained_bucket"] = case(j, [grid_step(coarse, strands), refine], reads=long_reads)

    # one read above NRA_MAX_QLEN_1BLOCK among short ones: a chain bucket, probe shadows, chain_cap
    out["long_read"] = case(j, [cells_step(window_cells(j, sit_out=False), None), cells_step(window_cells(j), strands),
                                grid_step(coarse, strands)], reads=long_reads)

    # flags and flanks that change the form of a list
    j = joint(12, 76)
    strands = j["strand"].astype(np.int8)
    both = [cells_step(window_cells(j), strands), grid_step(truth_grid(j), strands), cells_step(window_cells(j, 2, 1), None)]
    out["brute_force"] = case(j, both, flags=A.F_BRUTE_FORCE)
    left, u1, mid, u2, right = j["region"]
    out["left_flank_0"] = case(j, both, region=("", u1, mid, u2, right))
    out["right_flank_1"] = case(j, both, region=(left, u1, mid, u2, right[:1]))
    # flanks too short for the packed sweeps (fewer than 64 columns outside the window): one side packed, the other not
    out["short_left_flank"] = case(j, both, region=(left[-40:], u1, mid, u2, right))
    out["short_right_flank"] = case(j, both, region=(left, u1, mid, u2, right[:40]))
    out["test_chain"] = case(j, both, flags=A.F_TEST_CHAIN)                      # one group per read
    out["no_joint_pack"] = case(j, both, flags=A.F_NO_JOINT_PACK)
    out["scoring_not_packed"] = case(j, both, sc=dict(mismatch=8))               # gap_open1 + gap_ext1 < mismatch

    # an empty read with cells, a read with no cells; an odd read count in a bucket (read_b = -1)
    j = joint(11, 77)
    strands = j["strand"].astype(np.int8)
    reads = list(j["reads"]); reads[3] = ""
    cr, k1, k2 = window_cells(j, sit_out=False)
    drop = np.asarray(cr) != 6
    cl = tuple(np.asarray(a)[drop] for a in (cr, k1, k2))
    lo_none = truth_grid(j)
    lo_none.bounds[0][6] = 99.0                                                   # read 6: no grid value
    out["empty_read_and_no_cells"] = case(j, [cells_step(cl, strands), cells_step(cl, None), grid_step(lo_none, strands)],
                                          reads=reads)
    out["odd_read_count"] = case(j, [cells_step(window_cells(j, sit_out=False), strands), grid_step(truth_grid(j), strands)])

    # reads of about 500 and about 1500 bases together: two rows-per-lane classes, a nonzero state_base
    rng = np.random.default_rng(9202)
    reads = list(j["reads"])
    for r in (1, 4, 8, 9):
        reads[r] = synth.rand_seq(rng, 500) + reads[r] + synth.rand_seq(rng, 500)
    out["two_row_classes"] = case(j, [cells_step(window_cells(j, sit_out=False), strands), grid_step(truth_grid(j), strands),
                                      dict(kind="sweep_flanks", strand=-strands), grid_step(truth_grid(j), -strands)], reads=reads)

    # the errors
    j = joint(10, 78)
    strands = j["strand"].astype(np.int8)
    cr, k1, k2 = (np.asarray(a) for a in window_cells(j, sit_out=False))
    swapped = cr.copy(); swapped[[0, -1]] = swapped[[-1, 0]]
    neg = k2.copy(); neg[7] = -1
    ok = cells_step((cr, k1, k2), strands)
    out["error_cells_not_grouped"] = case(j, [ok, cells_step((swapped, k1, k2), strands), ok])
    out["error_negative_k"] = case(j, [cells_step((cr, k1, neg), strands)])
    far = k1.copy(); far[3] = 2000                                                # 6 * (3 * 2000 + ...) >= 32768
    out["error_window_too_long"] = case(j, [cells_step((cr, far, k2), strands)])
    rng = np.random.default_rng(9203)
    left, u1, mid, u2, right = j["region"]
    far = k1.copy(); far[3] = 1000                                                # 62000 + 3043 > NRA_MAX_TLEN = 65000
    out["error_template_too_long"] = case(j, [cells_step((cr, far, k2), strands)],
                                          region=(synth.rand_seq(rng, 31000), u1, mid, u2, synth.rand_seq(rng, 31000)))
    big = np.full(len(j["reads"]), 1e9)
    out["error_too_many_cells"] = case(j, [grid_step(A.Grid((0, 1, 20000), -big, big, (0, 1, 20000), -big, big), strands)])
    return out


def digest(c):
    """The digest text of a case."""
    return A.plan2d_digest(c["region"], c["reads"], c["steps"], sc=A.default_scoring(**c["sc"]), flags=c["flags"])
