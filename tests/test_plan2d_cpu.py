"""The plan of a joint (2D) cell list (nra_plan2d.cpp: what is fixed when the reads are packed, what a batch carries from
one list to the next, the keep decision, the buckets, the strand-only and the cell tasks, the groups, the statistics; the
flank sweeps ahead of a list; the refinement's checks and static tasks) is pinned, bit for bit, to what the batch functions
made before the plan was split from its upload: tests/golden/plan2d.json holds, per case of tests/plan2d_cases.py, the
digest text nra_plan2d_digest gives for the case's steps (per step the scalars, one line per bucket and per group, length
and FNV-1a hash per array of the plan and of the carried state, or the error code and text), recorded from that earlier
commit with the same digest writer patched into its function bodies.  No device is needed.

Branches no small input reaches, so that none of these cases pins them: a group of reads closed because the wave states
of a bucket exceed NRA_JOINT_STATE_CAP_INTS (4 G int32; NRA_F_TEST_CHAIN closes one per read instead); packed wave states
beyond 4 GB switching the packed sweeps off; kept column states whose template would exceed NRA_MAX_TLEN; fewer payload
strips than NRA_CHAIN_STRIPS because of NRA_CHAIN_SCRATCH_BUDGET; the refinement's exits "the current cell list is not a
routed grid" and "a read's bucket did not run", which the state check before them catches first (a refinement behind a
cell list says what one without kept states says); the second try of nra_batch2d_set_grid after NRA_E_NOMEM (keep_off),
which only a device's allocation failure starts."""
import json
import os

import pytest

import plan2d_cases as P

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan2d.json")))
E_ARG, E_RANGE, E_STATE = -1, -3, -5


def test_the_golden_holds_every_case():
    assert sorted(GOLDEN) == sorted(P.cases())


@pytest.mark.parametrize("name", sorted(P.cases()))
def test_plans_are_the_recorded_plans(capi, name):
    assert P.digest(P.cases()[name]) == GOLDEN[name]


def parse(text):
    """-> (the reads' scalars, [per step: dict of its lines; `buckets` / `groups` / `parts`: lists of dicts])"""
    head, *rest = text.split("\nstep ")
    reads = dict(line.partition(" ")[::2] for line in head.splitlines())
    steps = []
    for block in rest:
        first, *lines = block.splitlines()
        d = {"kind": int(first.split()[2]), "buckets": [], "groups": [], "parts": []}
        for line in lines:
            key, _, value = line.partition(" ")
            for what in ("bucket", "group", "part"):
                if key.startswith(what) and key[len(what):].isdigit():
                    d[what + "s"].append({k: int(v) for k, v in (kv.split("=") for kv in value.split())})
                    break
            else:
                d[key] = value
        steps.append(d)
    return reads, steps


@pytest.fixture(scope="module")
def plans():
    return {name: parse(text) for name, text in GOLDEN.items()}


def lists(plans, name=None):
    """the cell-list and grid steps that made a plan"""
    return [s for n, (_, steps) in plans.items() if name in (None, n) for s in steps if "keep" in s]


def test_the_golden_covers_every_form_of_a_list(plans):
    every = lists(plans)

    def some(f):
        return any(f(s) for s in every)

    for keep in "012":
        assert some(lambda s: s["keep"] == keep)
    assert some(lambda s: s["joint_v2"] == "1") and some(lambda s: s["joint_v2"] == "0")
    assert some(lambda s: s["joint_chain"] == "1") and some(lambda s: s["joint_v2"] == "1" and s["joint_chain"] == "0")
    assert some(lambda s: s["brute"] == "1") and some(lambda s: s["cells_need_clear"] == "0")
    assert some(lambda s: s["all_strands_given"] == "0" and any(b["n_pair"] for b in s["buckets"]))
    # a chain bucket with its probe shadows; a bucket with more than one group; two rows-per-lane classes
    assert some(lambda s: any(b["chain"] and b["n_probe"] and b["n_queue"] for b in s["buckets"]) and int(s["chain_cap"]) > 0)
    assert some(lambda s: len(s["groups"]) > len(s["buckets"]))
    assert some(lambda s: len([b for b in s["buckets"] if not b["chain"]]) == 2 and s["groups"][1]["R"] != s["groups"][0]["R"])
    # packed sweeps present and absent on each side
    for l, r in ((1, 1), (1, 0), (0, 1), (0, 0)):
        assert some(lambda s: s["brute"] == "0" and [sum(b[k] for b in s["buckets"]) > 0 for k in ("n_jlpk", "n_jrpk")] == [l, r]), (l, r)
    # everything reused: a list that sweeps (keep 0 or 1) and one that does not (keep 2) with nothing pending
    for keeps in ("01", "2"):
        assert some(lambda s: s["keep"] in keeps and s["brute"] == "0" and int(s["n_alignments"]) > 0 and
                    [s[k].split()[0] for k in ("rev_pending", "lst_pending", "rpk_pending")] == ["0"] * 3), keeps
    # the device is asked only when the budget holds and the arena does not
    assert some(lambda s: s["keep"] == "1" and s["device_asked"] == "0")
    assert not some(lambda s: s["device_asked"] == "1" and s["keep"] == "2")


def test_the_golden_shows_what_each_case_is_for(plans):
    def keeps(name):
        return [s["keep"] for s in lists(plans, name)]

    def errors(name):
        return [int(s["error"].split()[0]) if "error" in s else 0 for s in plans[name][1]]

    assert keeps("cell_lists") == ["0"] * 5 and keeps("finer_grid_no_keep") == ["0"] * 9
    assert keeps("finer_grid") == list("122121110")         # sweeps, kept, kept, sweeps, kept, sweeps, sweeps, sweeps, probed
    assert keeps("routed_grid_no_chain") == keeps("routed_grid_tails") == ["0"] * 5
    assert [s["n_alignments"] for s in lists(plans, "routed_grid")][-1] == "0"
    # the budget: none, one byte short, exact; then made again from an arena that holds enough, the device not asked
    budget = lists(plans, "keep_budget")
    assert [s["keep"] for s in budget] == list("0011") and [s["device_asked"] for s in budget] == list("0010")
    assert {s["keep_bytes"] for s in budget} == {str(P.COARSE_KEEP_BYTES)}
    free = lists(plans, "keep_free")
    assert [s["keep"] for s in free] == list("01") and [s["device_asked"] for s in free] == list("11")
    # flank sweeps ahead of a list: the second finds nothing stale, the grid behind them sweeps no flank
    (_, (a, b, grid)) = plans["flanks_then_grid"]
    assert a["parts"] and not b["parts"] and int(a["warm_cells"]) > 0 and b["warm_cells"] == "0"
    assert not any(bk["n_jlpk"] or bk["n_jrpk"] for bk in grid["buckets"])
    some = plans["flanks_some_strands"][1]
    assert 0 < int(some[0]["l_done"].split()[0]) < 17 and any(bk["n_jlpk"] for bk in some[1]["buckets"])
    # the refinement and its exits
    assert errors("refine") == [0, 0, E_STATE, 0, 0] and "rf_mid" in plans["refine"][1][1]
    for name in ("refine_no_kept_states", "refine_leaves_kept_range", "refine_chained_bucket", "refine_not_a_routed_grid"):
        assert errors(name) == [0, E_STATE], name
    assert "no column state was kept" in plans["refine_leaves_kept_range"][1][1]["error"]
    assert "register block" in plans["refine_chained_bucket"][1][1]["error"]
    # the forms
    for name in ("brute_force", "left_flank_0", "right_flank_1"):
        assert {s["brute"] for s in lists(plans, name)} == {"1"}, name
    assert len(lists(plans, "test_chain")[0]["groups"]) == 9
    for name in ("no_joint_pack", "scoring_not_packed"):
        assert (plans[name][0]["jpack_l"], plans[name][0]["jpack_r"]) == ("0", "0"), name
    assert (plans["short_left_flank"][0]["jpack_l"], plans["short_left_flank"][0]["jpack_r"]) == ("0", "1")
    assert (plans["short_right_flank"][0]["jpack_l"], plans["short_right_flank"][0]["jpack_r"]) == ("1", "0")
    assert lists(plans, "empty_read_and_no_cells")[2]["cells_need_clear"] == "1"
    assert lists(plans, "odd_read_count")[1]["cells_need_clear"] == "0"
    # the errors, and that a batch goes on after one
    assert errors("error_cells_not_grouped") == [0, E_ARG, 0]
    assert errors("error_negative_k") == [E_ARG]
    for name in ("error_window_too_long", "error_template_too_long", "error_too_many_cells"):
        assert errors(name) == [E_RANGE], name
    assert "window" in plans["error_window_too_long"][1][0]["error"] and "template" in plans["error_template_too_long"][1][0]["error"]
    assert "too many cells" in plans["error_too_many_cells"][1][0]["error"]
