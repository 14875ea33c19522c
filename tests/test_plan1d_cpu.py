"""The plan of a 1D batch (nra_plan1d.cpp: candidates, buckets, tasks, launch groups, ticket lists, the clears rule) is
pinned, bit for bit, to the plan the create function made before the plan was split from its upload:
tests/golden/plan1d.json holds, per case of tests/plan1d_cases.py, the digest text nra_plan1d_digest gives (scalars, one
line per bucket, length and FNV-1a hash per array) or the error code and text, recorded from that earlier commit with the
same digest writer patched into its create function.  No device is needed.

One branch stays uncovered: a second launch group of k_sweep_ringmt needs more strips than NRA_CHAIN_SCRATCH_BUDGET / 2
holds, which no small input reaches.

Two cases do not do what their names promise, in the golden as in the code: a read of 1550 - 1600 bases lies above
NRA_RING_MT_FROM and is chained on its own (`stragglers_1500` is the case where the straggler rule moves reads), and a
template longer than NRA_MAX_TLEN sends a short read to the packed chain bucket, not the int32 one
(`wide_by_template`)."""
import json
import os

import pytest

import plan1d_cases as P

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan1d.json")))
Q_WHOLE = 1 << 30        # NRA_Q_WHOLE


def test_the_golden_holds_every_case():
    assert sorted(GOLDEN) == sorted(P.cases())


@pytest.mark.parametrize("name", sorted(P.cases()))
def test_plan_is_the_recorded_plan(capi, monkeypatch, name):
    c = P.cases()[name]
    for k in P.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    assert P.digest(c) == GOLDEN[name]


def plans():
    """name -> (scalars, buckets) of every golden plan that is no error."""
    out = {}
    for name, text in GOLDEN.items():
        if isinstance(text, list):
            continue
        scalars, buckets = {}, []
        for line in text.splitlines():
            key, _, value = line.partition(" ")
            if key.startswith("bucket"):
                b = dict(kv.split("=") for kv in value.split())
                buckets.append({k: v if k == "mt_groups" else int(v) for k, v in b.items()})
            else:
                scalars[key] = value
        assert int(scalars["n_buckets"]) == len(buckets)
        out[name] = (scalars, buckets)
    return out


def test_the_golden_covers_every_bucket_form():
    p = plans()
    buckets = [b for _, bs in p.values() for b in bs]

    def some(f):
        return any(f(b) for b in buckets)

    assert some(lambda b: b["half"])
    assert some(lambda b: b["ring"] and not b["half"] and not b["chain"])
    assert some(lambda b: b["chain"] and b["mt"])
    assert some(lambda b: b["chain"] and not b["mt"])
    assert some(lambda b: b["wide"])
    assert some(lambda b: not b["ring"])
    assert some(lambda b: b["quanta"]) and some(lambda b: not b["quanta"])
    assert some(lambda b: b["taint"]) and some(lambda b: not b["taint"])
    assert some(lambda b: b["n_pair"] > 0)
    assert some(lambda b: b["n_queue"] > 0)
    # parts of fewer steps than a whole sweep, and more than one part in both directions: 131 reverse steps (a right
    # flank of 100 bases in a half-wave bucket) in parts of 64
    assert some(lambda b: b["quanta"] and b["q_steps"] < Q_WHOLE and b["n_quanta"] > 2 * b["n_sweep"])
    q64 = p["quanta_qsteps64"][1][0]
    assert q64["q_steps"] == 64 and q64["n_quanta"] >= (3 + 2) * q64["n_sweep"]


def test_the_golden_shows_what_each_case_is_for():
    p = plans()
    errors = {n: v for n, v in GOLDEN.items() if isinstance(v, list)}
    assert sorted(errors) == ["error_brute_long_read", "error_kmin_negative", "error_template_too_long", "error_test_chain_brute"]
    assert errors["error_kmin_negative"][1] == -1 and all(errors[n][1] == -3 for n in errors if n != "error_kmin_negative")
    # the fitted model: row blocks on 1024 SIMDs, one register block on 16
    assert all(b["chain"] and b["mt"] for b in p["mid_simds1024"][1])
    assert not any(b["chain"] for b in p["mid_simds16"][1])
    # folding: the reads of 100 - 700 bases end in fewer buckets than their lengths span
    assert len(p["short_no_half_wave"][1]) == 1 and p["short_no_half_wave"][1][0]["R"] == 11
    # the straggler rule: no one-block bucket is left
    assert [b["chain"] for b in p["stragglers_1500"][1]] == [1]
    # the chosen block height
    assert p["long"][1][0]["R"] == 14 and p["long_serial_chain"][1][0]["R"] == 20
    assert p["wide_by_score"][1][0]["wide"] == 1
    for name in ("short_brute_force", "short_all_extents", "no_left_flank", "scoring_brute"):
        assert p[name][0]["brute"] == "1", name
    assert p["scoring_no_taint"][0]["brute"] == "0" and p["scoring_no_taint"][0]["relax_c"] == "0"
    assert p["short"][0]["sweeps_write_all"] == "1" and p["skipped_and_empty"][0]["sweeps_write_all"] == "0"
    assert p["short_tie_extents"][0]["sweeps_write_all"] == "0"
    assert p["quanta_parts"][1][0]["q_steps"] == 384 and not p["quanta_too_many"][1][0]["quanta"]
    assert p["short"][1][0]["q_steps"] == Q_WHOLE
