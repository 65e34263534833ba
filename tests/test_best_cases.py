"""The facts the GPU cases of tests/test_gpu_best.py rely on (DESIGN.md §4.9 "Tests"), pinned without a
GPU on the shared CPU reference (tests/best_cases.py), so that a changed generator cannot quietly make a
case vacuous: the record is not the last pass (except where the case is built for that), the tie case
has a tie at its minimum, and improving passes are followed by non-improving ones.  The GPU tests
assert the same facts again before they compare."""
import numpy as np
import pytest

import best_cases as bc
from best_cases import counts, improving, record

BEST_FUNCS = ("alll_track_best", "alll_get_best", "alll_group_track_best", "alll_group_get_best",
              "alll_batch_track_best", "alll_batch_get_best")


@pytest.fixture(scope="module", autouse=True)
def tracking_api(native, oracle_mod):
    """The cases are those of the tracking entry points: without them there is nothing to pin."""
    for name in BEST_FUNCS:
        assert hasattr(native.lib(), name), name


def gaps(traj):
    """Non-improving passes between consecutive improving ones."""
    imp = improving(traj)
    return [b - a - 1 for a, b in zip(imp, imp[1:])]


def facts_hold(c, last_is_record=False):
    """What every case needs: the record is not the last pass (or is, where the case says so), and at
    least one non-improving pass lies between two improving ones."""
    traj = c["traj"]
    r = record(traj)
    assert (r["iteration"] == len(traj)) == last_is_record
    assert max(gaps(traj), default=0) >= 1
    return r


def test_trajectory_is_not_the_oracle_trace(oracle_mod):
    """The trajectory holds the assignment a pass evaluated and includes the last pass; the oracle's
    trace rows hold the assignment after the resample and omit it."""
    o, c = oracle_mod, bc.main_case()
    _, _, rows = o.solve(c["n"], c["offs"], c["lits"], c["seed"], max_iters=c["passes"], trace=True)
    assert len(rows) == c["passes"] - 1 and len(c["traj"]) == c["passes"]
    np.testing.assert_array_equal(c["traj"][0][1], o.init_assignment(c["seed"], c["n"]))
    assert not np.array_equal(rows[0][4], c["traj"][0][1])
    for p, row in enumerate(rows, 1):  # pass p's count, and the assignment pass p + 1 evaluates
        assert row[1] == c["traj"][p - 1][0]
        np.testing.assert_array_equal(row[4], c["traj"][p][1])


def test_main_case():
    c = bc.main_case()
    r = facts_hold(c)
    assert (r["n_violated"], r["iteration"]) == (37, 58) and counts(c["traj"])[:8] == [97, 82, 83, 81, 74, 83, 66, 49]
    assert counts(c["traj"])[-1] == 52
    # the three-run split of the GPU test (7, 1, 52) cuts between improving passes and inside a gap
    assert 7 in improving(c["traj"]) and 8 in improving(c["traj"]) and 9 not in improving(c["traj"])


def test_tie_case():
    c = bc.tie_case()
    r = facts_hold(c)
    us = counts(c["traj"])
    assert (r["n_violated"], r["iteration"]) == (8, 10)
    assert [p for p, u in enumerate(us, 1) if u == 8] == [10, 12]  # a tie at the minimum: the first one holds


def test_unit_case(oracle_mod):
    c = bc.unit_case()
    us = counts(c["traj"])
    assert c["n"] == 1 and us[0] == 1 and us[-1] == 0 and 2 <= len(us) <= 64
    r = record(c["traj"])
    assert (r["n_violated"], r["iteration"]) == (0, len(us))  # the solved pass is the record


def test_capped_case():
    c = bc.capped_case()
    traj, cap = c["traj"], c["cap"]
    assert cap == 58 and len(traj) == cap + bc.CAP_RUN
    r = facts_hold(dict(traj=traj[:cap]), last_is_record=True)  # the capped pass is the record
    assert (r["n_violated"], r["iteration"]) == (37, cap)
    # the continuation evaluates the same words again (a tie), then moves on without beating them
    np.testing.assert_array_equal(traj[cap][1], traj[cap - 1][1])
    assert traj[cap][0] == 37 and not np.array_equal(traj[cap + 1][1], traj[cap][1])
    assert record(traj)["iteration"] == cap


def test_blocks_case():
    c = bc.blocks_case()
    r = facts_hold(c)
    assert (r["n_violated"], r["iteration"]) == (1471, 38) and (c["n"] + 31) // 32 > 128  # two resample workgroups


def test_big_case():
    c = bc.big_case()
    r = record(c["traj"])  # (run until the record is not the last pass: the last pass does not improve)
    assert 2 <= r["iteration"] < c["passes"] == len(c["traj"]) <= bc.BIG_MAX_PASSES
    assert c["passes"] not in improving(c["traj"])
    assert all(int(c["thr"][v]) == t for v, t in bc.BIG_MUST)
    assert (c["n"] + 31) // 32 > 4 * 128  # five resample workgroups


def test_rr_and_biased_cases():
    main = bc.main_case()
    for c in (bc.rr_case(), bc.biased_case()):
        facts_hold(c)
        assert counts(c["traj"]) != counts(main["traj"])[:c["passes"]]  # another MIS, another stream
    thr = bc.biased_case()["thr"]
    assert (thr == 0).any() and (thr == bc.PIN1).any()


def test_inject_case():
    c = bc.inject_case()
    traj = c["traj"]
    before = record(traj[:bc.INJECT_WORSE_AT - 1])
    assert traj[bc.INJECT_WORSE_AT - 1][0] > before["n_violated"]  # the assignment set is worse: the record stays
    assert record(traj[:bc.INJECT_BETTER_AT - 1])["iteration"] == before["iteration"]
    assert traj[bc.INJECT_BETTER_AT - 1][0] < before["n_violated"]  # the assignment set is better: it is the record
    r = facts_hold(c)
    assert r["iteration"] == bc.INJECT_BETTER_AT
    np.testing.assert_array_equal(r["words"], c["better"])


def test_group_case():
    g = bc.group_case()
    cap, solved_at = g["cap"], g["solved_at"]
    assert solved_at == 38 and len(g["trajs"][4]) == solved_at < cap  # one item ends early, the others go on
    assert [t is not None for t in g["thrs"]] == [False, True, True, False, False]
    assert [n for n, _, _ in g["items"]] == [1500, 5003, 33, 4097, 200]
    for tr in g["trajs"][:4]:
        assert len(tr) == cap + bc.GROUP_MORE
        facts_hold(dict(traj=tr[:cap]))
        np.testing.assert_array_equal(tr[cap][1], tr[cap - 1][1])  # (the capped pass did not resample)
    # the later run beats the record of one item and leaves the others
    assert [record(tr)["iteration"] > cap for tr in g["trajs"]] == [False, True, False, False, False]


def test_batch_case():
    b = bc.batch_case()
    assert [len(tr) for tr in b["trajs"]] == [b["cap"]] * 4 + [38]
    for tr in b["trajs"][:4]:
        facts_hold(dict(traj=tr))
    assert len({record(tr)["iteration"] for tr in b["trajs"]}) == 5  # every item has a record of its own
