"""Unit propagation of the pinned variables past one workgroup of items and at the batch's limits
(DESIGN.md §4.10): the group form (k_prop_pack / k_prop_scan / k_prop_apply over a union of 130, 199
and 1000 items that end in different rounds, prop_drive's records) and the batch form
(k_small_propagate on 130 and 1000 workgroups and on an item of 8192 variables, 8192 clauses and
24576 literals).  Every comparison is an equality with prop_cases.propagate, the numpy restatement of
the rules, per item in the item's own numbering: status, rounds, n_forced, conflict_clause, every
threshold and every assignment word (the host's biased fill of the propagated thresholds, which
tests/test_prop_cases.py shows equal to the oracle's), then three iterations against the oracle under
the propagated thresholds.  The facts the cases are there for are pinned on the CPU in
tests/test_prop_cases.py."""
import numpy as np
import pytest

import prop_cases as P
import swarm_cases as sc
from test_gpu_prop import GENERIC_CSR, STAT_KEYS, fill_words, own_solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def same(got, want, what):
    if not np.array_equal(got, want):
        np.testing.assert_array_equal(got, want, err_msg=what)


def load(s, c):
    for i, thr in enumerate(c["thrs"]):
        if thr is not None:
            s.set_thresholds(i, thr)
    return s


def check_results(res, want, what):
    assert len(res) == len(want)
    bad = [(i, r, w) for i, (r, w) in enumerate(zip(res, want)) if r != w]
    assert not bad, (what, len(bad), bad[:5])


def check_state(native, o, s, c, outs, what):
    """Every item's thresholds and words: those of the reference's thresholds `outs` under the host's
    fill and the oracle's; an item without thresholds has none to read and its unbiased fill."""
    from alllsatisfiabilitysolver_amd import AlllError

    for i, ((n, _, _), seed, out) in enumerate(zip(c["items"], c["seeds"], outs)):
        words = s.assignment_words(i)
        if out is None:
            with pytest.raises(AlllError) as ei:
                s.thresholds(i)
            assert ei.value.code == native.ALLL_ERR_INVALID_ARG, (what, i)
            same(words, o.init_assignment(seed, n), f"{what}: unbiased fill of item {i}")
        else:
            same(s.thresholds(i), out, f"{what}: thresholds of item {i}")
            same(words, fill_words(seed, n, out), f"{what}: words of item {i}")


def check_run(s, c, refs, what, skip_conflicts=False):
    """RUN_STEPS iterations of every item against the oracle's run under the propagated thresholds
    (an item without thresholds: its unbiased run)."""
    stats = s.run(P.RUN_STEPS)
    for i, ref in enumerate(refs):
        if skip_conflicts and c["ress"][i]["status"] == P.CONFLICT:
            continue
        want, A = sc.rows_after(*ref, P.RUN_STEPS)
        assert {k: stats[i][k] for k in want} == want, (what, i)
        same(s.assignment_words(i), A, f"{what}: words of item {i} after run({P.RUN_STEPS})")


def check_uncapped(native, o, s, c, refs, what, skip_conflicts=False):
    """The checks of (a): the first call, a second one that finds nothing more, the iterations."""
    res = s.propagate_pins()
    check_results(res, c["ress"], what)
    check_state(native, o, s, c, c["outs"], what)
    check_results(s.propagate_pins(), [dict(r, rounds=0, n_forced=0) for r in c["ress"]], f"{what}, second call")
    check_state(native, o, s, c, c["outs"], f"{what}, second call")
    check_run(s, c, refs, what, skip_conflicts)


def problems(c):
    return list(c["items"]), list(c["seeds"])


# ----------------------------------------------------------------------------- a. ladder
def test_ladder_group(gpu, native, oracle_mod):
    """a. 130 items of 1 to 5 words in one group, item j ending after j rounds: every wave of words holds
    a dozen or more items that end in different rounds, 17 of them in a conflict beside neighbours that
    apply, 21 without thresholds whose unit and empty clauses every scan finds, 12 without a clause."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = P.ladder()
    with load(GroupSolver(*problems(c)), c) as g:
        check_uncapped(native, oracle_mod, g, c, P.ladder_references(), "ladder")


# ----------------------------------------------------------------------------- b. ladder, capped
@pytest.mark.parametrize("cap", P.LADDER_CAPS)
def test_ladder_group_capped(gpu, native, oracle_mod, cap):
    """b. max_rounds = 1, 10 and 129: an item with exactly max_rounds applying rounds is a fixpoint, its
    neighbour with one more is capped; a call without a cap then makes the remaining rounds."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c, full = P.ladder(P.N_LADDER, cap), P.ladder()
    with load(GroupSolver(*problems(c)), c) as g:
        res = g.propagate_pins(cap)
        check_results(res, c["ress"], f"ladder, max_rounds {cap}")
        if cap == 10:
            assert res[10] == dict(status=P.FIXPOINT, rounds=10, n_forced=10, conflict_clause=10)
            assert res[11] == dict(status=P.ROUND_CAP, rounds=10, n_forced=10, conflict_clause=11)
        if cap == 129:
            assert res[129]["status"] == P.FIXPOINT and res[129]["rounds"] == 129
        check_state(native, oracle_mod, g, c, c["outs"], f"ladder, max_rounds {cap}")
        check_results(g.propagate_pins(0), P.continued(full, c), f"ladder, continued after {cap}")
        check_state(native, oracle_mod, g, full, full["outs"], f"ladder, continued after {cap}")


# ----------------------------------------------------------------------------- c. prop swarm
@pytest.mark.parametrize("flags", [0, GENERIC_CSR], ids=["default", "generic_csr"])
def test_prop_swarm_group(gpu, native, oracle_mod, flags):
    """c. The thousand items of the ragged swarm, 669 with thresholds: conflicts at round 0 and later
    (conflict_clause in the item's numbering, three of them at a clause base that a run of clauseless
    items shares), fixpoints after 0 to 4 rounds, unbiased items with one-literal and empty clauses, and
    32 one-word items per word of the per-word bits.  The group honours ALLL_FLAG_GENERIC_CSR."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = P.prop_swarm()
    with load(GroupSolver(*problems(c), flags=flags), c) as g:
        assert g.layout() == 0
        check_uncapped(native, oracle_mod, g, c, P.prop_swarm_references(), "prop swarm")


def test_prop_swarm_group_capped(gpu, native, oracle_mod):
    """c. max_rounds = 1 on the swarm: 27 items are capped while their neighbours have just ended."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c, full = P.prop_swarm(1), P.prop_swarm()
    assert sum(1 for r in c["ress"] if r["status"] == P.ROUND_CAP) == 27
    with load(GroupSolver(*problems(c)), c) as g:
        check_results(g.propagate_pins(1), c["ress"], "prop swarm, max_rounds 1")
        check_state(native, oracle_mod, g, c, c["outs"], "prop swarm, max_rounds 1")
        check_results(g.propagate_pins(0), P.continued(full, c), "prop swarm, continued")
        check_state(native, oracle_mod, g, full, full["outs"], "prop swarm, continued")


# ----------------------------------------------------------------------------- d. mixed group
def test_mixed_group(gpu, native, oracle_mod):
    """d. Both counting branches of k_prop_apply in one call: a first wave of 64 distinct one-word
    items, the ladder, B1, B2, C', a chain of 4099 variables that holds a whole wave, and a star whose
    hub is hot in the union (bit 31 of its literals) at a variable index past 15000."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = P.mixed_group()
    with load(GroupSolver(*problems(c)), c) as g:
        check_uncapped(native, oracle_mod, g, c, P.mixed_group_references(), "mixed group")


# ----------------------------------------------------------------------------- e. batch
@pytest.mark.parametrize("name", ["ladder", "prop_swarm"])
def test_batch_equals_group(gpu, native, oracle_mod, name):
    """e. The ladder and the prop swarm in a BatchSolver: 130 and 1000 workgroups of k_small_propagate,
    each ending in its own round of the one launch; the results, thresholds and words are the
    reference's and, item for item, those of a GroupSolver; then run(3) of the items not in conflict."""
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver

    c, refs = (P.ladder(), P.ladder_references()) if name == "ladder" else (P.prop_swarm(), P.prop_swarm_references())
    with load(BatchSolver(*problems(c)), c) as b, load(GroupSolver(*problems(c)), c) as g:
        res_b, res_g = b.propagate_pins(), g.propagate_pins()
        check_results(res_b, c["ress"], f"{name} batch")
        assert res_b == res_g
        check_state(native, oracle_mod, b, c, c["outs"], f"{name} batch")
        for i, out in enumerate(c["outs"]):
            if out is not None:
                same(b.thresholds(i), g.thresholds(i), f"{name}: batch and group thresholds of item {i}")
            same(b.assignment_words(i), g.assignment_words(i), f"{name}: batch and group words of item {i}")
        check_results(b.propagate_pins(), [dict(r, rounds=0, n_forced=0) for r in c["ress"]], f"{name} batch, second call")
        check_state(native, oracle_mod, b, c, c["outs"], f"{name} batch, second call")
        check_run(b, c, refs, f"{name} batch", skip_conflicts=True)


def test_ladder_batch_capped(gpu, native, oracle_mod):
    """e. max_rounds = 10 inside the kernel: item 10 a fixpoint, item 11 capped; then the remainder."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    c, full = P.ladder(P.N_LADDER, 10), P.ladder()
    with load(BatchSolver(*problems(c)), c) as b:
        res = b.propagate_pins(10)
        check_results(res, c["ress"], "ladder batch, max_rounds 10")
        assert res[10] == dict(status=P.FIXPOINT, rounds=10, n_forced=10, conflict_clause=10)
        assert res[11] == dict(status=P.ROUND_CAP, rounds=10, n_forced=10, conflict_clause=11)
        check_state(native, oracle_mod, b, c, c["outs"], "ladder batch, max_rounds 10")
        check_results(b.propagate_pins(0), P.continued(full, c), "ladder batch, continued")
        check_state(native, oracle_mod, b, full, full["outs"], "ladder batch, continued")


# ----------------------------------------------------------------------------- f. the limits
def test_limit_item_batch(gpu, native, oracle_mod):
    """f. An item of 8192 variables, 8192 clauses and 24576 literals -- word 255 of the LDS bitmaps,
    variable 8191, literals 16382 and 16383 of the 16-bit pool -- four times over the same arrays (one
    problem copy on the device) under four cubes, beside a one-variable item and an item without
    thresholds.  Every item against the reference, the first also against a Solver of its own: the
    result, the thresholds, the words at iteration 0 and after run(3)."""
    import bias_cases
    from alllsatisfiabilitysolver_amd import BatchSolver

    n, offs, lits = P.limit_instance()
    cubes = [P.limit_item(cs) for cs in range(len(P.LIMIT_CUBES))]
    one_offs, one_lits = P.csr([[P.pos(0)]])
    bn, boffs, blits = P.b_instance()
    items = [(n, offs, lits)] * len(cubes) + [(1, one_offs, one_lits), (bn, boffs, blits)]
    thrs = [c["thr"] for c in cubes] + [np.full(1, P.FAIR, np.uint32), None]
    c = P.many(items, [sc.swarm_seed(6000 + i) for i in range(len(items))], thrs)
    assert [r["status"] for r in c["ress"]] == [P.FIXPOINT, P.FIXPOINT, P.CONFLICT, P.FIXPOINT, P.FIXPOINT, P.NONE]
    assert c["ress"][4] == dict(status=P.FIXPOINT, rounds=1, n_forced=1, conflict_clause=1)
    assert len({(r["rounds"], r["n_forced"]) for r in c["ress"][:4]}) == 4  # (the cubes differ in what they force)
    refs = [None if c["ress"][i]["status"] == P.CONFLICT else
            (bias_cases.unbiased_reference(oracle_mod, *it, s, P.RUN_STEPS) if out is None else
             bias_cases.reference(oracle_mod, *it, s, out, P.RUN_STEPS))
            for i, (it, s, out) in enumerate(zip(c["items"], c["seeds"], c["outs"]))]
    with load(BatchSolver(*problems(c)), c) as b, own_solver(cubes[0], c["seeds"][0]) as s:
        assert s.layout() == 3
        res = b.propagate_pins()
        check_results(res, c["ress"], "limit batch")
        assert s.propagate_pins() == res[0]
        check_state(native, oracle_mod, b, c, c["outs"], "limit batch")
        same(b.thresholds(0), s.thresholds(), "limit item: batch and Solver thresholds")
        same(b.assignment_words(0), s.assignment_words(), "limit item: batch and Solver words")
        assert b.thresholds(0)[8191] == P.PIN1 and (int(b.assignment_words(0)[255]) >> 31) & 1
        stats, want = b.run(P.RUN_STEPS), s.run(P.RUN_STEPS)
        assert {k: stats[0][k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}
        same(b.assignment_words(0), s.assignment_words(), f"limit item: batch and Solver words after run({P.RUN_STEPS})")
        for i, ref in enumerate(refs):
            if ref is not None:
                ref_stats, A = sc.rows_after(*ref, P.RUN_STEPS)
                assert {k: stats[i][k] for k in ref_stats} == ref_stats, i
                same(b.assignment_words(i), A, f"limit batch: words of item {i} after run({P.RUN_STEPS})")
