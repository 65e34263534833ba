"""Block-diagonal groups (GroupSolver, alll_group_*) on the GPU: items of any size advanced together
by the one-instance loop.  Every item's trajectory is fully determined by (instance, seed), so each
is compared bit for bit with the oracle (CPU restatement of the serial path) run on the item alone
at the item's seed, and with the one-instance path (Solver)."""
import functools

import numpy as np
import pytest

from group_cases import mixed_bag, oracle_step
from lfmis_structures import all_false, chain
from test_gpu_parity import LAYOUTS

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
NO_GRAPH = 1 << 0


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def oracle_stats(st_o):
    d = {k: st_o[k] for k in STAT_KEYS if k != "n_violated"}
    d["n_violated"] = st_o["last_violated"]
    return d


def check_item(g, i, res, st_o, A_o, native, what):
    assert {k: res[k] for k in STAT_KEYS} == oracle_stats(st_o), (what, i)
    if "status" in res:
        assert res["status"] == (native.ALLL_OK if st_o["solved"] else native.ALLL_ERR_MAX_ITERS), (what, i)
    assert res["n_gpus"] == 1 and res["gpu_resamples"] == [st_o["n_resamples"]], (what, i)
    np.testing.assert_array_equal(g.assignment_words(i), A_o, err_msg=f"{what} item {i}")


class Trace:
    """The oracle's run of one item: the state after every run(1) of a group that holds it."""

    def __init__(self, o, item, seed, max_iters, A0=None):
        n, offs, lits = item
        self.A0 = o.init_assignment(seed, n) if A0 is None else A0
        self.st, self.A, self.rows = o.solve(n, offs, lits, seed, max_iters=max_iters, A0=A0, trace=True)

    def after(self, steps):
        """(n_iterations, n_violated of the last pass, sum |MIS|, resamples, solved, assignment) after
        `steps` iterations of a run that is not capped before them."""
        done = self.rows[:steps]
        ended = steps > len(self.rows)  # the pass after the last resample found nothing (or the cap)
        assert not ended or self.st["solved"], "the oracle run was capped before these steps"
        return dict(n_iterations=self.st["n_iterations"] if ended else steps,
                    n_violated=0 if ended else done[-1][1],
                    sum_mis_size=sum(r[2] for r in done), n_resamples=sum(r[3] for r in done),
                    solved=1 if ended else 0), (done[-1][4] if done else self.A0)


def check_steps(g, traces, steps, what):
    res = [g.stats(i) for i in range(len(traces))]
    for i, t in enumerate(traces):
        want, A = t.after(steps)
        assert {k: res[i][k] for k in want} == want, (what, i, steps)
        np.testing.assert_array_equal(g.assignment_words(i), A, err_msg=f"{what} item {i} after {steps} iterations")


@functools.lru_cache(maxsize=None)
def bag():
    import oracle as o

    items, seeds = mixed_bag()
    traces = [Trace(o, it, s, 40) for it, s in zip(items, seeds)]
    return items, seeds, traces


def test_mixed_bag(gpu, native, oracle_mod):
    """1. Items past the batch's limits, tiny ones, a clause-less one, mixed widths and shared arrays
    in one group: six single steps against the oracle's traces, then a capped solve."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    items, seeds, traces = bag()
    assert not native.lib().alll_batch_fits(items[0][0], 10000, 30000)   # past the batch's clause limit
    assert not native.lib().alll_batch_fits(9000, 9000, 27000)           # past its variable limit
    assert traces[0].st["solved"] == 0 and traces[1].st["solved"] == 1 and traces[3].st["n_iterations"] == 1
    with GroupSolver(items, seeds) as g:
        assert g.layout() == 0  # mixed widths: the union is ragged
        for i, t in enumerate(traces):
            np.testing.assert_array_equal(g.assignment_words(i), t.A0, err_msg=f"initial assignment, item {i}")
        for step in range(1, 7):
            g.run(1)
            check_steps(g, traces, step, "run(1)")
    with GroupSolver(items, seeds, max_iters=40) as g:
        res = g.solve()
        for i, t in enumerate(traces):
            check_item(g, i, res[i], t.st, t.A, native, "solve")
        assert res[3]["n_iterations"] == 1 and res[3]["solved"] == 1
        assert res[0]["status"] == native.ALLL_ERR_MAX_ITERS and res[0]["n_iterations"] == 40
        # a second solve changes nothing: solved items are final, capped ones stay at the cap
        again = g.solve()
        assert [{k: r[k] for k in STAT_KEYS} for r in again] == [{k: r[k] for k in STAT_KEYS} for r in res]


BOUNDARY_M = (4097, 8191, 100, 4096, 12345)  # item ends one past, one short of and on tile boundaries
BOUNDARY_N = (1025, 2047, 27, 1023, 3087)    # no multiple of 32


@functools.lru_cache(maxsize=None)
def boundary():
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    items = [(n, *generate_ksat(7 + i, n, m, 3)) for i, (n, m) in enumerate(zip(BOUNDARY_N, BOUNDARY_M))]
    seeds = [21, 22, 23, 24, 25]
    return items, seeds, [Trace(o, it, s, 9) for it, s in zip(items, seeds)]


VARIANTS = ["hybrid", "csr", "fixed", "atomic_claims", "no_graph", "buckets", "bscatter", "tail_all", "no_small_u",
            "positions", "windows"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_fixed_width_union_with_item_boundaries_everywhere(gpu, oracle_mod, variant, monkeypatch):
    """2. Five 3-SAT items whose ends fall around the 4096-clause tiles, under every layout flag a
    group honours and the knobs that force the bucketed and the small-set LFMIS variants: eight
    iterations against the oracle, and against a Solver per item under the same variant."""
    from alllsatisfiabilitysolver_amd import GroupSolver, Solver

    items, seeds, traces = boundary()
    flags, env = (NO_GRAPH, {}) if variant == "no_graph" else LAYOUTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with GroupSolver(items, seeds, flags=flags) as g:
        assert g.layout() == (0 if variant == "csr" else 3)
        assert g.eval_kernel() == {"csr": "k_eval_csr", "fixed": "k_eval_fixed<3>"}.get(variant, "k_eval_hybrid<3>")
        for step in range(1, 9):
            g.run(1)
            check_steps(g, traces, step, variant)
        res = [g.stats(i) for i in range(len(items))]
        for i, ((n, offs, lits), s) in enumerate(zip(items, seeds)):
            with Solver(n, offs, lits, seed=s, flags=flags) as one:
                one.run(8)
                st = one.stats()
                assert {k: res[i][k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (variant, i)
                np.testing.assert_array_equal(g.assignment_words(i), one.assignment_words())


def test_the_capped_pass(gpu, native, oracle_mod):
    """3. max_iters is the pass at which item one has its first clean pass: that pass is counted and
    item one is solved (the zero check comes before the cap check), although the capped pass runs no
    MIS for anybody; item two is capped with its own violated count."""
    from alllsatisfiabilitysolver_amd import GroupSolver, generate_ksat

    o = oracle_mod
    one = (500, *generate_ksat(31, 500, 1000, 3))
    two = (300, *generate_ksat(32, 300, 1290, 3))
    st1, A1, _ = o.solve(*one, 41, max_iters=5000)
    cap = st1["n_iterations"]
    assert st1["solved"] == 1 and cap >= 3
    st2, A2, _ = o.solve(*two, 42, max_iters=cap)
    assert st2["solved"] == 0 and st2["last_violated"] > 0  # the oracle really has item two unsolved there
    assert o.solve(*one, 41, max_iters=cap)[0] == st1       # ... and item one solved by the capped pass itself
    with GroupSolver([one, two], [41, 42], max_iters=cap) as g:
        res = g.solve()
        check_item(g, 0, res[0], st1, A1, native, "capped pass")
        check_item(g, 1, res[1], st2, A2, native, "capped pass")
        assert (res[0]["status"], res[0]["solved"], res[0]["n_iterations"]) == (native.ALLL_OK, 1, cap)
        assert (res[1]["status"], res[1]["solved"], res[1]["n_iterations"]) == (native.ALLL_ERR_MAX_ITERS, 0, cap)
        assert res[1]["n_violated"] == st2["last_violated"]


def test_one_item_is_a_solver(gpu, oracle_mod):
    """4. A group of one item and Solver(seed): ten iterations, every statistic and the assignment."""
    from alllsatisfiabilitysolver_amd import GroupSolver, Solver, generate_ksat

    n, m = 3001, 12000
    offs, lits = generate_ksat(5, n, m, 3)
    with GroupSolver([(n, offs, lits)], [77]) as g, Solver(n, offs, lits, seed=77) as s:
        np.testing.assert_array_equal(g.assignment_words(0), s.assignment_words())
        for steps in (3, 7):
            a = g.run(steps)[0]
            s.run(steps)
            b = s.stats()
            assert a == b  # (one item: the union's LFMIS rounds are the item's)
            np.testing.assert_array_equal(g.assignment_words(0), s.assignment_words())
        assert a["n_iterations"] == 10 and a["solved"] == 0


@pytest.mark.parametrize("m", [513, 1025])
def test_deep_item_beside_a_shallow_one(gpu, oracle_mod, m):
    """5. chain(m) from all-false needs (m + 1) / 2 dependent LFMIS rounds (claim_rounds,
    tests/test_lfmis_structures.py: 257 for chain(513), 513 for chain(1025)); a random 3-SAT item
    beside it settles in a handful.  Both trajectories are the oracle's, and the rounds the group
    reports are the union's."""
    from alllsatisfiabilitysolver_amd import GroupSolver, generate_ksat

    o = oracle_mod
    deep = chain(m)
    flat = (2000, *generate_ksat(9, 2000, 8000, 3))
    A0 = all_false(deep[0])
    traces = [Trace(o, deep, 51, 5, A0=A0), Trace(o, flat, 52, 5)]
    assert traces[0].rows[0][1:3] == (m, (m + 1) // 2)  # everything violated, every second clause in the MIS
    with GroupSolver([deep, flat], [51, 52]) as g:
        g.set_assignment_words(0, A0)
        for step in range(1, 5):
            g.run(1)
            check_steps(g, traces, step, f"chain({m})")
        rounds = g.stats(1)["lfmis_rounds_max"]
        assert rounds == g.stats(0)["lfmis_rounds_max"] and rounds >= (m + 1) // 2
        if m == 1025:
            assert rounds >= 513


PORTFOLIO_CAP = 5000  # (never reached: the assertion below has every seed solved long before)


@functools.lru_cache(maxsize=None)
def portfolio():
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    n, m = 1000, 2000
    offs, lits = generate_ksat(17, n, m, 3)
    seeds = list(range(101, 117))
    return (n, offs, lits), seeds, [o.solve(n, offs, lits, s, max_iters=PORTFOLIO_CAP) for s in seeds]


def test_portfolio_first_solved(gpu, native, oracle_mod):
    """6. Sixteen seeds of one instance: first_solved returns with the oracle's winner solved (the
    fewest iterations, the lowest index on a tie); a plain solve() then finishes every item exactly
    as a fresh full solve would."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    item, seeds, want = portfolio()
    iters = [st["n_iterations"] for st, _, _ in want]
    assert all(st["solved"] for st, _, _ in want) and len(set(iters)) >= 2
    winner = min(range(16), key=lambda i: (iters[i], i))
    with GroupSolver([item] * 16, seeds, max_iters=PORTFOLIO_CAP) as g:
        res = g.solve(first_solved=True)
        solved = [i for i, r in enumerate(res) if r["solved"]]
        assert solved and min(solved, key=lambda i: (res[i]["n_iterations"], i)) == winner
        check_item(g, winner, res[winner], want[winner][0], want[winner][1], native, "winner")
        for i, r in enumerate(res):  # everybody is on their own trajectory: solved at their own pass or still short of it
            assert r["n_iterations"] == iters[i] if r["solved"] else r["n_iterations"] < iters[i]
        again = g.solve(first_solved=True)  # an item is solved already: nothing runs
        assert [r["n_iterations"] for r in again] == [r["n_iterations"] for r in res]
        res = g.solve()
        for i, (st_o, A_o, _) in enumerate(want):
            check_item(g, i, res[i], st_o, A_o, native, "after first_solved")


def test_set_assignment_words(gpu, native, oracle_mod):
    """7. After three iterations one item gets a new assignment: it follows the oracle from that
    assignment at resample round 3, the other items go on undisturbed.  A solved item is final."""
    from alllsatisfiabilitysolver_amd import AlllError, GroupSolver, generate_ksat

    o = oracle_mod
    items = [(777, *generate_ksat(41, 777, 3100, 3)), (1501, *generate_ksat(42, 1501, 6000, 3)),
             (333, *generate_ksat(43, 333, 1400, 3)), (10, np.zeros(1, np.uint64), np.zeros(0, np.uint32))]
    seeds = [61, 62, 63, 64]
    traces = [Trace(o, it, s, 8) for it, s in zip(items, seeds)]
    n, offs, lits = items[1]
    W = o.init_assignment(999, n)
    with GroupSolver(items, seeds) as g:
        g.run(3)
        check_steps(g, traces, 3, "before")
        before = g.stats(1)
        g.set_assignment_words(1, W)
        np.testing.assert_array_equal(g.assignment_words(1), W)
        A, sum_mis, n_res = W, before["sum_mis_size"], before["n_resamples"]
        for it in range(3, 6):
            U, M, A = oracle_step(o, n, offs, lits, A, 62, it)
            assert U.size > 0
            sum_mis += M.size
            n_res += int((offs[M.astype(np.int64) + 1] - offs[M.astype(np.int64)]).sum())
            g.run(1)
            st = g.stats(1)
            assert (st["n_iterations"], st["n_violated"], st["sum_mis_size"], st["n_resamples"]) == (
                it + 1, U.size, sum_mis, n_res), it
            np.testing.assert_array_equal(g.assignment_words(1), A, err_msg=f"item 1 after round {it}")
            for i in (0, 2, 3):
                want, Ai = traces[i].after(it + 1)
                got = g.stats(i)
                assert {k: got[k] for k in want} == want, (i, it)
                np.testing.assert_array_equal(g.assignment_words(i), Ai)
        with pytest.raises(AlllError) as ei:  # item 3 (no clause) was solved by the first pass
            g.set_assignment_words(3, np.zeros(1, np.uint32))
        assert ei.value.code == native.ALLL_ERR_INVALID_ARG
