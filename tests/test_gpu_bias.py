"""Per-variable resample probabilities and pinned variables on the GPU (DESIGN.md §4.8;
alll_set_var_thresholds, alll_group_set_var_thresholds): k_init_biased, k_resample_biased and
k_group_resample_biased against bias_cases.py, which composes the oracle's own primitives (its
Philox, evaluation, LFMIS and round robin) into the biased stream and one iteration under it."""
import ctypes
import functools

import numpy as np
import pytest

from bias_cases import PIN1, follow, mixed_thresholds, reference

pytestmark = pytest.mark.gpu

NO_GRAPH, GENERIC_CSR, NO_RANGED, ATOMIC_CLAIMS, REFERENCE_RNG = 1 << 0, 1 << 2, 1 << 3, 1 << 5, 1 << 7
STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
HALF = 1 << 31


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


SPECIAL = [(31, 0), (32, PIN1), (63, PIN1), (64, 0), (202, 0x40000000), (30, 0xC0000000), (33, 1), (62, 0xFFFFFFFE)]


@functools.lru_cache(maxsize=None)
def trajectory_case():
    """n = 203 (no multiple of 4, 16 or 32), m = 800, k = 3; ~10 % of the variables pinned each way,
    pins and biases on both sides of the word boundaries and on the last variable."""
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    n, m, seed = 203, 800, 5
    offs, lits = generate_ksat(3, n, m, 3)
    thr = mixed_thresholds(n, 1, must=SPECIAL)
    A0, rows = reference(o, n, offs, lits, seed, thr, 12)
    return n, offs, lits, seed, thr, A0, rows


@pytest.mark.parametrize("flags", [0, GENERIC_CSR, NO_RANGED, ATOMIC_CLAIMS, NO_GRAPH])
def test_trajectory(gpu, oracle_mod, flags):
    """1. Twelve single iterations under every layout flag and with eager launches."""
    from alllsatisfiabilitysolver_amd import Solver

    n, offs, lits, seed, thr, A0, rows = trajectory_case()
    assert len(rows) == 12 and rows[-1][1] > 0  # unsolved within the twelve iterations
    assert (thr == 0).sum() >= 10 and (thr == PIN1).sum() >= 10
    with Solver(n, offs, lits, seed=seed, flags=flags) as s:
        s.set_thresholds(thr)
        follow(s, A0, rows, f"flags {flags}")
        a = s.assignment()
        assert (a[thr == PIN1] == 1).all() and (a[thr == 0] == 0).all()


def edge_33():
    from alllsatisfiabilitysolver_amd import generate_ksat

    return (33, *generate_ksat(3, 33, 20, 2)), 13, mixed_thresholds(33, 2, must=[(31, PIN1), (32, 0x30000000), (0, 0)])


def edge_1():
    # the one-literal clause (x0); seed 5: the fill and the first resample draw 0, the second 1
    return (1, np.array([0, 1], np.uint64), np.array([0], np.uint32)), 5, np.array([0x50000000], np.uint32)


def edge_mixed():
    from alllsatisfiabilitysolver_amd import generate_mixed

    return (300, *generate_mixed(5, 300, 700, 1, 5)), 15, mixed_thresholds(300, 3, must=SPECIAL)


@pytest.mark.parametrize("case", [edge_33, edge_1, edge_mixed])
def test_edge_sizes(gpu, oracle_mod, case):
    """2. n = 33 (one variable in the last word), n = 1, and mixed widths 1-5 with repeated variables
    (the ragged layout): eight iterations, or until solved."""
    from alllsatisfiabilitysolver_amd import Solver

    (n, offs, lits), seed, thr = case()
    A0, rows = reference(oracle_mod, n, offs, lits, seed, thr, 8)
    assert rows[0][1] > 0  # something is violated at the start: a resample is compared
    with Solver(n, offs, lits, seed=seed, probabilities=None) as s:
        s.set_thresholds(thr)
        follow(s, A0, rows, case.__name__)


def test_round_robin(gpu, oracle_mod):
    """3. n_threads = 4: the resample after the round-robin MIS (fixpoint passes) is the biased one."""
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, seed = 200, 800, 7
    offs, lits = generate_ksat(4, n, m, 3)
    thr = mixed_thresholds(n, 4, must=SPECIAL)
    A0, rows = reference(oracle_mod, n, offs, lits, seed, thr, 8, T=4)
    assert len(rows) == 8 and rows[-1][1] > 0
    with Solver(n, offs, lits, seed=seed, n_threads=4) as s:
        s.set_thresholds(thr)
        follow(s, A0, rows, "T = 4")


PIN_CASE = (2000, 4000, 21, 9)  # n, m, generator seed, solver seed (biased_step alone solves it within the cap)
PIN_CAP = 2000


def test_pins_hold_and_the_loop_solves(gpu, native, oracle_mod):
    """4. Every second variable pinned to a known solution, the rest fair: the solve ends solved within
    the cap with every pin in place; with every variable pinned to the solution the first pass is clean."""
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat, var_thresholds

    n, m, gen, seed = PIN_CASE
    offs, lits = generate_ksat(gen, n, m, 3)
    with Solver(n, offs, lits, seed=1) as plain:
        assert plain.solve()["solved"] == 1
        sol = plain.assignment()
    pinned = np.arange(n) % 2 == 0
    p = np.where(pinned, sol.astype(np.float64), 0.5)
    with Solver(n, offs, lits, seed=seed, max_iters=PIN_CAP, probabilities=p) as s:
        a0 = s.assignment()
        np.testing.assert_array_equal(a0[pinned], sol[pinned])
        st = s.solve()
        assert st["solved"] == 1 and 1 < st["n_iterations"] <= PIN_CAP, st
        a = s.assignment()
        np.testing.assert_array_equal(a[pinned], sol[pinned])
        assert s.verify() == (True, 0)
        nu, _ = oracle_mod.eval_mask(offs, lits, oracle_mod.pack_bools(a))
        assert nu == 0
    with Solver(n, offs, lits, seed=seed, max_iters=PIN_CAP) as s:
        s.set_thresholds(var_thresholds(sol.astype(np.float64)))
        np.testing.assert_array_equal(s.assignment(), sol)
        st = s.solve()
        assert (st["solved"], st["n_iterations"], st["n_resamples"]) == (1, 1, 0)


def test_pins_that_cannot_be_met(gpu, native):
    """5. A clause whose literals are all pinned false: the loop runs to max_iters, the pins stay."""
    from alllsatisfiabilitysolver_amd import Solver

    # (x0 | x1 | x2), (x3 | !x4 | x5), (!x3 | x4 | x0); x0 x1 x2 pinned to 0, x5 to 1
    offs = np.array([0, 3, 6, 9], np.uint64)
    lits = np.array([0, 2, 4, 6, 9, 10, 7, 8, 0], np.uint32)
    thr = np.array([0, 0, 0, HALF, HALF, PIN1], np.uint32)
    with Solver(6, offs, lits, seed=3, max_iters=20) as s:
        s.set_thresholds(thr)
        st = native.Stats()
        assert s._L.alll_solve(s._ctx, ctypes.byref(st)) == native.ALLL_ERR_MAX_ITERS
        assert native.last_error()
        assert (st.solved, st.n_iterations) == (0, 20) and st.n_violated >= 1
        assert s.assignment()[[0, 1, 2, 5]].tolist() == [0, 0, 0, 1]
        assert s.verify()[0] is False


def test_restore(gpu):
    """6. Thresholds set and taken back: the unbiased fill and stream of a plain Solver."""
    from alllsatisfiabilitysolver_amd import Solver

    n, offs, lits, seed, thr, _, _ = trajectory_case()
    with Solver(n, offs, lits, seed=seed) as plain, Solver(n, offs, lits, seed=seed) as s:
        s.set_thresholds(thr)
        assert not np.array_equal(s.assignment_words(), plain.assignment_words())
        s.set_thresholds(None)
        np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words())
        for it in range(6):
            assert s.run(1) == plain.run(1), it
            np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words(), err_msg=f"iteration {it}")
            np.testing.assert_array_equal(s.mis(), plain.mis())
        assert plain.stats()["n_resamples"] > 0


def test_refusals(gpu, native):
    """7. After the first iteration, a wrong count, and the configurations the draws do not cover."""
    from alllsatisfiabilitysolver_amd import AlllError, Solver

    n, offs, lits, seed, thr, _, _ = trajectory_case()

    def refused(s, t, code):
        with pytest.raises(AlllError) as ei:
            s.set_thresholds(t)
        assert ei.value.code == code
        assert native.last_error()

    with Solver(n, offs, lits, seed=seed) as s:
        refused(s, thr[:-1], native.ALLL_ERR_INVALID_ARG)
        refused(s, np.concatenate([thr, thr[:1]]), native.ALLL_ERR_INVALID_ARG)
        s.set_thresholds(thr)  # (the refused calls changed nothing: this one is still allowed)
        s.run(1)
        refused(s, thr, native.ALLL_ERR_INVALID_ARG)
        refused(s, None, native.ALLL_ERR_INVALID_ARG)
    with Solver(n, offs, lits, seed=seed, flags=REFERENCE_RNG) as s:
        refused(s, thr, native.ALLL_ERR_UNSUPPORTED)
    with Solver(n, offs, lits, seed=seed, stream_batch=64) as s:
        refused(s, thr, native.ALLL_ERR_UNSUPPORTED)


CUBE_SEEDS = [31, 32, 33, 34, 35]


def cube_thresholds(n, i):
    """Cube i of variables 0 and 1 (00, 01, 10, 11: variable 0 is the high digit); the rest fair."""
    thr = np.full(n, HALF, np.uint32)
    thr[0] = PIN1 if i & 2 else 0
    thr[1] = PIN1 if i & 1 else 0
    return thr


def one_solver(item, seed, thr, max_iters=0):
    from alllsatisfiabilitysolver_amd import Solver

    s = Solver(*item, seed=seed, max_iters=max_iters)
    if thr is not None:
        s.set_thresholds(thr)
    return s


def test_group_cube_portfolio(gpu, native):
    """8. One instance five times: four cubes of two pinned variables and an item without
    thresholds.  Every item follows a Solver of its own, step by step and to the first solved."""
    from alllsatisfiabilitysolver_amd import GroupSolver, generate_ksat

    n, m = 203, 500
    item = (n, *generate_ksat(6, n, m, 3))
    thrs = [cube_thresholds(n, i) for i in range(4)] + [None]
    ones = [one_solver(item, s, t) for s, t in zip(CUBE_SEEDS, thrs)]
    try:
        with GroupSolver([item] * 5, CUBE_SEEDS) as g:
            for i in range(4):
                g.set_thresholds(i, thrs[i])
            for i, one in enumerate(ones):
                np.testing.assert_array_equal(g.assignment_words(i), one.assignment_words(), err_msg=f"fill, item {i}")
            busy = 0
            for it in range(10):
                res = g.run(1)
                for i, one in enumerate(ones):
                    st = one.run(1)
                    assert {k: res[i][k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (i, it)
                    np.testing.assert_array_equal(g.assignment_words(i), one.assignment_words(),
                                                  err_msg=f"item {i}, iteration {it}")
                    busy += st["n_violated"] > 0
            assert busy >= 15  # (the comparison is of running items, not of solved ones)
            for i in range(4):
                a = g.assignment_words(i)
                assert (int(a[0]) & 3) == ((i >> 1) | ((i & 1) << 1)), i
    finally:
        for one in ones:
            one.close()
    # first solved under a cap: the winner and its statistics from the five solvers
    cap = 400
    want = []
    for s, t in zip(CUBE_SEEDS, thrs):
        with one_solver(item, s, t, max_iters=cap) as one:
            want.append((one.solve(), one.assignment_words()))
    solved = [i for i, (st, _) in enumerate(want) if st["solved"]]
    assert solved
    winner = min(solved, key=lambda i: (want[i][0]["n_iterations"], i))
    with GroupSolver([item] * 5, CUBE_SEEDS, max_iters=cap) as g:
        for i in range(4):
            g.set_thresholds(i, thrs[i])
        res = g.solve(first_solved=True)
        got = [i for i, r in enumerate(res) if r["solved"]]
        assert got and min(got, key=lambda i: (res[i]["n_iterations"], i)) == winner
        assert {k: res[winner][k] for k in STAT_KEYS} == {k: want[winner][0][k] for k in STAT_KEYS}
        np.testing.assert_array_equal(g.assignment_words(winner), want[winner][1])
        for i, r in enumerate(res):
            if not r["solved"]:
                assert r["n_iterations"] < want[i][0]["n_iterations"] or not want[i][0]["solved"]


def test_group_item_boundary(gpu, native):
    """8b. A biased item of n = 33 between an unbiased and a biased one: the per-word bit changes at
    both of its ends, and its second word holds one variable.  Thresholds taken back restore the item."""
    from alllsatisfiabilitysolver_amd import AlllError, GroupSolver, generate_ksat

    items = [(203, *generate_ksat(6, 203, 500, 3)), (33, *generate_ksat(3, 33, 20, 2)), (100, *generate_ksat(8, 100, 420, 3)),
             (70, *generate_ksat(9, 70, 300, 3))]
    seeds = [41, 42, 43, 44]
    thrs = [None, mixed_thresholds(33, 2, must=[(31, PIN1), (32, 0x30000000)]), mixed_thresholds(100, 5), None]
    ones = [one_solver(it, s, t) for it, s, t in zip(items, seeds, thrs)]
    try:
        with GroupSolver(items, seeds) as g:
            g.set_thresholds(3, mixed_thresholds(70, 6))
            for i in (1, 2):
                g.set_thresholds(i, thrs[i])
            g.set_thresholds(3, None)  # item 3 is unbiased again, fill and stream
            with pytest.raises(AlllError) as ei:
                g.set_thresholds(1, thrs[2])  # 100 thresholds for 33 variables
            assert ei.value.code == native.ALLL_ERR_INVALID_ARG
            for i, one in enumerate(ones):
                np.testing.assert_array_equal(g.assignment_words(i), one.assignment_words(), err_msg=f"fill, item {i}")
            for it in range(6):
                res = g.run(1)
                for i, one in enumerate(ones):
                    st = one.run(1)
                    assert {k: res[i][k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (i, it)
                    np.testing.assert_array_equal(g.assignment_words(i), one.assignment_words(),
                                                  err_msg=f"item {i}, iteration {it}")
            with pytest.raises(AlllError) as ei:
                g.set_thresholds(0, None)  # after the first iteration
            assert ei.value.code == native.ALLL_ERR_INVALID_ARG and native.last_error()
    finally:
        for one in ones:
            one.close()
