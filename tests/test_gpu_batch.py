"""Batches of LDS-resident instances (BatchSolver, alll_batch_*) on the GPU: every item's
trajectory is fully determined by (instance, seed), so each is compared bit for bit with the
oracle (CPU restatement of the serial path) and with the one-instance path (Solver)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
CAP = 300


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


def check_item(b, i, res, st_o, A_o, native, what):
    got = {k: res[k] for k in STAT_KEYS}
    assert got == oracle_stats(st_o), (what, i)
    if "status" in res:
        assert res["status"] == (native.ALLL_OK if st_o["solved"] else native.ALLL_ERR_MAX_ITERS), (what, i)
    assert res["n_gpus"] == 1 and res["gpu_resamples"] == [st_o["n_resamples"]], (what, i)
    np.testing.assert_array_equal(b.assignment_words(i), A_o, err_msg=f"{what} item {i}")


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    """The mixed batch: (problems, seeds, oracle results at max_iters = CAP), computed once."""
    from alllsatisfiabilitysolver_amd import generate_ksat, generate_mixed

    problems, seeds = [], []

    def add(n, offs, lits, ss):
        for s in ss:
            problems.append((n, offs, lits))
            seeds.append(s)

    add(200, *generate_ksat(1, 200, 400, 3), range(1, 17))
    add(1000, *generate_ksat(1, 1000, 2400, 3), range(1, 5))
    add(1500, *generate_ksat(1, 1500, 2500, 8), range(1, 3))
    add(8192, *generate_ksat(1, 8192, 8192, 3), [1])            # exactly at all three limits
    add(200, *generate_ksat(1, 200, 800, 3), range(1, 3))       # unsolved at the cap
    add(2000, *generate_ksat(1, 2000, 5000, 3, 1), range(1, 3))  # power-law, unsolved at the cap
    add(900, *generate_mixed(5, 900, 2000, 1, 11), range(1, 3))  # mixed widths, unsolved at the cap
    f = dict(np.load(os.path.join(GOLDEN, "edge_T1.npz")))
    add(int(f["n_vars"]), f["offs"], f["lits"], [3])
    add(10, np.zeros(1, np.uint64), np.zeros(0, np.uint32), [4])                      # m = 0
    add(5, np.array([0, 0], np.uint64), np.zeros(0, np.uint32), [5])                   # one empty clause
    want = [oracle_mod.solve(n, o, l, s, max_iters=CAP) for (n, o, l), s in zip(problems, seeds)]
    return problems, seeds, want


@pytest.mark.parametrize("slice_", [1, 7, 0], ids=["slice1", "slice7", "default"])
def test_mixed_batch_matches_oracle(gpu, native, mixed, slice_):
    from alllsatisfiabilitysolver_amd import BatchSolver

    problems, seeds, want = mixed
    with BatchSolver(problems, seeds, max_iters=CAP) as b:
        b.set_slice(slice_)
        res = b.solve()
        assert len(res) == len(problems)
        for i, (st_o, A_o, _) in enumerate(want):
            check_item(b, i, res[i], st_o, A_o, native, f"slice {slice_}")
            assert b.stats(i)["n_iterations"] == st_o["n_iterations"]
    # the empty clause is never solved and resamples nothing; m = 0 is solved by its first pass
    assert res[-1]["solved"] == 0 and res[-1]["n_resamples"] == 0 and res[-1]["n_iterations"] == CAP
    assert res[-2]["solved"] == 1 and res[-2]["n_iterations"] == 1


def test_step_parity(gpu, oracle_mod, mixed):
    """run(1) twelve times: the assignment and the statistics after every step are the oracle's trace rows."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    problems, seeds, _ = mixed
    pick = [0, 16, 27]  # (200, 400, 3); (1000, 2400, 3); mixed widths
    sub = [problems[i] for i in pick]
    sd = [seeds[i] for i in pick]
    traces = [oracle_mod.solve(n, o, l, s, max_iters=13, trace=True)[2] for (n, o, l), s in zip(sub, sd)]
    with BatchSolver(sub, sd) as b:
        sum_mis = [0] * len(sub)
        n_res = [0] * len(sub)
        for step in range(12):
            res = b.run(1)
            for i, rows in enumerate(traces):
                assert len(rows) > step  # (none of the three is solved this early)
                it, nu, nm, dres, A_after = rows[step]
                sum_mis[i] += nm
                n_res[i] += dres
                assert res[i]["n_iterations"] == it == step + 1
                assert res[i]["n_violated"] == nu and res[i]["sum_mis_size"] == sum_mis[i]
                assert res[i]["n_resamples"] == n_res[i]
                np.testing.assert_array_equal(b.assignment_words(i), A_after, err_msg=f"item {i} step {step}")


@pytest.mark.parametrize("n_clauses", [513, 65, 64])
def test_deep_lfmis_chain(gpu, native, oracle_mod, n_clauses):
    """Clauses (x_i or x_{i+1}), all false: every clause is violated, the MIS is every second
    clause, and a claim scheme needs one dependent round per MIS clause."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    n = n_clauses + 1
    offs = np.arange(n_clauses + 1, dtype=np.uint64) * 2
    lits = np.stack([2 * np.arange(n_clauses), 2 * np.arange(1, n_clauses + 1)], 1).astype(np.uint32).ravel()
    A0 = np.zeros((n + 31) // 32, np.uint32)
    st_o, A_o, rows = oracle_mod.solve(n, offs, lits, 9, max_iters=CAP, A0=A0, trace=True)
    assert rows[0][1] == n_clauses and rows[0][2] == (n_clauses + 1) // 2
    with BatchSolver([(n, offs, lits)] * 2, [9, 9], max_iters=CAP) as b:
        for i in range(2):
            b.set_assignment_words(i, A0)
        first = b.run(1)
        for i in range(2):
            assert first[i]["sum_mis_size"] == rows[0][2] and first[i]["n_resamples"] == rows[0][3]
            np.testing.assert_array_equal(b.assignment_words(i), rows[0][4])
        res = b.solve()
        for i in range(2):
            check_item(b, i, res[i], st_o, A_o, native, f"chain {n_clauses}")


def test_more_items_than_resident_workgroups(gpu, native, oracle_mod):
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat

    n = 200
    offs, lits = generate_ksat(1, n, 400, 3)
    seeds = list(range(1, 601))
    with BatchSolver([(n, offs, lits)] * len(seeds), seeds, max_iters=CAP) as b:
        res = b.solve()
        for i, s in enumerate(seeds):
            st_o, A_o, _ = oracle_mod.solve(n, offs, lits, s, max_iters=CAP)
            check_item(b, i, res[i], st_o, A_o, native, "600 items")


def test_same_answer_as_one_instance_path(gpu, mixed):
    from alllsatisfiabilitysolver_amd import BatchSolver, Solver

    problems, seeds, _ = mixed
    pick = [1, 17, 23]  # solved (200, 400); solved (1000, 2400); capped (200, 800)
    sub = [problems[i] for i in pick]
    sd = [seeds[i] for i in pick]
    with BatchSolver(sub, sd, max_iters=CAP) as b:
        res = b.solve()
        for i, ((n, o, l), s) in enumerate(zip(sub, sd)):
            with Solver(n, o, l, seed=s, max_iters=CAP) as one:
                st = one.solve()
                for k in STAT_KEYS + ("n_gpus", "gpu_resamples"):
                    assert res[i][k] == st[k], (i, k)
                np.testing.assert_array_equal(b.assignment_words(i), one.assignment_words())


def test_portfolio_first_solved(gpu, native, oracle_mod):
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat, solve_portfolio

    n, cap, sl = 200, 4000, 64
    offs, lits = generate_ksat(1, n, 520, 3)
    seeds = list(range(1, 33))
    full = [oracle_mod.solve(n, offs, lits, s, max_iters=cap) for s in seeds]
    early = {i for i, (st_o, _, _) in enumerate(full) if st_o["n_iterations"] <= sl}
    assert early  # (the instance was chosen so that some seed finishes inside the first slice)
    with BatchSolver([(n, offs, lits)] * len(seeds), seeds, max_iters=cap) as b:
        b.set_slice(sl)
        res = b.solve(first_solved=True)
        assert {i for i, r in enumerate(res) if r["solved"]} == early
        for i, s in enumerate(seeds):
            if i in early:
                check_item(b, i, res[i], full[i][0], full[i][1], native, "portfolio, first slice")
            else:
                assert res[i]["n_iterations"] == sl and res[i]["status"] == native.ALLL_ERR_MAX_ITERS
                rows = oracle_mod.solve(n, offs, lits, s, max_iters=sl + 1, trace=True)[2]
                assert rows[sl - 1][0] == sl
                np.testing.assert_array_equal(b.assignment_words(i), rows[sl - 1][4])
        res = b.solve()
        for i in range(len(seeds)):
            assert full[i][0]["solved"] == 1
            check_item(b, i, res[i], full[i][0], full[i][1], native, "portfolio, finished")
    best = min(range(len(seeds)), key=lambda i: (full[i][0]["n_iterations"], i))
    seed, st, A = solve_portfolio(n, offs, lits, seeds, max_iters=cap)
    assert seed == seeds[best] and st["n_iterations"] == full[best][0]["n_iterations"] and st["solved"] == 1
    np.testing.assert_array_equal(A, full[best][1])


def test_run_then_solve(gpu, native, oracle_mod):
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat

    n = 1000
    offs, lits = generate_ksat(1, n, 2400, 3)
    st_o, A_o, _ = oracle_mod.solve(n, offs, lits, 2, max_iters=CAP)
    assert st_o["n_iterations"] > 10
    with BatchSolver([(n, offs, lits)], [2], max_iters=CAP) as b:
        st = b.run(10)
        assert st[0]["n_iterations"] == 10 and st[0]["solved"] == 0
        res = b.solve()
        check_item(b, 0, res[0], st_o, A_o, native, "run then solve")


@pytest.mark.parametrize("serial", [1, 8, 64])
def test_lfmis_choice_is_invisible(gpu, native, oracle_mod, mixed, monkeypatch, serial):
    """Violated sets of at most ALLL_BATCH_SERIAL_MAX clauses take the one-wave serial greedy, larger
    ones the claim rounds: same results.  The chains of 64 and 65 clauses sit on both sides of a
    full wave."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    monkeypatch.setenv("ALLL_BATCH_SERIAL_MAX", str(serial))
    problems, seeds, want = mixed
    with BatchSolver(problems, seeds, max_iters=CAP) as b:
        res = b.solve()
        for i, (st_o, A_o, _) in enumerate(want):
            check_item(b, i, res[i], st_o, A_o, native, f"serial {serial}")
    chains = []
    for mc in (64, 65):
        offs = np.arange(mc + 1, dtype=np.uint64) * 2
        lits = np.stack([2 * np.arange(mc), 2 * np.arange(1, mc + 1)], 1).astype(np.uint32).ravel()
        chains.append((mc + 1, offs, lits))
    with BatchSolver(chains, [9, 9], max_iters=CAP) as b:
        for i, (n, offs, lits) in enumerate(chains):
            b.set_assignment_words(i, np.zeros((n + 31) // 32, np.uint32))
        res = b.solve()
        for i, (n, offs, lits) in enumerate(chains):
            st_o, A_o, _ = oracle_mod.solve(n, offs, lits, 9, max_iters=CAP, A0=np.zeros((n + 31) // 32, np.uint32))
            check_item(b, i, res[i], st_o, A_o, native, f"serial {serial}, chain {n - 1}")


# ---------------------------------------------------------------------------------------------
# Crafted conflict graphs (tests/lfmis_structures.py) that fit an item (at most 8192 variables,
# 8192 clauses, 24576 literals): the chains need 2049 claim rounds and more than 64 ballot
# groups (the prefix scan takes a second pass); the star, the copies and the dense instances put
# thousands of claims on a few LDS addresses.

@pytest.fixture(scope="module")
def structures_batch(oracle_mod):
    """(problems, all-false words, oracle row of the first iteration and results at max_iters = CAP)."""
    import lfmis_structures as S

    problems = [S.chain(4097), S.rchain(4097), S.star(8191, 1), S.copies(8192), S.dense(5000, 8, 3),
                S.dense(5000, 40, 3), S.combs(16, 300, 2)]
    from alllsatisfiabilitysolver_amd import batch_fits

    for n, offs, lits in problems:
        assert batch_fits(n, offs.size - 1, lits.size)
    A0 = [S.all_false(n) for n, _, _ in problems]
    want = [oracle_mod.solve(n, o, l, 9, max_iters=CAP, A0=a, trace=True) for (n, o, l), a in zip(problems, A0)]
    # (|U|, |M|) of the first iteration: the chains, the star, the copies as constructed
    assert [w[2][0][1:3] for w in want[:4]] == [(4097, 2049), (4097, 2049), (8191, 1), (8192, 1)]
    assert want[6][2][0][1:3] == (4800, 2400)
    return problems, A0, want


@pytest.mark.parametrize("mode", ["slice1", "default", "serial64", "rounds"])
def test_structures_batch_matches_oracle(gpu, native, structures_batch, monkeypatch, mode):
    """One run(1) from all-false, then solve(): every item against the oracle.  mode "rounds":
    the chains report at least their 2049 claim rounds (claim_rounds, pinned on the CPU); if a
    later LFMIS needs fewer, the chains no longer exercise the deep rounds and must be
    replaced."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    problems, A0, want = structures_batch
    if mode == "serial64":
        monkeypatch.setenv("ALLL_BATCH_SERIAL_MAX", "64")
    with BatchSolver(problems, [9] * len(problems), max_iters=CAP) as b:
        if mode == "slice1":
            b.set_slice(1)
        for i, a in enumerate(A0):
            b.set_assignment_words(i, a)
        first = b.run(1)
        for i, (st_o, A_o, rows) in enumerate(want):
            it, nu, nm, dres, A_after = rows[0]
            assert first[i]["n_violated"] == nu and first[i]["sum_mis_size"] == nm, (mode, i)
            assert first[i]["n_resamples"] == dres, (mode, i)
            np.testing.assert_array_equal(b.assignment_words(i), A_after, err_msg=f"{mode} item {i} step 0")
        if mode == "rounds":
            for i in (0, 1):
                assert b.stats(i)["lfmis_rounds_max"] >= 2049
            assert b.stats(6)["lfmis_rounds_max"] >= 150
        res = b.solve()
        for i, (st_o, A_o, _) in enumerate(want):
            check_item(b, i, res[i], st_o, A_o, native, f"structures, {mode}")
