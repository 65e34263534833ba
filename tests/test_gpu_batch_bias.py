"""Per-variable resample probabilities and pinned variables in BatchSolver on the GPU (DESIGN.md §4.6,
§4.8; alll_batch_set_var_thresholds): the biased instantiation of the batch kernel, with LDS-resident
thresholds and with thresholds read from global memory, against bias_cases.py, which composes the
oracle's own primitives into the biased loop.  Every comparison is bit for bit: the assignment words,
n_iterations, n_violated, sum_mis_size, n_resamples and solved."""
import functools

import numpy as np
import pytest

from bias_cases import PIN1, mixed_thresholds, reference, unbiased_reference
from test_batch_bias_host import rule_fits
from test_gpu_bias import cube_thresholds, edge_1, edge_33, edge_mixed, trajectory_case

pytestmark = pytest.mark.gpu

KEYS = ("n_iterations", "n_violated", "sum_mis_size", "n_resamples", "solved")
STEPS = 12


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


# ---------------------------------------------------------------------------------------------
# What a batch item shows after k calls of run(1), and after solve(), from the rows of a CPU reference
# (bias_cases.reference: per iteration (violated mask, |U|, MIS, its literal count, next assignment);
# the rows end with the iteration that found nothing violated)


def after_steps(A0, rows, k):
    """(statistics, assignment) after k iterations asked of an item: it stops at its solving pass."""
    k = min(k, len(rows))
    done = rows[:k]
    nu = done[-1][1]
    st = dict(n_iterations=k, n_violated=nu, sum_mis_size=sum(r[2].size for r in done if r[1]),
              n_resamples=sum(r[3] for r in done if r[1]), solved=int(nu == 0))
    last = [r for r in done if r[1]]  # (the solving pass changes nothing)
    return st, (last[-1][4] if last else A0)


def after_solve(A0, rows, cap):
    """(statistics, assignment) after solve() under max_iters = cap, from rows computed with `cap`
    iterations: the capped pass counts and evaluates but does not resample."""
    if rows[-1][1] == 0:
        return after_steps(A0, rows, len(rows))
    assert len(rows) == cap
    st, A = after_steps(A0, rows, cap - 1) if cap > 1 else (dict(sum_mis_size=0, n_resamples=0), A0)
    return dict(st, n_iterations=cap, n_violated=rows[-1][1], solved=0), A


def check(b, i, res, want, what):
    st, A = want
    assert {k: res[k] for k in KEYS} == st, (what, i)
    np.testing.assert_array_equal(b.assignment_words(i), A, err_msg=f"{what}: item {i}")


def make_batch(case, **kw):
    from alllsatisfiabilitysolver_amd import BatchSolver

    b = BatchSolver(case["items"], case["seeds"], **kw)
    try:
        for i, t in enumerate(case["thrs"]):
            if t is not None:
                b.set_thresholds(i, t)
    except Exception:
        b.close()
        raise
    return b


def pins_hold(b, case):
    for i, t in enumerate(case["thrs"]):
        if t is not None and case["items"][i][0]:
            a = np.unpackbits(b.assignment_words(i).view(np.uint8), bitorder="little")[:t.size]
            assert (a[t == PIN1] == 1).all() and (a[t == 0] == 0).all(), i


def _frozen(case):
    for r in case["refs"]:
        r[0].flags.writeable = False
        for row in r[1]:
            for x in row:
                if isinstance(x, np.ndarray):
                    x.flags.writeable = False
    return case


# ---------------------------------------------------------------------------------------------
# 1. The mixed batch


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Seven items.  0, 1, 2 share one problem, generate_ksat(3, 203, 800, 3) (203 is no multiple of 4
    or 32; 800 clauses make a four-wave workgroup): seed 5 with the thresholds of
    test_gpu_bias.trajectory_case, seed 6 with other thresholds, seed 7 unbiased.  3: n = 33; 4: n = 1;
    5: mixed widths with repeated variables; 6: a biased item without clauses."""
    import oracle as o

    n, offs, lits, seed, thr, A0, rows = trajectory_case()
    shared = (n, offs, lits)
    items, seeds, thrs = [shared, shared, shared], [seed, 6, 7], [thr, mixed_thresholds(n, 9), None]
    for case in (edge_33, edge_1, edge_mixed):
        item, s, t = case()
        items.append(item)
        seeds.append(s)
        thrs.append(t)
    items.append((10, np.zeros(1, np.uint64), np.zeros(0, np.uint32)))
    seeds.append(4)
    thrs.append(mixed_thresholds(10, 5, must=[(0, PIN1), (9, 0)]))
    refs = [(A0, rows)]
    for item, s, t in list(zip(items, seeds, thrs))[1:-1]:
        refs.append(unbiased_reference(o, *item, s, STEPS) if t is None else reference(o, *item, s, t, STEPS))
    # no clause: the biased fill, and a first pass that finds nothing violated
    from bias_cases import biased_init

    fill = biased_init(o, seeds[-1], 10, thrs[-1])
    refs.append((fill, [(np.zeros(0, np.uint64), 0, np.zeros(0, np.uint32), 0, fill)]))
    return _frozen(dict(items=items, seeds=seeds, thrs=thrs, refs=refs))


def assert_mixed_conditions(case):
    """What the comparisons rely on, on the CPU reference."""
    refs, thrs = case["refs"], case["thrs"]
    for i in (0, 1, 2):
        assert len(refs[i][1]) == STEPS and refs[i][1][-1][1] > 0, i  # unsolved through the twelve iterations
    for i in (3, 4, 5):
        assert refs[i][1][0][1] > 0, i  # something is violated at the start: a resample is compared
    assert (thrs[0] == 0).sum() >= 10 and (thrs[0] == PIN1).sum() >= 10
    assert not np.array_equal(thrs[0], thrs[1]) and not np.array_equal(refs[0][0], refs[1][0])
    assert case["items"][0][1] is case["items"][1][1] is case["items"][2][1]  # one copy of the clauses


def follow_mixed(case, what, slice_=None):
    """The fill and twelve run(1) steps of every item; then the same twelve iterations in one call of a
    second batch, which reloads the thresholds with every slice."""
    with make_batch(case) as b:
        if slice_ is not None:
            b.set_slice(slice_)
        for i, (A0, _) in enumerate(case["refs"]):
            np.testing.assert_array_equal(b.assignment_words(i), A0, err_msg=f"{what}: fill, item {i}")
        for step in range(STEPS):
            res = b.run(1)
            for i, (A0, rows) in enumerate(case["refs"]):
                check(b, i, res[i], after_steps(A0, rows, step + 1), f"{what}, step {step}")
        pins_hold(b, case)
    with make_batch(case) as b:
        if slice_ is not None:
            b.set_slice(slice_)
        res = b.run(STEPS)
        for i, (A0, rows) in enumerate(case["refs"]):
            check(b, i, res[i], after_steps(A0, rows, STEPS), f"{what}, {STEPS} at once")
            assert b.stats(i)["n_iterations"] == res[i]["n_iterations"]
        pins_hold(b, case)


@pytest.mark.parametrize("slice_", [1, 7, 0], ids=["slice1", "slice7", "default"])
def test_mixed_batch(gpu, oracle_mod, slice_):
    """1. Biased and unbiased items side by side, two sets of thresholds on one stored problem."""
    case = mixed_case()
    assert_mixed_conditions(case)
    # (the thresholds of this batch fit the LDS: 203 variables, 800 clauses, 2400 literals at most)
    assert rule_fits(300, 800, 2400)
    follow_mixed(case, f"slice {slice_}", slice_)


# ---------------------------------------------------------------------------------------------
# 2. Both threshold paths

LIMITS_MUST = [(8191, PIN1), (8190, 0x40000000), (4095, 0), (4096, PIN1)]


@functools.lru_cache(maxsize=None)
def path_case(which):
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    if which == "global":  # the item at all three limits: its thresholds do not fit the LDS
        n, gen, thr = 8192, 1, mixed_thresholds(8192, 11, must=LIMITS_MUST)
    else:  # LDS-resident thresholds in a workgroup of 1024 threads
        n, gen, thr = 2048, 2, mixed_thresholds(2048, 12)
    item = (n, *generate_ksat(gen, n, 8192, 3))
    return _frozen(dict(items=[item], seeds=[9], thrs=[thr], refs=[reference(o, *item, 9, thr, 6)]))


@pytest.mark.parametrize("which", ["global", "lds"])
def test_threshold_paths_by_size(gpu, oracle_mod, which):
    """2. Six steps of an item whose thresholds are read from global memory (by size) and of one whose
    thresholds are LDS-resident."""
    case = path_case(which)
    n = case["items"][0][0]
    assert rule_fits(n, 8192, 24576) == (which == "lds")
    A0, rows = case["refs"][0]
    assert len(rows) == 6 and all(r[1] > 0 for r in rows)  # unsolved throughout
    print(which, "|U| per iteration", [r[1] for r in rows])
    with make_batch(case) as b:
        np.testing.assert_array_equal(b.assignment_words(0), A0, err_msg="fill")
        for step in range(6):
            res = b.run(1)
            check(b, 0, res[0], after_steps(A0, rows, step + 1), f"{which}, step {step}")
        pins_hold(b, case)


def test_mixed_batch_from_global_memory(gpu, oracle_mod, monkeypatch):
    """2. The mixed batch again with the thresholds forced to global memory: the same results."""
    monkeypatch.setenv("ALLL_BATCH_THR_GLOBAL", "1")
    case = mixed_case()
    assert_mixed_conditions(case)
    follow_mixed(case, "global thresholds")


# ---------------------------------------------------------------------------------------------
# 4. (and 3.) The cube portfolio

CUBE_SEEDS = [31, 32, 33, 34, 35]
CUBE_CAP = 400


@functools.lru_cache(maxsize=None)
def cube_case():
    """generate_ksat(6, 203, 500, 3) five times: the four cubes of variables 0 and 1, and an item
    without thresholds; every reference runs to its end or to the cap."""
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    n = 203
    item = (n, *generate_ksat(6, n, 500, 3))
    thrs = [cube_thresholds(n, i) for i in range(4)] + [None]
    refs = [unbiased_reference(o, *item, s, CUBE_CAP) if t is None else reference(o, *item, s, t, CUBE_CAP)
            for s, t in zip(CUBE_SEEDS, thrs)]
    return _frozen(dict(items=[item] * 5, seeds=list(CUBE_SEEDS), thrs=thrs, refs=refs))


def test_serial_greedy_shares_the_biased_draw(gpu, oracle_mod, monkeypatch):
    """3. ALLL_BATCH_SERIAL_MAX = 64: violated sets of at most 64 clauses take the one-wave serial greedy,
    whose joins draw through the same small_join.  The mixed batch step by step, and the cube items to
    their end (their violated sets shrink through 64 on the way)."""
    monkeypatch.setenv("ALLL_BATCH_SERIAL_MAX", "64")
    case = mixed_case()
    assert_mixed_conditions(case)
    small = [i for i, t in enumerate(case["thrs"]) if t is not None and any(0 < r[1] <= 64 for r in case["refs"][i][1])]
    assert small  # a biased item with a violated set of at most 64 clauses within the twelve steps
    follow_mixed(case, "serial 64")
    cubes = cube_case()
    sizes = [[r[1] for r in ref[1]] for ref in cubes["refs"]]
    assert any(max(s) > 64 for s in sizes[:4])  # both LFMIS paths in one biased item
    for i in range(4):
        assert sum(0 < s <= 64 for s in sizes[i]) >= 100, i  # the serial greedy, many times
    with make_batch(cubes, max_iters=CUBE_CAP) as b:
        res = b.solve()
        for i, (A0, rows) in enumerate(cubes["refs"]):
            check(b, i, res[i], after_solve(A0, rows, CUBE_CAP), "serial 64, cubes")


def test_cube_portfolio(gpu, native, oracle_mod):
    """4. First solved in slices of 64 under a cap of 400; the rest finished by a second solve(); the
    same five items in a GroupSolver; solve_cubes with a dead cube among the four."""
    from alllsatisfiabilitysolver_amd import GroupSolver, solve_cubes

    case = cube_case()
    refs, sl = case["refs"], 64
    finals = [after_solve(A0, rows, CUBE_CAP) for A0, rows in refs]
    solved = [i for i, (st, _) in enumerate(finals) if st["solved"]]
    assert set(solved) >= {0, 1, 2, 3}  # every cube ends solved within the cap
    print("iterations", [st["n_iterations"] for st, _ in finals], "solved", solved)
    winner = min(solved, key=lambda i: (finals[i][0]["n_iterations"], i))
    n_slices = -(-finals[winner][0]["n_iterations"] // sl)  # the call returns after the winner's slice
    assert n_slices >= 2 and n_slices * sl < CUBE_CAP  # more than one slice; nobody is capped meanwhile
    early = {i for i in solved if finals[i][0]["n_iterations"] <= n_slices * sl}
    with make_batch(case, max_iters=CUBE_CAP) as b:
        b.set_slice(sl)
        res = b.solve(first_solved=True)
        assert {i for i, r in enumerate(res) if r["solved"]} == early and winner in early
        assert min(early, key=lambda i: (res[i]["n_iterations"], i)) == winner
        for i, (A0, rows) in enumerate(refs):
            if i in early:
                check(b, i, res[i], finals[i], "first solved")
                assert res[i]["status"] == native.ALLL_OK
            else:  # a whole number of slices of its own trajectory
                assert res[i]["n_iterations"] == n_slices * sl and res[i]["status"] == native.ALLL_ERR_MAX_ITERS
                check(b, i, res[i], after_steps(A0, rows, n_slices * sl), "first solved, unsolved item")
        res = b.solve()
        for i in range(5):
            check(b, i, res[i], finals[i], "finished")
        pins_hold(b, case)
    with GroupSolver(case["items"], case["seeds"], max_iters=CUBE_CAP) as g:
        for i in range(4):
            g.set_thresholds(i, case["thrs"][i])
        res = g.solve()
        for i in range(5):
            check(g, i, res[i], finals[i], "group")
    # solve_cubes: cube i as literals (variable 0 is the high digit), a dead cube in the middle
    n, offs, lits = case["items"][0]
    lit_cubes = [[0 if i & 2 else 1, 2 if i & 1 else 3] for i in range(4)]
    for i, c in enumerate(lit_cubes):
        want = np.full(n, 1 << 31, np.uint32)
        want[[l >> 1 for l in c]] = [0 if l & 1 else PIN1 for l in c]
        np.testing.assert_array_equal(want, case["thrs"][i])
    dead = [int(l) ^ 1 for l in lits[int(offs[0]):int(offs[1])]]  # all three variables of clause 0 pinned false
    order = [0, 1, None, 2, 3]
    cubes = [dead if i is None else lit_cubes[i] for i in order]
    seeds = [99 if i is None else CUBE_SEEDS[i] for i in order]
    best4 = min(range(4), key=lambda i: (finals[i][0]["n_iterations"], i))
    idx, st, A = solve_cubes(n, offs, lits, cubes, seeds=seeds, max_iters=CUBE_CAP)
    assert idx == order.index(best4)
    assert {k: st[k] for k in KEYS} == finals[best4][0]
    np.testing.assert_array_equal(A, finals[best4][1])


# ---------------------------------------------------------------------------------------------
# 5. Restore and refusals


def test_restore(gpu):
    """5. Thresholds set and taken back: six steps equal to an untouched item of the same seed."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    n, offs, lits, seed, thr, _, _ = trajectory_case()
    with BatchSolver([(n, offs, lits)] * 2, [seed, seed]) as b:
        plain = b.assignment_words(1)
        b.set_thresholds(0, thr)
        assert not np.array_equal(b.assignment_words(0), plain)
        np.testing.assert_array_equal(b.assignment_words(1), plain)  # that item's words only
        b.set_thresholds(0, None)
        np.testing.assert_array_equal(b.assignment_words(0), plain)
        for it in range(6):
            res = b.run(1)
            assert {k: res[0][k] for k in KEYS} == {k: res[1][k] for k in KEYS}, it
            np.testing.assert_array_equal(b.assignment_words(0), b.assignment_words(1), err_msg=f"iteration {it}")
        assert res[1]["n_resamples"] > 0 and res[1]["n_iterations"] == 6


def test_refusals(gpu, native):
    """5. A wrong count, an item past the end, and calls after the first iteration.  The rule is per item
    (its n_iterations == 0), but every call that advances a batch advances all of its items, so no item
    can have run while a sibling has not: the rule is tested per batch.  The item without clauses is
    finished by its first pass and is refused like the others."""
    from alllsatisfiabilitysolver_amd import AlllError, BatchSolver

    n, offs, lits, seed, thr, A0, rows = trajectory_case()
    items = [(n, offs, lits), (10, np.zeros(1, np.uint64), np.zeros(0, np.uint32)), (n, offs, lits)]

    def refused(b, i, t):
        with pytest.raises(AlllError) as ei:
            b.set_thresholds(i, t)
        assert ei.value.code == native.ALLL_ERR_INVALID_ARG
        assert native.last_error()

    with BatchSolver(items, [seed, 4, 8]) as b:
        before = [b.assignment_words(i) for i in range(3)]
        refused(b, 0, thr[:-1])
        refused(b, 0, np.concatenate([thr, thr[:1]]))
        refused(b, 1, thr)  # 203 thresholds for 10 variables
        refused(b, 3, thr)  # item == n_items
        refused(b, 3, None)
        for i in range(3):  # a refused call changes nothing
            np.testing.assert_array_equal(b.assignment_words(i), before[i])
        b.set_thresholds(0, thr)  # ... and leaves a later valid call allowed
        np.testing.assert_array_equal(b.assignment_words(0), A0)
        res = b.run(1)
        assert [r["n_iterations"] for r in res] == [1, 1, 1] and res[1]["solved"] == 1
        check(b, 0, res[0], after_steps(A0, rows, 1), "after the refusals")
        for i, t in ((0, thr), (1, np.zeros(10, np.uint32)), (2, thr)):
            refused(b, i, t)
            refused(b, i, None)
        res = b.run(1)  # the refused calls changed nothing: item 0 goes on under its thresholds
        check(b, 0, res[0], after_steps(A0, rows, 2), "after the late refusals")


# ---------------------------------------------------------------------------------------------
# 6. Nothing else moved


def test_unbiased_items_do_not_move(gpu):
    """6. Items 0, 16 and 27 of test_gpu_batch's mixed batch after run(12): alone; beside an item that
    was given thresholds and then None (the batch is back on the unbiased kernel); and beside an item
    that keeps its thresholds (unbiased items inside the biased kernel)."""
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat, generate_mixed

    items = [(200, *generate_ksat(1, 200, 400, 3)), (1000, *generate_ksat(1, 1000, 2400, 3)),
             (900, *generate_mixed(5, 900, 2000, 1, 11))]
    seeds = [1, 1, 1]
    other = (200, *generate_ksat(1, 200, 800, 3))
    thr = mixed_thresholds(200, 13)
    with BatchSolver(items, seeds) as b:
        want = b.run(12)
        words = [b.assignment_words(i) for i in range(3)]
    assert all(r["n_iterations"] == 12 and r["solved"] == 0 and r["n_resamples"] > 0 for r in want)
    for keep in (False, True):
        with BatchSolver(items + [other], seeds + [2]) as b:
            b.set_thresholds(3, thr)
            if not keep:
                b.set_thresholds(3, None)
            res = b.run(12)
            for i in range(3):
                assert res[i] == want[i], (keep, i)
                np.testing.assert_array_equal(b.assignment_words(i), words[i], err_msg=f"keep {keep}, item {i}")
