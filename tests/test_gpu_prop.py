"""Unit propagation of the pinned variables on the GPU (alll_propagate_pins and its
group and batch forms): k_prop_pack / k_prop_scan / k_prop_apply and k_small_propagate against the
numpy reference of prop_cases.py, and the propagated context against a fresh one given the reference's
thresholds."""
import numpy as np
import pytest

import prop_cases as P

pytestmark = pytest.mark.gpu

NO_GRAPH, GENERIC_CSR, ATOMIC_CLAIMS, REFERENCE_RNG = 1 << 0, 1 << 2, 1 << 5, 1 << 7
STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def fill_words(seed, n, thr):
    """The biased fill of thresholds thr as packed words (the host form, itself tested against the oracle)."""
    from alllsatisfiabilitysolver_amd import biased_initial_assignment

    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = biased_initial_assignment(seed, n, thr)
    return np.packbits(bits, bitorder="little").view(np.uint32)


def own_solver(c, seed, flags=0, thr="thr"):
    from alllsatisfiabilitysolver_amd import Solver

    s = Solver(c["n"], c["offs"], c["lits"], seed=seed, flags=flags)
    if thr is not None:
        s.set_thresholds(c[thr])
    return s


CASE_FLAGS = [(name, 0) for name in P.ALL_CASES] + [(name, f) for name in ("A1", "A2", "E")
                                                   for f in (GENERIC_CSR, NO_GRAPH, ATOMIC_CLAIMS)]
# the layout every case is there for: fixed width 3, generic CSR, ragged
LAYOUT = {"A1": 3, "E": 0, "G": 3, "G2": 3, "H": 0, "H2": 0}


@pytest.mark.parametrize("name,flags", CASE_FLAGS, ids=[f"{n}-{f}" for n, f in CASE_FLAGS])
def test_cases(gpu, name, flags):
    """1. Every case through Solver.propagate_pins: the result, the thresholds and the refilled words.
    Cases G and G2 run on the instance whose hubs the planner flags hot (bit 31 of the clause-order
    literals the scan reads; the ABI has no query for the flags, test_prop_cases re-asserts the
    planner's criterion on the instance), H and H2 on the ragged layout."""
    c = P.case(name)
    with own_solver(c, 7, flags) as s:
        if not flags and name in LAYOUT:
            assert s.layout() == LAYOUT[name]
        if name in ("H", "H2"):
            assert s.eval_kernel() == "k_eval_ragged"
        if flags & GENERIC_CSR:
            assert s.layout() == 0
        res = s.propagate_pins(c["max_rounds"])
        print(name, flags, res)
        assert res == c["res"]
        np.testing.assert_array_equal(s.thresholds(), c["out"])
        np.testing.assert_array_equal(s.assignment_words(), fill_words(7, c["n"], c["out"]))


@pytest.mark.parametrize("name", ["A1", "A4"])
def test_propagated_context_is_a_fresh_one_with_the_propagated_thresholds(gpu, name):
    """2. Words at iteration 0 and after run(5), violated mask, MIS and statistics; the forced pins hold."""
    c = P.case(name)
    forced = np.flatnonzero(c["out"] != c["thr"])
    with own_solver(c, 11) as s, own_solver(c, 11, thr="out") as fresh:
        assert s.propagate_pins() == c["res"]
        np.testing.assert_array_equal(s.assignment_words(), fresh.assignment_words())
        a, b = s.run(5), fresh.run(5)
        assert a["n_iterations"] == 5 and {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        np.testing.assert_array_equal(s.assignment_words(), fresh.assignment_words())
        np.testing.assert_array_equal(s.violated_mask(), fresh.violated_mask())
        np.testing.assert_array_equal(s.mis(), fresh.mis())
        bits = s.assignment()
        assert forced.size == c["res"]["n_forced"]
        np.testing.assert_array_equal(bits[forced], (c["out"][forced] == P.PIN1).astype(np.uint8))


def test_refusals_and_repeats(gpu, native):
    """3. A second call, the calls that come too late or without thresholds, the contexts that
    thresholds refuse, and alll_track_best on either side of the call."""
    from alllsatisfiabilitysolver_amd import AlllError, Solver

    def refused(fn, code):
        with pytest.raises(AlllError) as ei:
            fn()
        assert ei.value.code == code and native.last_error()

    for name in ("B1", "B2", "B3"):
        c = P.case(name)
        with own_solver(c, 3) as s:
            assert s.propagate_pins() == c["res"]
            assert s.propagate_pins() == dict(c["res"], rounds=0, n_forced=0)
            np.testing.assert_array_equal(s.thresholds(), c["out"])
    cap, full = P.case("C_cap"), P.case("C")
    with own_solver(cap, 3) as s:  # the capped chain goes on where it stopped
        assert s.propagate_pins(100) == cap["res"]
        assert s.propagate_pins(0) == dict(full["res"], rounds=199, n_forced=199)
        np.testing.assert_array_equal(s.thresholds(), full["out"])
    c = P.case("B1")
    with own_solver(c, 3, thr=None) as s:
        refused(s.propagate_pins, native.ALLL_ERR_INVALID_ARG)  # no thresholds
        refused(s.thresholds, native.ALLL_ERR_INVALID_ARG)
        s.set_thresholds(c["thr"])
        s.run(1)
        refused(s.propagate_pins, native.ALLL_ERR_INVALID_ARG)  # too late
        np.testing.assert_array_equal(s.thresholds(), c["thr"])
    with Solver(c["n"], c["offs"], c["lits"], seed=3, flags=REFERENCE_RNG) as s:
        refused(s.propagate_pins, native.ALLL_ERR_UNSUPPORTED)
    with Solver(c["n"], c["offs"], c["lits"], seed=3, stream_batch=64) as s:
        refused(s.propagate_pins, native.ALLL_ERR_UNSUPPORTED)
    # tracking before the call and after it: the same records as a fresh tracking context
    with own_solver(c, 3, thr="out") as fresh:
        fresh.track_best()
        fresh.run(4)
        want = fresh.best()
    for before in (True, False):
        with own_solver(c, 3) as s:
            if before:
                s.track_best()
            assert s.propagate_pins() == c["res"]
            if not before:
                s.track_best()
            s.run(4)
            got = s.best()
            assert (got["n_violated"], got["iteration"]) == (want["n_violated"], want["iteration"])
            np.testing.assert_array_equal(got["words"], want["words"])


def two_sat_item():
    """33 variables (one full word and one bit), 2-SAT, x0 pinned 1: three rounds."""
    from alllsatisfiabilitysolver_amd import generate_ksat

    n = 33
    offs, lits = generate_ksat(42, n, 50, 2)
    thr = np.full(n, P.FAIR, np.uint32)
    thr[0] = P.PIN1
    out, res = P.propagate(n, offs, lits, thr)
    return dict(name="2sat", n=n, offs=offs, lits=lits, thr=thr, out=out, res=res, max_rounds=0)


def unbiased(c):
    return dict(c, thr=None, out=None, res=dict(status=P.NONE, rounds=0, n_forced=0, conflict_clause=len(c["offs"]) - 1))


def check_items(native, b, cases, seeds, run_iters, survivors_only):
    """The comparisons of the group and the batch test: every item's result, thresholds and words
    against the reference and against a Solver of its own; then run_iters iterations of both."""
    from alllsatisfiabilitysolver_amd import AlllError

    res = b.propagate_pins()
    print([(c["name"], r) for c, r in zip(cases, res)])
    own = []
    try:
        for i, (c, seed) in enumerate(zip(cases, seeds)):
            assert res[i] == c["res"], (i, c["name"])
            s = own_solver(c, seed, thr=None if c["thr"] is None else "thr")
            own.append(s)
            if c["thr"] is None:
                with pytest.raises(AlllError) as ei:
                    b.thresholds(i)
                assert ei.value.code == native.ALLL_ERR_INVALID_ARG
            else:
                assert s.propagate_pins() == c["res"]
                np.testing.assert_array_equal(b.thresholds(i), c["out"], err_msg=c["name"])
                np.testing.assert_array_equal(b.thresholds(i), s.thresholds(), err_msg=c["name"])
                np.testing.assert_array_equal(b.assignment_words(i), fill_words(seed, c["n"], c["out"]), err_msg=c["name"])
            np.testing.assert_array_equal(b.assignment_words(i), s.assignment_words(), err_msg=c["name"])
        again = b.propagate_pins()  # the same statuses, nothing more to apply
        assert again == [dict(c["res"], rounds=0, n_forced=0) for c in cases]
        stats = b.run(run_iters)
        for i, (c, s) in enumerate(zip(cases, own)):
            if survivors_only and c["res"]["status"] == P.CONFLICT:
                continue
            want = s.run(run_iters)
            assert {k: stats[i][k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}, c["name"]
            np.testing.assert_array_equal(b.assignment_words(i), s.assignment_words(), err_msg=c["name"])
    finally:
        for s in own:
            s.close()


def test_group(gpu, native):
    """4. Six items at different word bases: the three B cubes (a fixpoint after six rounds, a conflict
    after one, a conflict at round 0), B's instance without thresholds (left alone: its zeros in the
    union's thresholds are no pins), the chain C and a 33-variable 2-SAT item with a pin.  The chain
    runs 299 rounds: the items that ended in the first six are left alone for some 290 more."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    cases = [P.case("B1"), P.case("B2"), P.case("B3"), unbiased(P.case("B1")), P.case("C"), two_sat_item()]
    seeds = [21, 22, 23, 24, 25, 26]
    assert cases[5]["res"]["rounds"] == 3
    with GroupSolver([(c["n"], c["offs"], c["lits"]) for c in cases], seeds) as g:
        for i, c in enumerate(cases):
            if c["thr"] is not None:
                g.set_thresholds(i, c["thr"])
        check_items(native, g, cases, seeds, 2, survivors_only=False)
    # too late after the group's first iteration
    from alllsatisfiabilitysolver_amd import AlllError

    with GroupSolver([(c["n"], c["offs"], c["lits"]) for c in cases[:2]], seeds[:2]) as g:
        g.set_thresholds(0, cases[0]["thr"])
        g.run(1)
        with pytest.raises(AlllError) as ei:
            g.propagate_pins()
        assert ei.value.code == native.ALLL_ERR_INVALID_ARG


def test_batch(gpu, native):
    """5. The B cubes, C', D, E, F and an item without thresholds in one BatchSolver; after the
    propagation run(3) of every surviving item against a Solver of its own."""
    from alllsatisfiabilitysolver_amd import AlllError, BatchSolver

    cases = [P.case(name) for name in P.BATCH_CASES] + [unbiased(P.case("B1"))]
    seeds = list(range(31, 31 + len(cases)))
    with BatchSolver([(c["n"], c["offs"], c["lits"]) for c in cases], seeds) as b:
        for i, c in enumerate(cases):
            if c["thr"] is not None:
                b.set_thresholds(i, c["thr"])
        check_items(native, b, cases, seeds, 3, survivors_only=True)
        with pytest.raises(AlllError) as ei:  # an item has made an iteration
            b.propagate_pins()
        assert ei.value.code == native.ALLL_ERR_INVALID_ARG
    # a round cap inside the kernel, and a batch in which no item has thresholds
    c = P.case("C'")
    with BatchSolver([(c["n"], c["offs"], c["lits"])] * 2, [1, 2]) as b:
        assert [r["status"] for r in b.propagate_pins()] == [P.NONE, P.NONE]
        b.set_thresholds(1, c["thr"])
        res = b.propagate_pins(40)
        assert res[0]["status"] == P.NONE
        assert res[1] == dict(status=P.ROUND_CAP, rounds=40, n_forced=40, conflict_clause=len(c["offs"]) - 1)
        np.testing.assert_array_equal(b.thresholds(1), P.propagate(c["n"], c["offs"], c["lits"], c["thr"], 40)[0])


def cube_of(thr):
    v = np.flatnonzero(thr != P.FAIR)
    return (2 * v + (thr[v] == 0)).tolist()


def satisfied(offs, lits, words):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    lit_true = bits[lits >> 1] != (lits & 1)
    cl = np.repeat(np.arange(len(offs) - 1), np.diff(offs.astype(np.int64)))
    return bool((np.bincount(cl, lit_true, len(offs) - 1) > 0).all())


def test_solve_cubes_propagated(gpu):
    """6. On B's instance: the three B cubes and two live ones.  Then an instance at ratio 2, which
    the loop solves in a few iterations, under four cubes of 200 pins: one in conflict after a
    round of propagation (only the device's propagation drops it), one dead at depth 0, two live."""
    from alllsatisfiabilitysolver_amd import generate_ksat, solve_cubes_propagated

    def portfolio(n, offs, lits, thrs, max_iters):
        dead = [i for i, t in enumerate(thrs) if P.propagate(n, offs, lits, t)[1]["status"] == P.CONFLICT]
        win, st, words = solve_cubes_propagated(n, offs, lits, [cube_of(t) for t in thrs], max_iters=max_iters)
        print("winner", win, st and {k: st[k] for k in STAT_KEYS})
        if win is not None:
            assert win not in dead and st["solved"] == 1
            assert satisfied(offs, lits, words)
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
            pinned = np.flatnonzero(thrs[win] != P.FAIR)
            np.testing.assert_array_equal(bits[pinned], (thrs[win][pinned] == P.PIN1).astype(np.uint8))
        return win, dead

    n, offs, lits = P.b_instance()
    thrs = [P.case(name)["thr"] for name in ("B1", "B2", "B3", "B4", "B5")]
    _, dead = portfolio(n, offs, lits, thrs, 300)
    assert dead == [1, 2]
    n = 2003
    offs, lits = generate_ksat(7, n, 4000, 3)
    thrs = [P.cube(n, 200, cs) for cs in (10, 3, 0, 2)]
    win, dead = portfolio(n, offs, lits, thrs, 2000)
    assert dead == [0, 1] and win in (2, 3)
