"""Split scores and the cube splitter on the GPU (alll_var_scores and its group form,
split_cubes, solve_cubes_split): k_score_scan / k_score_pick_* against the numpy reference of
split_cases.py.  Every comparison is an equality; the facts the cases are there for are pinned on the
CPU in tests/test_split_cases.py."""
import ctypes

import numpy as np
import pytest

import prop_cases as P
import split_cases as C
from test_gpu_prop import ATOMIC_CLAIMS, GENERIC_CSR, NO_GRAPH, REFERENCE_RNG, STAT_KEYS, satisfied

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def own_solver(c, seed=7, flags=0, thr="thr", **kw):
    from alllsatisfiabilitysolver_amd import Solver

    s = Solver(c["n"], c["offs"], c["lits"], seed=seed, flags=flags, **kw)
    if thr is not None and c[thr] is not None:
        s.set_thresholds(c[thr])
    return s


CASE_FLAGS = [(name, 0) for name in C.ALL_CASES] + [(name, f) for name in C.FLAG_CASES
                                                   for f in (GENERIC_CSR, NO_GRAPH, ATOMIC_CLAIMS)]
# the layout a case is there for: fixed width 3, ragged
LAYOUT = {"A": 3, "PL": 3, "R": 0}


@pytest.mark.parametrize("name,flags", CASE_FLAGS, ids=[f"{n}-{f}" for n, f in CASE_FLAGS])
def test_cases(gpu, name, flags):
    """1. Every case through Solver.var_scores: the full score array and the record; the record alone
    is the same record."""
    c = C.case(name)
    with own_solver(c, flags=flags) as s:
        if not flags and name in LAYOUT:
            assert s.layout() == LAYOUT[name]
        if not flags and name == "R":
            assert s.eval_kernel() == "k_eval_ragged"
        if flags & GENERIC_CSR:
            assert s.layout() == 0
        S, rec = s.var_scores()
        print(name, flags, rec)
        assert rec == c["rec"]
        np.testing.assert_array_equal(S, c["S"])
        assert s.var_scores(with_scores=False) == c["rec"]


@pytest.mark.parametrize("track", [False, True])
def test_the_call_changes_nothing(gpu, track):
    """2. On A4: thresholds, var_scores, run(5) against the same without the call -- words, violated
    mask, MIS, statistics (and the best record); var_scores after run(3) is the call before it."""
    c = P.case("A4")
    want_S, want = C.scores(c["n"], c["offs"], c["lits"], c["thr"])
    with own_solver(c, 11, track_best=track) as s, own_solver(c, 11, track_best=track) as plain:
        S, rec = s.var_scores()
        assert rec == want
        np.testing.assert_array_equal(S, want_S)
        np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words())
        np.testing.assert_array_equal(s.thresholds(), c["thr"])
        a, b = s.run(3), plain.run(3)
        assert {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        S, rec = s.var_scores()  # mid-run: a function of clauses and thresholds only
        assert rec == want
        np.testing.assert_array_equal(S, want_S)
        a, b = s.run(2), plain.run(2)
        assert a["n_iterations"] == 5 and {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words())
        np.testing.assert_array_equal(s.violated_mask(), plain.violated_mask())
        np.testing.assert_array_equal(s.mis(), plain.mis())
        np.testing.assert_array_equal(s.thresholds(), c["thr"])
        if track:
            x, y = s.best(), plain.best()
            assert (x["n_violated"], x["iteration"]) == (y["n_violated"], y["iteration"])
            np.testing.assert_array_equal(x["words"], y["words"])


def test_refusals(gpu, native):
    from alllsatisfiabilitysolver_amd import AlllError, Solver

    c = C.case("B")
    for kw in (dict(flags=REFERENCE_RNG), dict(stream_batch=64)):
        with Solver(c["n"], c["offs"], c["lits"], seed=3, **kw) as s:
            with pytest.raises(AlllError) as ei:
                s.var_scores()
            assert ei.value.code == native.ALLL_ERR_UNSUPPORTED and native.last_error()
    with own_solver(c) as s:
        res, S = native.SplitResult(), np.zeros(2 * c["n"] + 2, np.uint64)
        p = S.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        for n_scores in (2 * c["n"] - 1, 2 * c["n"] + 2, 0):
            assert native.lib().alll_var_scores(s._ctx, p, n_scores, ctypes.byref(res)) == native.ALLL_ERR_INVALID_ARG
        assert not S.any()


def check_items(got, want, what):
    recs, arrays = got
    assert len(recs) == len(arrays) == len(want)
    bad = [(i, r, w[1]) for i, (r, w) in enumerate(zip(recs, want)) if r != w[1]]
    assert not bad, (what, len(bad), bad[:5])
    for i, (S, w) in enumerate(zip(arrays, want)):
        if not np.array_equal(S, w[0]):
            np.testing.assert_array_equal(S, w[0], err_msg=f"{what}: scores of item {i}")


@pytest.mark.parametrize("name", ["mixed_group", "ladder", "prop_swarm"])
def test_groups(gpu, name):
    """3. 199, 130 and 1000 items in one group: before the propagation under the items' own thresholds,
    after it under the propagated ones -- waves of words and of clauses that span many items,
    clauseless items, items without thresholds, items in conflict (their thresholds are those of the
    failing round's start), the star's hub."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = {"mixed_group": P.mixed_group, "ladder": P.ladder, "prop_swarm": P.prop_swarm}[name]()
    with GroupSolver(list(c["items"]), list(c["seeds"])) as g:
        for i, thr in enumerate(c["thrs"]):
            if thr is not None:
                g.set_thresholds(i, thr)
        check_items(g.var_scores(with_scores=True), C.many_scores(c, c["thrs"]), f"{name}, before")
        res = g.propagate_pins()
        assert [r["status"] for r in res] == [r["status"] for r in c["ress"]]
        want = C.many_scores(c, c["outs"])
        check_items(g.var_scores(with_scores=True), want, name)
        assert g.var_scores() == [w[1] for w in want]


def test_group_without_thresholds(gpu):
    """A group in which no item has thresholds (the union has no threshold array), and one of a single item."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    cases = [C.case(name) for name in ("B", "wide20", "tie_far", "taut", "R")]
    want = [C.scores(c["n"], c["offs"], c["lits"], None) for c in cases]
    with GroupSolver([(c["n"], c["offs"], c["lits"]) for c in cases], [1, 2, 3, 4, 5]) as g:
        check_items(g.var_scores(with_scores=True), want, "no thresholds")
        g.run(2)  # an item's being solved or ended does not matter
        check_items(g.var_scores(with_scores=True), want, "no thresholds, after run(2)")
    c = C.case("B4p")
    with GroupSolver([(c["n"], c["offs"], c["lits"])], [9]) as g:
        g.set_thresholds(0, c["thr"])
        check_items(g.var_scores(with_scores=True), [(c["S"], c["rec"])], "one item")


def check_leaves(got, want, what):
    assert [(l["cube"], l["status"]) for l in got] == [(list(l["cube"]), l["status"]) for l in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        if w["thr"] is None:
            assert g["thr"] is None, (what, i)
        else:
            np.testing.assert_array_equal(g["thr"], w["thr"], err_msg=f"{what}: thresholds of leaf {i}")


@pytest.mark.parametrize("name", list(C.SPLIT_CASES))
def test_split_cubes(gpu, name):
    """4. Leaves, statuses and thresholds are the reference splitter's.  On the power-law instance all
    16 items are dead after two decisions and stay frozen through the two levels that follow."""
    from alllsatisfiabilitysolver_amd import split_cubes

    c = C.split_case(name)
    leaves = split_cubes(c["n"], c["offs"], c["lits"], c["depth"], c["base"])
    print(name, [(l["status"], len(l["cube"])) for l in leaves])
    check_leaves(leaves, c["leaves"], name)
    if name == "PL":
        assert [(l["status"], len(l["cube"])) for l in leaves] == [("conflict", 2)] * 4


def test_solve_cubes_split(gpu):
    """5. On the 40-variable case: exactly solve_cubes_propagated fed the reference's live leaves; the
    winning words satisfy every clause; a satisfied leaf ends at its first pass."""
    from alllsatisfiabilitysolver_amd import solve_cubes_propagated, solve_cubes_split

    c = C.split_case("S40")
    leaves, (win, st, words) = solve_cubes_split(c["n"], c["offs"], c["lits"], c["depth"], max_iters=500)
    check_leaves(leaves, c["leaves"], "S40")
    live = [j for j, l in enumerate(c["leaves"]) if l["status"] != "conflict"]
    w2, st2, words2 = solve_cubes_propagated(c["n"], c["offs"], c["lits"], [list(c["leaves"][j]["cube"]) for j in live],
                                             max_iters=500)
    assert win == live[w2] and st == st2
    np.testing.assert_array_equal(words, words2)
    assert st["solved"] == 1 and satisfied(c["offs"], c["lits"], words)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    for d in leaves[win]["cube"]:
        assert bits[d >> 1] == 1 - (d & 1)
    # the four satisfied leaves end at their first pass, so the winner needs no more than that
    assert st["n_iterations"] == 1
    done = [list(l["cube"]) for l in c["leaves"] if l["status"] == "satisfied"]
    w3, st3, _ = solve_cubes_propagated(c["n"], c["offs"], c["lits"], done, max_iters=500)
    assert len(done) == 4 and w3 == 0 and st3["n_iterations"] == 1 and st3["solved"] == 1
