"""The residual formula on the GPU (alll_residual and its group form,
solve_cubes_residual): the k_resid_* kernels against the numpy restatement of resid_cases.py.  Every
comparison is an equality; the facts the cases are there for are pinned on the CPU in
tests/test_resid_cases.py."""
import numpy as np
import pytest

import prop_cases as P
import resid_cases as C
import split_cases as S
from test_gpu_prop import ATOMIC_CLAIMS, GENERIC_CSR, NO_GRAPH, REFERENCE_RNG, STAT_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def own_solver(c, seed=7, flags=0, **kw):
    from alllsatisfiabilitysolver_amd import Solver

    s = Solver(c["n"], c["offs"], c["lits"], seed=seed, flags=flags, **kw)
    if c["thr"] is not None:
        s.set_thresholds(c["thr"])
    return s


CASE_FLAGS = [(name, 0) for name in C.ALL_CASES] + [(name, f) for name in C.FLAG_CASES
                                                   for f in (GENERIC_CSR, NO_GRAPH, ATOMIC_CLAIMS)]
# the layout a case is there for: fixed width 3, ragged
LAYOUT = {"A4p": 3, "PL": 3, "Z": 3, "R": 0}


@pytest.mark.parametrize("name,flags", CASE_FLAGS, ids=[f"{n}-{f}" for n, f in CASE_FLAGS])
def test_cases(gpu, name, flags):
    """1. Every case through Solver.residual: the record and all five arrays; the record alone is the
    same record."""
    c = C.case(name)
    with own_solver(c, flags=flags) as s:
        if not flags and name in LAYOUT:
            assert s.layout() == LAYOUT[name]
        if not flags and name == "R":
            assert s.eval_kernel() == "k_eval_ragged"
        if flags & GENERIC_CSR:
            assert s.layout() == 0
        got = s.residual()
        print(name, flags, C.counts(got))
        assert C.same(got, c["res"]) is None
        assert set(got) == set(c["res"])
        assert s.residual(with_arrays=False) == C.counts(c["res"])


@pytest.mark.parametrize("track", [False, True])
def test_the_call_changes_nothing(gpu, track):
    """2. On A4p: thresholds, residual, run(5) against the same without the call -- words, violated
    mask, MIS, statistics (and the best record); residual after run(3) is the call before it."""
    c = C.case("A4p")
    with own_solver(c, 11, track_best=track) as s, own_solver(c, 11, track_best=track) as plain:
        assert C.same(s.residual(), c["res"]) is None
        np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words())
        np.testing.assert_array_equal(s.thresholds(), c["thr"])
        a, b = s.run(3), plain.run(3)
        assert {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        assert C.same(s.residual(), c["res"]) is None  # mid-run: a function of clauses and thresholds only
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

    c = C.case("B4p")
    for kw in (dict(flags=REFERENCE_RNG), dict(stream_batch=64)):
        with Solver(c["n"], c["offs"], c["lits"], seed=3, **kw) as s:
            with pytest.raises(AlllError) as ei:
                s.residual()
            assert ei.value.code == native.ALLL_ERR_UNSUPPORTED and native.last_error()


def check_items(got, want, what):
    assert len(got) == len(want)
    bad = [(i, d) for i, d in ((i, C.same(g, w)) for i, (g, w) in enumerate(zip(got, want))) if d]
    assert not bad, (what, len(bad), bad[:5])


@pytest.mark.parametrize("name", ["mixed_group", "ladder", "prop_swarm"])
def test_groups(gpu, name):
    """3. 199, 130 and 1000 items in one group: before the propagation under the items' own thresholds,
    after it under the propagated ones -- tiles of words and of clauses that span many items,
    clauseless items, items without thresholds, items in conflict (their thresholds are those of the
    failing round's start), the star's hub."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = {"mixed_group": P.mixed_group, "ladder": P.ladder, "prop_swarm": P.prop_swarm}[name]()
    with GroupSolver(list(c["items"]), list(c["seeds"])) as g:
        for i, thr in enumerate(c["thrs"]):
            if thr is not None:
                g.set_thresholds(i, thr)
        check_items(g.residuals(), C.many_residuals(c, c["thrs"]), f"{name}, before")
        res = g.propagate_pins()
        assert [r["status"] for r in res] == [r["status"] for r in c["ress"]]
        want = C.many_residuals(c, c["outs"])
        check_items(g.residuals(), want, name)
        assert g.residuals(with_arrays=False) == [C.counts(w) for w in want]


def test_group_without_thresholds(gpu):
    """A group in which no item has thresholds (the union has no threshold array), and one of a single item."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    cases = [C.case(name) for name in ("B4p", "far", "W", "taut", "R", "null_thr")]
    want = [C.residual(c["n"], c["offs"], c["lits"], None) for c in cases]
    with GroupSolver([(c["n"], c["offs"], c["lits"]) for c in cases], [1, 2, 3, 4, 5, 6]) as g:
        check_items(g.residuals(), want, "no thresholds")
        g.run(2)  # an item's being solved or ended does not matter
        check_items(g.residuals(), want, "no thresholds, after run(2)")
    c = C.case("B4p")
    with GroupSolver([(c["n"], c["offs"], c["lits"])], [9]) as g:
        g.set_thresholds(0, c["thr"])
        check_items(g.residuals(), [c["res"]], "one item")


def test_a_solver_of_the_device_residual(gpu):
    """4. A Solver built from the device residual of B4p under thr_res runs the trajectory of a Solver
    built from the restatement's residual: words after 5 iterations, and statistics."""
    from alllsatisfiabilitysolver_amd import Solver

    c = C.case("B4p")
    with own_solver(c) as s:
        got = s.residual()
    want = c["res"]
    runs = []
    for r in (got, want):
        with Solver(r["n_vars"], r["offsets"], r["literals"], seed=21) as t:
            t.set_thresholds(r["thr"])
            st = t.run(5)
            runs.append(({k: st[k] for k in STAT_KEYS}, t.assignment_words()))
    assert runs[0][0] == runs[1][0] and runs[0][0]["n_iterations"] == 5
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


def reference_winner(n, offs, lits, cubes, seeds, max_iters):
    """solve_cubes_residual from the restatement: a BatchSolver of the reference residuals."""
    from alllsatisfiabilitysolver_amd import BatchSolver, batch_fits

    ref = C.reference_portfolio(n, offs, lits, cubes)
    assert ref and all(batch_fits(r["n_vars"], r["n_clauses"], r["n_literals"]) for _, _, r in ref)
    with BatchSolver([(r["n_vars"], r["offsets"], r["literals"]) for _, _, r in ref], [seeds[i] for i, _, _ in ref],
                     max_iters=max_iters) as b:
        for j, (_, _, r) in enumerate(ref):
            b.set_thresholds(j, r["thr"])
        st = b.solve(first_solved=True)
        solved = [j for j, x in enumerate(st) if x["solved"]]
        assert solved
        best = min(solved, key=lambda j: (st[j]["n_iterations"], j))
        i, thr, r = ref[best]
        return i, st[best], C.lift(n, thr, r["var_map"], b.assignment_words(best))


def check_portfolio(monkeypatch, n, offs, lits, cubes, max_iters):
    """-> (winner, stats, the solver classes solve_cubes_residual built, in order, with their item sizes)."""
    from alllsatisfiabilitysolver_amd import solve_cubes_residual, solver

    built = []
    for cls in (solver.BatchSolver, solver.GroupSolver):
        def init(self, problems, *a, _cls=cls, _init=cls.__init__, **kw):
            problems = list(problems)
            built.append((_cls.__name__, max(p[0] for p in problems)))
            _init(self, problems, *a, **kw)

        monkeypatch.setattr(cls, "__init__", init)
    seeds = list(range(1, len(cubes) + 1))
    win, st, words = solve_cubes_residual(n, offs, lits, cubes, max_iters=max_iters)
    monkeypatch.undo()
    w2, st2, words2 = reference_winner(n, offs, lits, cubes, seeds, max_iters)
    print(win, st)
    assert win == w2 and st == st2
    np.testing.assert_array_equal(words, words2)
    assert st["solved"] == 1 and C.satisfied(offs, lits, words)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    for d in cubes[win]:
        assert bits[d >> 1] == 1 - (d & 1)
    return win, st, built


def test_solve_cubes_residual_takes_the_batch_path(gpu, monkeypatch):
    """5. W does not fit a batch item (30011 variables); each of its residuals does (at most 6596
    variables and 2500 clauses), so the residuals run in a BatchSolver: the result is that of a
    BatchSolver built from the restatement's residuals, lifted; the words satisfy W and obey the cube."""
    from alllsatisfiabilitysolver_amd import batch_fits

    n, offs, lits = C.instance("W")
    assert not batch_fits(n, offs.size - 1, lits.size)
    _, _, built = check_portfolio(monkeypatch, n, offs, lits, C.w_cubes(), 2000)
    # the group that propagates and compacts holds W itself; the solver of the residuals is a batch
    assert [b[0] for b in built] == ["GroupSolver", "BatchSolver"] and built[0][1] == n and built[1][1] <= 6596


def test_solve_cubes_residual_on_split_leaves(gpu, monkeypatch):
    """The same on the 40-variable case with the open leaves of the reference splitter as cubes."""
    c = S.split_case("S40")
    cubes = [list(l["cube"]) for l in c["leaves"] if l["status"] == "open"]
    assert len(cubes) == 39
    _, _, built = check_portfolio(monkeypatch, c["n"], c["offs"], c["lits"], cubes, 500)
    assert [b[0] for b in built] == ["GroupSolver", "BatchSolver"]


def test_a_cube_whose_residual_has_no_clause(gpu):
    """A satisfied leaf's residual is 0 / 0 / 0: the planners accept the empty item, it is solved at
    its first pass, and the lift is the pins alone."""
    from alllsatisfiabilitysolver_amd import solve_cubes_residual

    c = S.split_case("S40")
    done = [l for l in c["leaves"] if l["status"] == "satisfied"]
    opened = [l for l in c["leaves"] if l["status"] == "open"]
    cubes = [list(opened[0]["cube"]), list(done[0]["cube"])]
    assert C.counts(C.residual(c["n"], c["offs"], c["lits"], done[0]["thr"]))["n_clauses"] == 0
    win, st, words = solve_cubes_residual(c["n"], c["offs"], c["lits"], cubes, max_iters=500)
    print(win, st)
    assert win == 1 and st["solved"] == 1 and st["n_iterations"] == 1 and C.satisfied(c["offs"], c["lits"], words)
    np.testing.assert_array_equal(words, C.lift(c["n"], done[0]["thr"], [], np.zeros(0, np.uint32)))
