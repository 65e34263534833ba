"""Failed-literal probing of a whole group on the GPU (alll_group_probe_literals,
GroupSolver.probes): the group instantiations of the k_probe_* kernels against the numpy reference of
probe_cases.py per item (lookahead_cases.py builds the groups), against a Solver of every item's own
and against the host form.  Every comparison is an equality; the facts the cases are there for are
pinned on the CPU in tests/test_lookahead_cases.py."""
import ctypes

import numpy as np
import pytest

import lookahead_cases as L
import prop_cases as P
from test_gpu_prop import GENERIC_CSR, NO_GRAPH, REFERENCE_RNG, STAT_KEYS

pytestmark = pytest.mark.gpu
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def group_of(c, flags=0, seed0=1):
    from alllsatisfiabilitysolver_amd import GroupSolver

    g = GroupSolver(list(c["items"]), range(seed0, seed0 + len(c["items"])), flags=flags)
    for i, thr in enumerate(c["thrs"]):
        if thr is not None:
            g.set_thresholds(i, thr)
    return g


def records_only(c):
    return [list(w[0]) for w in c["want"]]


@pytest.mark.parametrize("reverse", [False, True])
def test_one_word_items_side_by_side(gpu, reverse):
    """1. 130 items of one assignment word: every wave of the apply and rows kernels holds two items, with
    their own probe counts and row bases -- counts that leak across the border show in n_forced."""
    c = L.one_word(reverse)
    with group_of(c) as g:
        L.check_group(g.probes(c["probes"], rows=True), c, f"one word, reverse={reverse}")
        assert g.probes(c["probes"]) == records_only(c)


@pytest.mark.parametrize("flags", [0, GENERIC_CSR, NO_GRAPH])
def test_ragged_layers(gpu, flags):
    """2. Items of 1, 63, 64, 65, 130, 0, 140, 140 and 130 probes: three layers with ragged ends, items
    of 2003 variables over several workgroups of the apply kernel, an item without thresholds."""
    c = L.ragged()
    with group_of(c, flags) as g:
        if flags & GENERIC_CSR:
            assert g.layout() == 0
        L.check_group(g.probes(c["probes"], rows=True), c, f"ragged, flags={flags}")
        assert g.probes(c["probes"]) == records_only(c)  # (without rows the scratch holds none)


@pytest.mark.parametrize("layers", [1, 2])
def test_ragged_layers_in_chunks(gpu, layers, monkeypatch):
    """Chunks of one layer, and of two with a ragged last chunk of one."""
    monkeypatch.setenv("ALLL_PROBE_SLABS", str(layers))
    c = L.ragged()
    with group_of(c) as g:
        L.check_group(g.probes(c["probes"], rows=True), c, f"chunks of {layers}")
        assert g.probes(c["probes"]) == records_only(c)


def test_max_rounds_is_the_calls(gpu):
    """3. Chain C under a cap of 100 next to a crafted item: ROUND_CAP, FIXPOINT at the cap and before it
    per item."""
    c = L.capped()
    with group_of(c) as g:
        L.check_group(g.probes(c["probes"], c["max_rounds"], rows=True), c, "capped")
        statuses = [r["status"] for r in g.probes(c["probes"], c["max_rounds"])[0]]
        assert P.ROUND_CAP in statuses and P.FIXPOINT in statuses


def test_group_equals_own_context_equals_host(gpu):
    """4. Every item of the ragged group against Solver.probe on a Solver of its own and against
    probe_literals on the host."""
    from alllsatisfiabilitysolver_amd import Solver, probe_literals

    c = L.ragged()
    with group_of(c) as g:
        got = g.probes(c["probes"], rows=True)
    for i, ((n, offs, lits), thr, probes) in enumerate(zip(c["items"], c["thrs"], c["probes"])):
        with Solver(n, offs, lits, seed=7) as s:
            if thr is not None:
                s.set_thresholds(thr)
            own = s.probe(probes, rows=True)
        host = probe_literals(n, offs, lits, thr, probes, rows=True)
        for other in (own, host):
            assert got[i][0] == other[0], i
            np.testing.assert_array_equal(got[i][1], other[1])
            np.testing.assert_array_equal(got[i][2], other[2])


def snapshot(g, n_items, track):
    out = []
    for i in range(n_items):
        s = dict(words=g.assignment_words(i), stats={k: g.stats(i)[k] for k in STAT_KEYS})
        try:
            s["thr"] = g.thresholds(i)
        except Exception:  # (an item without thresholds has none to read)
            s["thr"] = None
        if track:
            b = g.best(i)
            s.update(best=(b["n_violated"], b["iteration"]), best_words=b["words"])
        out.append(s)
    return out


def same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            if isinstance(x[k], np.ndarray):
                np.testing.assert_array_equal(x[k], y[k], err_msg=f"item {i}: {k}")
            else:
                assert x[k] == y[k], (i, k)


@pytest.mark.parametrize("track", [False, True])
def test_the_call_changes_nothing(gpu, track):
    """5. Before and after a probe call, after run(3), and with a call between two runs, against a group
    that never probed: every item's words, thresholds, statistics and best record."""
    c = L.one_word()
    n = len(c["items"])
    with group_of(c) as g, group_of(c) as plain:
        if track:
            g.track_best()
            plain.track_best()
        before = snapshot(g, n, track)
        L.check_group(g.probes(c["probes"], rows=True), c, "before the first iteration")
        same(snapshot(g, n, track), before)
        same(snapshot(g, n, track), snapshot(plain, n, track))
        a, b = g.run(3), plain.run(3)
        assert [{k: r[k] for k in STAT_KEYS} for r in a] == [{k: r[k] for k in STAT_KEYS} for r in b]
        same(snapshot(g, n, track), snapshot(plain, n, track))
        L.check_group(g.probes(c["probes"], rows=True), c, "between two runs")  # a function of clauses and thresholds only
        same(snapshot(g, n, track), snapshot(plain, n, track))
        a, b = g.run(2), plain.run(2)
        assert [{k: r[k] for k in STAT_KEYS} for r in a] == [{k: r[k] for k in STAT_KEYS} for r in b]
        same(snapshot(g, n, track), snapshot(plain, n, track))


def test_refusals(gpu, native):
    """6. A refused call writes nothing; no probes at all is ALLL_OK.  (No group with an unsupported option
    is reachable: the group's creation refuses every option its context's thresholds would refuse.)"""
    from alllsatisfiabilitysolver_amd import AlllError, GroupSolver

    c = L.one_word()
    with pytest.raises(AlllError) as ei:
        GroupSolver(list(c["items"][:2]), [1, 2], flags=REFERENCE_RNG)
    assert ei.value.code == native.ALLL_ERR_UNSUPPORTED
    lib = native.lib()
    items = [c["items"][0], c["items"][1]]  # 2 and 3 variables: a word each
    with GroupSolver(items, [1, 2]) as g:
        fn = lib.alll_group_probe_literals
        res = (native.PropagateResult * 4)(*[native.PropagateResult(12345, 12345, 12345, 12345) for _ in range(4)])
        pm, pv = np.full(4, 12345, np.uint32), np.full(4, 12345, np.uint32)
        rows = (pm.ctypes.data_as(u32p), pv.ctypes.data_as(u32p))
        offs = np.array([0, 2, 4], np.uint64)
        o = offs.ctypes.data_as(u64p)
        # literal 4 is past item 0's two variables and a valid literal of the union
        bad = np.array([0, 4, 0, 5], np.uint32)
        assert fn(g._h, bad.ctypes.data_as(u32p), o, 0, res, *rows, 4) == native.ALLL_ERR_INVALID_ARG and native.last_error()
        good = np.array([0, 3, 0, 5], np.uint32)
        p = good.ctypes.data_as(u32p)
        for n_row_words in (3, 5, 0):
            assert fn(g._h, p, o, 0, res, *rows, n_row_words) == native.ALLL_ERR_INVALID_ARG
        assert fn(g._h, p, o, 0, res, rows[0], None, 4) == native.ALLL_ERR_INVALID_ARG  # the rows go together
        assert fn(g._h, None, o, 0, res, *rows, 4) == native.ALLL_ERR_INVALID_ARG
        for bad_offs in ([1, 2, 4], [0, 3, 2]):
            b = np.array(bad_offs, np.uint64)
            assert fn(g._h, p, b.ctypes.data_as(u64p), 0, res, None, None, 0) == native.ALLL_ERR_INVALID_ARG
        assert all(r.status == 12345 and r.rounds == 12345 for r in res) and (pm == 12345).all() and (pv == 12345).all()
        # no probes: fine, nothing written, null probes allowed
        zero = np.zeros(3, np.uint64)
        assert fn(g._h, None, zero.ctypes.data_as(u64p), 0, res, *rows, 0) == native.ALLL_OK
        assert all(r.status == 12345 for r in res) and (pm == 12345).all()
        assert g.probes([[], []]) == [[], []]
        empty = g.probes([[], []], rows=True)
        assert empty[0][1].shape == (0, 1) and empty[1][2].shape == (0, 1)
        # (n_row_words is not looked at without rows) and the good call is the reference's
        assert fn(g._h, p, o, 0, res, None, None, 77) == native.ALLL_OK
        want = [P_probe(items[0], [0, 3]), P_probe(items[1], [0, 5])]
        assert [res[i].as_dict() for i in range(4)] == want[0] + want[1]
        with pytest.raises(ValueError):
            g.probes([[0]])


def P_probe(item, probes):
    import probe_cases as C

    return C.probe(*item, None, probes)[0]


def test_a_swarm(gpu):
    """7. A thousand items, three probes each where the item has a free variable: past one workgroup of
    items in every kernel, clauseless items and items without thresholds among them."""
    c = L.swarm()
    with group_of(c) as g:
        L.check_group(g.probes(c["probes"], rows=True), c, "swarm")
