"""Failed-literal probing on the GPU (alll_probe_literals, Solver.probe,
failed_literal_reduce): the k_probe_* kernels against the numpy reference of probe_cases.py and
against the host form.  Every comparison is an equality; the facts the cases are there for are pinned
on the CPU in tests/test_probe_cases.py."""
import ctypes

import numpy as np
import pytest

import probe_cases as C
import prop_cases as P
from test_gpu_prop import GENERIC_CSR, NO_GRAPH, REFERENCE_RNG, STAT_KEYS
from test_probe_host import check

pytestmark = pytest.mark.gpu
u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def own_solver(c, seed=7, flags=0, thr="thr", **kw):
    from alllsatisfiabilitysolver_amd import Solver

    s = Solver(c["n"], c["offs"], c["lits"], seed=seed, flags=flags, **kw)
    if c[thr] is not None:
        s.set_thresholds(c[thr])
    return s


FLAG_CASES = [*C.CRAFTED, "C", "C_cap"]  # and B_fail's slab-edge slices: also under GENERIC_CSR and NO_GRAPH
CASE_FLAGS = [(name, 0) for name in C.ALL_CASES] + [(name, f) for name in FLAG_CASES for f in (GENERIC_CSR, NO_GRAPH)]
# the layout a case is there for: fixed width 3, ragged
LAYOUT = {"A4": 3, "G2": 3, "H2": 0}


@pytest.mark.parametrize("name,flags", CASE_FLAGS, ids=[f"{n}-{f}" for n, f in CASE_FLAGS])
def test_cases(gpu, name, flags):
    """1. Every case through Solver.probe: records and rows; the records alone are the same records.
    B_fail's 3422 probes are 54 slabs in one chunk here."""
    c = C.case(name)
    with own_solver(c, flags=flags) as s:
        if not flags and name in LAYOUT:
            assert s.layout() == LAYOUT[name]
        if flags & GENERIC_CSR:
            assert s.layout() == 0
        check(s.probe(c["probes"], c["max_rounds"], rows=True), c, name)
        assert s.probe(c["probes"][:3], c["max_rounds"]) == list(c["res"][:3])


@pytest.mark.parametrize("flags", [0, GENERIC_CSR, NO_GRAPH])
def test_slab_edges(gpu, flags):
    """1, 63, 64, 65 and 130 probes of B_fail, the first of them a failed literal."""
    for c in C.b_slices():
        with own_solver(c, flags=flags) as s:
            check(s.probe(c["probes"], rows=True), c, f"{len(c['probes'])} probes")


@pytest.mark.parametrize("slabs", [1, 5])
def test_chunks(gpu, slabs, monkeypatch):
    """B_fail's 54 slabs in chunks of one slab, and of five with a ragged last chunk of four."""
    monkeypatch.setenv("ALLL_PROBE_SLABS", str(slabs))
    c = C.case("B_fail")
    with own_solver(c) as s:
        check(s.probe(c["probes"], rows=True), c, f"chunks of {slabs}")
        got = s.probe(c["probes"])  # (without rows the scratch holds none)
        assert got == list(c["res"])


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_device_equals_host(gpu, name):
    """2. alll_probe_literals against alll_pinned_probe."""
    from alllsatisfiabilitysolver_amd import probe_literals

    c = C.case(name)
    host = probe_literals(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], c["max_rounds"], rows=True)
    with own_solver(c) as s:
        res, pm, pv = s.probe(c["probes"], c["max_rounds"], rows=True)
    assert res == host[0]
    np.testing.assert_array_equal(pm, host[1])
    np.testing.assert_array_equal(pv, host[2])


def snapshot(s, track):
    out = dict(words=s.assignment_words(), thr=s.thresholds(), stats={k: s.stats()[k] for k in STAT_KEYS})
    if out["stats"]["n_iterations"]:  # (the last pass's violated clauses and MIS)
        out.update(mask=s.violated_mask(), mis=s.mis())
    if track:
        b = s.best()
        out.update(best=(b["n_violated"], b["iteration"]), best_words=b["words"])
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("track", [False, True])
def test_the_call_changes_nothing(gpu, track):
    """3. On A4: before and after a probe call, after run(3), and with a probe call between two runs,
    against a context that never probed -- words, statistics, thresholds, violated mask, MIS, best record."""
    c = C.case("A4")
    with own_solver(c, 11, track_best=track) as s, own_solver(c, 11, track_best=track) as plain:
        before = snapshot(s, track)
        check(s.probe(c["probes"], rows=True), c, "before the first iteration")
        same(snapshot(s, track), before)
        same(snapshot(s, track), snapshot(plain, track))
        a, b = s.run(3), plain.run(3)
        assert {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        same(snapshot(s, track), snapshot(plain, track))
        check(s.probe(c["probes"], rows=True), c, "between two runs")  # a function of clauses and thresholds only
        same(snapshot(s, track), snapshot(plain, track))
        a, b = s.run(2), plain.run(2)
        assert a["n_iterations"] == 5 and {k: a[k] for k in STAT_KEYS} == {k: b[k] for k in STAT_KEYS}
        same(snapshot(s, track), snapshot(plain, track))


def test_refusals(gpu, native):
    """4. The refusals (nothing is written), no probes, and a context without thresholds.  (The refusal
    of a context that belongs to a group has no test: a group's member handles are not reachable
    through the public interface.)"""
    from alllsatisfiabilitysolver_amd import AlllError, Solver

    c = C.case("B_free")
    for kw in (dict(flags=REFERENCE_RNG), dict(stream_batch=64)):
        with Solver(c["n"], c["offs"], c["lits"], seed=3, **kw) as s:
            with pytest.raises(AlllError) as ei:
                s.probe(c["probes"])
            assert ei.value.code == native.ALLL_ERR_UNSUPPORTED and native.last_error()
    L = native.lib()
    nw = (c["n"] + 31) // 32
    with own_solver(c) as s:
        assert s.probe([]) == [] and s.probe([], rows=True)[1].shape == (0, nw)
        probes = np.array([0, 1, 2 * c["n"]], np.uint32)  # the last probe is past the variables
        res = (native.PropagateResult * 3)(*[native.PropagateResult(12345, 12345, 12345, 12345) for _ in range(3)])
        pm, pv = np.full((3, nw), 12345, np.uint32), np.full((3, nw), 12345, np.uint32)
        args = (pm.ctypes.data_as(u32p), pv.ctypes.data_as(u32p))
        assert L.alll_probe_literals(s._ctx, probes.ctypes.data_as(u32p), 3, 0, res, *args, nw) == native.ALLL_ERR_INVALID_ARG
        for bad in (nw - 1, nw + 1, 0):  # a wrong n_words
            assert L.alll_probe_literals(s._ctx, probes.ctypes.data_as(u32p), 2, 0, res, *args, bad) == native.ALLL_ERR_INVALID_ARG
        assert all(r.status == 12345 and r.rounds == 12345 for r in res) and (pm == 12345).all() and (pv == 12345).all()
        # (n_words is not looked at without rows)
        assert L.alll_probe_literals(s._ctx, probes.ctypes.data_as(u32p), 2, 0, res, None, None, 0) == native.ALLL_OK
        assert [res[i].as_dict() for i in range(2)] == list(c["res"][:2]) and res[2].status == 12345
        check(s.probe(c["probes"], rows=True), c, "no thresholds")  # every variable free


@pytest.mark.parametrize("name", list(C.REDUCE_CASES))
def test_reduce_on_the_device_equals_the_host(gpu, name):
    """5. failed_literal_reduce(device=True) against device=False and the restatement."""
    from alllsatisfiabilitysolver_amd import failed_literal_reduce

    n, offs, lits, thr, kw = C.reduce_input(name)
    dev = failed_literal_reduce(n, offs, lits, thr, device=True, **kw)
    host = failed_literal_reduce(n, offs, lits, thr, device=False, **kw)
    want = C.reduce_case(name)
    for other in (host, want):
        assert {k: v for k, v in dev.items() if k != "thr"} == {k: v for k, v in other.items() if k != "thr"}
        np.testing.assert_array_equal(dev["thr"], other["thr"])
