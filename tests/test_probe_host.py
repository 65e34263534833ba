"""Failed-literal probing on the host and the ABI of the feature: alll_pinned_probe
through the library against the numpy reference of probe_cases.py on every case, rows included, the
validation it shares with alll_pinned_scores and its own refusals (a refused call writes nothing), the
record's layout, the two entry points declared, exported and bound, the null refusals of the device
entry point (no device is touched), the host function once more through tests/cpp/probe_host_dump.cpp,
a stand-alone program built with a plain host compiler under the address and undefined-behaviour
sanitizers, and failed_literal_reduce(device=False) against its restatement and against brute force.
No GPU; no sanitizer on anything loaded into Python."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import probe_cases as C
import prop_cases as P
from conftest import ROOT
from test_batch_bias_host import CASES as CONFLICT_CASES, arrays

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG = 0, 1
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
NEW = ["alll_pinned_probe", "alll_probe_literals"]


def check(got, c, what=""):
    """Records and rows of a probe call against those of case c."""
    res, pm, pv = got
    bad = [(i, int(c["probes"][i]), r, w) for i, (r, w) in enumerate(zip(res, c["res"])) if r != w]
    assert len(res) == len(c["res"]) and not bad, (what, len(bad), bad[:5])
    np.testing.assert_array_equal(pm, c["pm"], err_msg=f"{what}: pm rows")
    np.testing.assert_array_equal(pv, c["pv"], err_msg=f"{what}: pv rows")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_matches_the_reference(native, name):
    from alllsatisfiabilitysolver_amd import probe_literals

    c = C.case(name)
    check(probe_literals(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], c["max_rounds"], rows=True), c, name)
    assert probe_literals(c["n"], c["offs"], c["lits"], c["thr"], c["probes"][:3], c["max_rounds"]) == list(c["res"][:3])


def test_slices_match_the_reference(native):
    from alllsatisfiabilitysolver_amd import probe_literals

    for c in C.b_slices():
        check(probe_literals(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], rows=True), c, len(c["probes"]))


def call(native, n, offs, lits, thr, probes, n_thr=None, max_rounds=0):
    prob = native.Problem(n, 0, offs.size - 1, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    probes = np.asarray(probes, np.uint32)
    res = (native.PropagateResult * max(1, probes.size))(*[native.PropagateResult(12345, 12345, 12345, 12345)
                                                           for _ in range(max(1, probes.size))])
    nw = (n + 31) // 32
    pm, pv = np.full((probes.size, nw), 12345, np.uint32), np.full((probes.size, nw), 12345, np.uint32)
    rc = native.lib().alll_pinned_probe(ctypes.byref(prob), None if thr is None else thr.ctypes.data_as(u32p),
                                        (0 if thr is None else thr.size) if n_thr is None else n_thr,
                                        probes.ctypes.data_as(u32p), probes.size, max_rounds, res, pm.ctypes.data_as(u32p),
                                        pv.ctypes.data_as(u32p))
    return rc, [r.as_dict() for r in res][:probes.size], pm, pv


UNTOUCHED = dict(conflict_clause=12345, n_forced=12345, rounds=12345, status=12345)


@pytest.mark.parametrize("case", CONFLICT_CASES, ids=[c[0] for c in CONFLICT_CASES])
def test_validation_is_that_of_pinned_propagate(native, case):
    n, offs, lits, thr, rc, _ = arrays(case)
    probes = np.arange(2 * n, dtype=np.uint32)
    got, res, pm, pv = call(native, n, offs, lits, thr, probes)
    assert got == rc
    if rc != OK:  # a refused call writes nothing
        assert native.last_error()
        assert all(r == UNTOUCHED for r in res) and (pm == 12345).all() and (pv == 12345).all()
        return
    want = C.probe(n, offs, lits, thr, probes)
    assert res == want[0]
    np.testing.assert_array_equal(pm, want[1])
    np.testing.assert_array_equal(pv, want[2])
    # a null thr: every variable a fair coin, whatever n says
    got, res, pm, pv = call(native, n, offs, lits, None, probes, n_thr=n + 5)
    want = C.probe(n, offs, lits, None, probes)
    assert got == OK and res == want[0]
    np.testing.assert_array_equal(pm, want[1])
    np.testing.assert_array_equal(pv, want[2])


def test_refusals_write_nothing(native):
    L = native.lib()
    c = C.case("fail_both")
    n, offs, lits, thr = c["n"], c["offs"].copy(), c["lits"].copy(), c["thr"].copy()
    # a literal of a variable that is not there, the last of the probes: checked before anything is written
    for bad in (2 * n, 2 * n + 1, 0xFFFFFFFF):
        got, res, pm, pv = call(native, n, offs, lits, thr, [0, 1, 2, bad])
        assert got == INVALID_ARG and native.last_error()
        assert all(r == UNTOUCHED for r in res) and (pm == 12345).all() and (pv == 12345).all()
    prob = native.Problem(n, 0, offs.size - 1, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = (native.PropagateResult * 4)()
    probes = np.arange(4, dtype=np.uint32)
    t, p = thr.ctypes.data_as(u32p), probes.ctypes.data_as(u32p)
    assert L.alll_pinned_probe(None, t, n, p, 4, 0, res, None, None) == INVALID_ARG
    assert L.alll_pinned_probe(ctypes.byref(prob), t, n, p, 4, 0, None, None, None) == INVALID_ARG
    assert L.alll_pinned_probe(ctypes.byref(prob), t, n, None, 4, 0, res, None, None) == INVALID_ARG
    assert L.alll_pinned_probe(ctypes.byref(prob), t, n - 1, p, 4, 0, res, None, None) == INVALID_ARG
    # no probes: fine, and nothing is written
    got, res, pm, pv = call(native, n, offs, lits, thr, [])
    assert got == OK and res == []
    assert L.alll_pinned_probe(ctypes.byref(prob), t, n, None, 0, 0, (native.PropagateResult * 1)(), None, None) == OK
    # the rows are optional, one by one
    probes = c["probes"]
    res = (native.PropagateResult * probes.size)()
    pm = np.zeros_like(c["pm"])
    assert L.alll_pinned_probe(ctypes.byref(prob), t, n, probes.ctypes.data_as(u32p), probes.size, 0, res,
                               pm.ctypes.data_as(u32p), None) == OK
    np.testing.assert_array_equal(pm, c["pm"])
    np.testing.assert_array_equal(thr, c["thr"])  # (the base thresholds are only read)


def test_max_rounds(native):
    """The cap is that of alll_pinned_propagate: every value from none to past the longest probe."""
    from alllsatisfiabilitysolver_amd import probe_literals

    c = C.case("E_all")
    for cap in (1, 2, 3):
        want = C.probe(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], cap)
        got = probe_literals(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], cap, rows=True)
        assert got[0] == want[0], cap
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
    assert P.ROUND_CAP in [r["status"] for r in C.probe(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], 1)[0]]


def test_record_layout_and_symbols(native, tmp_path):
    R = native.PropagateResult
    assert ctypes.sizeof(R) == 24
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "alll.h"\n'
                   "_Static_assert(sizeof(alll_propagate_result) == 24, \"size\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, n_forced) == 8, \"n_forced\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, rounds) == 16, \"rounds\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, status) == 20, \"status\");\n"
                   "_Static_assert(ALLL_ABI_VERSION == 1, \"the ABI version stays\");\n"
                   "int (*probe)(alll_ctx*, const uint32_t*, uint64_t, uint64_t, alll_propagate_result*, uint32_t*, uint32_t*,\n"
                   "             uint64_t) = alll_probe_literals;\n"
                   "int (*host)(const alll_problem*, const uint32_t*, uint64_t, const uint32_t*, uint64_t, uint64_t,\n"
                   "            alll_propagate_result*, uint32_t*, uint32_t*) = alll_pinned_probe;\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "alll.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(alll_\w+)\(", text, re.M))
    for name in NEW:
        assert name in declared and name in native.EXPORTED and name in native._SIGS
        assert getattr(native.lib(), name).argtypes == native._SIGS[name][0]
    assert declared == set(native.EXPORTED)


def test_null_handles_and_null_results(native):
    """The device entry point refuses null arguments before any device work."""
    L = native.lib()
    res = (native.PropagateResult * 2)()
    probes = np.zeros(2, np.uint32)
    p = probes.ctypes.data_as(u32p)
    assert L.alll_probe_literals(None, p, 2, 0, res, None, None, 0) == INVALID_ARG and native.last_error()
    fake = ctypes.c_void_p(8)  # (null results and null probes are refused before the handle is looked at)
    assert L.alll_probe_literals(fake, p, 2, 0, None, None, None, 0) == INVALID_ARG
    assert L.alll_probe_literals(fake, None, 2, 0, res, None, None, 0) == INVALID_ARG


def test_python_surface(native):
    from alllsatisfiabilitysolver_amd import (BatchSolver, GroupSolver, Solver, failed_literal_reduce, probe_literals,
                                              solve_cubes_split, split_cubes)

    assert list(inspect.signature(probe_literals).parameters) == ["n_vars", "offsets", "literals", "thr", "probes",
                                                                  "max_rounds", "rows"]
    assert list(inspect.signature(Solver.probe).parameters) == ["self", "probes", "max_rounds", "rows"]
    sig = inspect.signature(failed_literal_reduce)
    assert list(sig.parameters) == ["n_vars", "offsets", "literals", "thr", "n_candidates", "max_passes", "device"]
    assert [sig.parameters[k].default for k in ("thr", "n_candidates", "max_passes", "device")] == [None, 64, 0, True]
    assert not hasattr(BatchSolver, "probe") and not hasattr(GroupSolver, "probe")  # (no group or batch form)
    # the splitter keeps its signatures
    assert list(inspect.signature(split_cubes).parameters) == ["n_vars", "offsets", "literals", "depth", "base", "device"]
    assert list(inspect.signature(solve_cubes_split).parameters) == ["n_vars", "offsets", "literals", "depth", "base",
                                                                     "seeds", "max_iters"]


@pytest.mark.parametrize("name", list(C.REDUCE_CASES))
def test_reduce_matches_its_restatement(native, name):
    from alllsatisfiabilitysolver_amd import failed_literal_reduce

    n, offs, lits, thr, kw = C.reduce_input(name)
    before = None if thr is None else thr.copy()
    got, want = failed_literal_reduce(n, offs, lits, thr, device=False, **kw), C.reduce_case(name)
    assert {k: v for k, v in got.items() if k != "thr"} == {k: v for k, v in want.items() if k != "thr"}
    np.testing.assert_array_equal(got["thr"], want["thr"])
    if thr is not None:
        np.testing.assert_array_equal(thr, before)  # (the caller's thresholds are left alone)


@pytest.mark.parametrize("name", C.BRUTE_CASES)
def test_reduce_is_sound_by_brute_force(native, name):
    """The satisfying assignments consistent with the input thresholds are exactly those consistent
    with the returned ones; "conflict" means there are none."""
    from alllsatisfiabilitysolver_amd import failed_literal_reduce

    n, offs, lits, thr, kw = C.reduce_input(name)
    before = C.consistent_models(n, offs, lits, np.full(n, P.FAIR, np.uint32) if thr is None else thr)
    got = failed_literal_reduce(n, offs, lits, thr, device=False, **kw)
    if got["status"] == "conflict":
        assert not before
    else:
        assert C.consistent_models(n, offs, lits, got["thr"]) == before
        if got["status"] == "satisfied":
            assert before


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe_host")
    exe = str(d / "probe_host_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "probe_host_dump.cpp"), os.path.join(CSRC, "alll_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return [ln.split() for ln in r.stdout.splitlines()]

    return d, run


def pack(n, offs, lits, thr, probes, max_rounds=0):
    t = np.zeros(0, np.uint32) if thr is None else thr
    return (struct.pack("<II", n, offs.size - 1) + offs.astype("<u8").tobytes() + struct.pack("<I", lits.size) +
            lits.astype("<u4").tobytes() + struct.pack("<II", thr is not None, t.size) + t.astype("<u4").tobytes() +
            struct.pack("<II", max_rounds, len(probes)) + np.asarray(probes, "<u4").tobytes())


# (B_fail's 3422 probes run under the sanitizers as their slab-edge slice of 130)
SANITIZED = [n for n in C.ALL_CASES if n != "B_fail"] + ["B_fail_130"]


@pytest.mark.parametrize("name", SANITIZED)
def test_sanitized_matches_the_reference(dump, name):
    d, run = dump
    c = C.b_slices()[-1] if name == "B_fail_130" else C.case(name)
    i = SANITIZED.index(name)
    f, o = d / f"case{i}.bin", d / f"out{i}.bin"
    f.write_bytes(pack(c["n"], c["offs"], c["lits"], c["thr"], c["probes"], c["max_rounds"]))
    rows = run(f, o)
    assert rows[0] == ["rc", "0"]
    assert rows[1:] == [["res", str(r["status"]), str(r["rounds"]), str(r["n_forced"]), str(r["conflict_clause"])]
                        for r in c["res"]]
    out = np.frombuffer(o.read_bytes(), "<u4").reshape(2, *c["pm"].shape)
    np.testing.assert_array_equal(out[0], c["pm"])
    np.testing.assert_array_equal(out[1], c["pv"])


def test_sanitized_refusals_write_nothing(dump):
    d, run = dump
    c = C.case("fail_both")
    refused = [pack(c["n"], c["offs"], c["lits"], c["thr"], [0, 3, 6])]  # a probe past the variables
    for case in CONFLICT_CASES:
        n, offs, lits, thr, rc, _ = arrays(case)
        if rc != OK:
            refused.append(pack(n, offs, lits, thr, [0, 1]))
    for k, blob in enumerate(refused):
        f, o = d / f"refused{k}.bin", d / f"refused_out{k}.bin"
        f.write_bytes(blob)
        rows = run(f, o)
        assert rows[0][0] == "rc" and rows[0][1] != "0"
        assert all(r == ["res"] + ["12345"] * 4 for r in rows[1:]) and len(rows) > 1
        assert (np.frombuffer(o.read_bytes(), "<u4") == 12345).all()
