"""Split scores on the host and the ABI of the feature: alll_pinned_scores through
the library against the numpy reference of split_cases.py on every case and on the items of the
many-item propagation cases, the validation it shares with alll_pinned_conflict (a refused call
writes nothing), the record's layout in C and in the binding, the three entry points declared,
exported and bound, the null refusals of the device entry points (no device is touched), and the host
function once more through tests/cpp/split_host_dump.cpp, a stand-alone program built with a plain
host compiler under the address and undefined-behaviour sanitizers.  No GPU; no sanitizer on anything
loaded into Python."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import prop_cases as P
import split_cases as C
from conftest import ROOT
from test_batch_bias_host import CASES as CONFLICT_CASES, arrays

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG = 0, 1
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
NEW = ["alll_pinned_scores", "alll_var_scores", "alll_group_var_scores"]


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_matches_the_reference(native, name):
    from alllsatisfiabilitysolver_amd import var_scores

    c = C.case(name)
    S, rec = var_scores(c["n"], c["offs"], c["lits"], c["thr"])
    assert rec == c["rec"]
    np.testing.assert_array_equal(S, c["S"])


@pytest.mark.parametrize("name", ["ladder", "prop_swarm", "mixed_group"])
def test_many_items_match_the_reference(native, name):
    """The items of the many-item cases under their propagated thresholds (None: no thresholds),
    clauseless items, items in conflict and the star's hub among them."""
    from alllsatisfiabilitysolver_amd import var_scores

    c = {"ladder": P.ladder, "prop_swarm": P.prop_swarm, "mixed_group": P.mixed_group}[name]()
    for i, ((n, offs, lits), thr, (S, rec)) in enumerate(zip(c["items"], c["outs"], C.many_scores(c, c["outs"]))):
        got_S, got = var_scores(n, offs, lits, thr)
        assert got == rec, (name, i)
        np.testing.assert_array_equal(got_S, S, err_msg=f"{name} item {i}")


def call(native, n, offs, lits, thr, n_thr=None):
    prob = native.Problem(n, 0, offs.size - 1, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.SplitResult(12345, 12345, 12345, 12345, 12345)
    S = np.full(2 * n, 12345, np.uint64)
    rc = native.lib().alll_pinned_scores(ctypes.byref(prob), None if thr is None else thr.ctypes.data_as(u32p),
                                         (0 if thr is None else thr.size) if n_thr is None else n_thr,
                                         S.ctypes.data_as(u64p), ctypes.byref(res))
    return rc, S, res


@pytest.mark.parametrize("case", CONFLICT_CASES, ids=[c[0] for c in CONFLICT_CASES])
def test_validation_is_that_of_pinned_conflict(native, case):
    n, offs, lits, thr, rc, _ = arrays(case)
    got, S, res = call(native, n, offs, lits, thr)
    assert got == rc
    if rc != OK:  # a refused call writes nothing
        assert native.last_error()
        assert (S == 12345).all()
        assert (res.score_pos, res.score_neg, res.n_open, res.var, res.pad) == (12345,) * 5
        return
    want_S, want = C.scores(n, offs, lits, thr)
    assert dict(res.as_dict()) == want and res.pad == 0
    np.testing.assert_array_equal(S, want_S)
    # a null thr: every variable free, whatever n says; the instance is validated all the same
    got, S, res = call(native, n, offs, lits, None, n_thr=n + 5)
    want_S, want = C.scores(n, offs, lits, None)
    assert got == OK and res.as_dict() == want
    np.testing.assert_array_equal(S, want_S)


def test_null_arguments_and_bad_instances_without_thresholds(native):
    L = native.lib()
    c = C.case("dead")
    offs, lits, thr = c["offs"].copy(), c["lits"].copy(), c["thr"].copy()
    prob = native.Problem(3, 0, 3, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.SplitResult()
    t = thr.ctypes.data_as(u32p)
    assert L.alll_pinned_scores(None, t, 3, None, ctypes.byref(res)) == INVALID_ARG and native.last_error()
    assert L.alll_pinned_scores(ctypes.byref(prob), t, 3, None, None) == INVALID_ARG
    for bad in (native.Problem(3, 0, 3, None, lits.ctypes.data_as(u32p)), native.Problem(3, 0, 3, offs.ctypes.data_as(u64p), None)):
        assert L.alll_pinned_scores(ctypes.byref(bad), None, 0, None, ctypes.byref(res)) == INVALID_ARG
    for case in CONFLICT_CASES:
        n, o, l, _, rc, _ = arrays(case)
        if rc not in (OK, INVALID_ARG):  # (the refusals that concern the instance, not the thresholds)
            got, S, r = call(native, n, o, l, None)
            assert got == rc and (S == 12345).all() and r.var == 12345
    # scores == NULL: the record alone
    assert L.alll_pinned_scores(ctypes.byref(prob), t, 3, None, ctypes.byref(res)) == OK
    assert res.as_dict() == c["rec"]


def test_record_layout(native, tmp_path):
    R = native.SplitResult
    assert ctypes.sizeof(R) == 32
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("score_pos", 0), ("score_neg", 8), ("n_open", 16),
                                                                  ("var", 24), ("pad", 28)]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "alll.h"\n'
                   "_Static_assert(sizeof(alll_split_result) == 32, \"size\");\n"
                   "_Static_assert(offsetof(alll_split_result, score_neg) == 8, \"score_neg\");\n"
                   "_Static_assert(offsetof(alll_split_result, n_open) == 16, \"n_open\");\n"
                   "_Static_assert(offsetof(alll_split_result, var) == 24, \"var\");\n"
                   "_Static_assert(offsetof(alll_split_result, pad) == 28, \"pad\");\n"
                   "_Static_assert(ALLL_ABI_VERSION == 1, \"the ABI version stays\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_are_declared_exported_and_bound(native):
    text = open(os.path.join(ROOT, "include", "alll.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(alll_\w+)\(", text, re.M))
    for name in NEW:
        assert name in declared and name in native.EXPORTED and name in native._SIGS
        assert getattr(native.lib(), name).argtypes == native._SIGS[name][0]
    assert declared == set(native.EXPORTED)


def test_null_handles_and_null_results(native):
    """The device entry points refuse null arguments before any device work."""
    L = native.lib()
    res = native.SplitResult()
    S = np.zeros(4, np.uint64)
    assert L.alll_var_scores(None, S.ctypes.data_as(u64p), 4, ctypes.byref(res)) == INVALID_ARG and native.last_error()
    assert L.alll_group_var_scores(None, ctypes.byref(res), S.ctypes.data_as(u64p), 4) == INVALID_ARG
    # (a null result is refused before the handle is looked at: any non-null value will do)
    fake = ctypes.c_void_p(8)
    assert L.alll_var_scores(fake, None, 0, None) == INVALID_ARG
    assert L.alll_group_var_scores(fake, None, None, 0) == INVALID_ARG


def test_python_surface(native):
    from alllsatisfiabilitysolver_amd import (BatchSolver, GroupSolver, Solver, solve_cubes, solve_cubes_propagated,
                                              solve_cubes_split, split_cubes, var_scores)

    assert list(inspect.signature(var_scores).parameters) == ["n_vars", "offsets", "literals", "thr"]
    assert list(inspect.signature(split_cubes).parameters) == ["n_vars", "offsets", "literals", "depth", "base", "device"]
    assert list(inspect.signature(solve_cubes_split).parameters) == ["n_vars", "offsets", "literals", "depth", "base",
                                                                     "seeds", "max_iters"]
    assert inspect.signature(Solver.var_scores).parameters["with_scores"].default is True
    assert inspect.signature(GroupSolver.var_scores).parameters["with_scores"].default is False
    assert not hasattr(BatchSolver, "var_scores")  # (no batch form)
    want = ["n_vars", "offsets", "literals", "cubes", "seeds", "max_iters"]  # the portfolios keep their signatures
    assert list(inspect.signature(solve_cubes).parameters) == want
    assert list(inspect.signature(solve_cubes_propagated).parameters) == want
    offs, lits = np.array([0, 2], np.uint64), np.array([0, 2], np.uint32)
    for depth in (0, 11):  # refused before a device is touched
        with pytest.raises(ValueError):
            split_cubes(2, offs, lits, depth)
    S, rec = var_scores(2, offs, lits)
    assert S.tolist() == [16384, 0, 16384, 0] and rec == dict(var=0, score_pos=16384, score_neg=0, n_open=1)
    S, rec = var_scores(3, [0], [])  # no clause: nothing to split on
    assert not S.any() and rec == dict(var=3, score_pos=0, score_neg=0, n_open=0)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("split_host")
    exe = str(d / "split_host_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "split_host_dump.cpp"), os.path.join(CSRC, "alll_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return [ln.split() for ln in r.stdout.splitlines()]

    return d, run


def pack(n, offs, lits, thr):
    t = np.zeros(0, np.uint32) if thr is None else thr
    return (struct.pack("<II", n, offs.size - 1) + offs.astype("<u8").tobytes() + struct.pack("<I", lits.size) +
            lits.astype("<u4").tobytes() + struct.pack("<II", thr is not None, t.size) + t.astype("<u4").tobytes())


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_sanitized_matches_the_reference(dump, name):
    d, run = dump
    c = C.case(name)
    i = C.ALL_CASES.index(name)
    f, o = d / f"case{i}.bin", d / f"out{i}.bin"
    f.write_bytes(pack(c["n"], c["offs"], c["lits"], c["thr"]))
    rows = run(f, o)
    r = c["rec"]
    assert rows == [["rc", "0"], ["res", str(r["var"]), str(r["score_pos"]), str(r["score_neg"]), str(r["n_open"]), "0"]]
    np.testing.assert_array_equal(np.frombuffer(o.read_bytes(), "<u8"), c["S"])


@pytest.mark.parametrize("case", [c for c in CONFLICT_CASES if c[5] != OK], ids=lambda c: c[0])
def test_sanitized_refusals_write_nothing(dump, case):
    d, run = dump
    n, offs, lits, thr, rc, _ = arrays(case)
    f, o = d / "refused.bin", d / "refused_out.bin"
    f.write_bytes(pack(n, offs, lits, thr))
    rows = run(f, o)
    assert rows == [["rc", str(rc)], ["res"] + ["12345"] * 5]
    assert (np.frombuffer(o.read_bytes(), "<u8") == 12345).all()
