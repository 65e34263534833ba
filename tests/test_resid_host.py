"""The residual formula on the host and the ABI of the feature: alll_pinned_residual
through the library against the numpy restatement of resid_cases.py on every case and on the items of
the many-item propagation cases, the validation it shares with alll_pinned_conflict (a refused call
writes nothing), the record's layout in C and in the binding, the three entry points declared,
exported and bound, the null refusals of the device entry points (no device is touched), the lift, and
the host function once more through tests/cpp/resid_host_dump.cpp, a stand-alone program built with a
plain host compiler under the address and undefined-behaviour sanitizers.  No GPU; no sanitizer on
anything loaded into Python."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import prop_cases as P
import resid_cases as C
from conftest import ROOT
from test_batch_bias_host import CASES as CONFLICT_CASES, arrays

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG = 0, 1
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
NEW = ["alll_pinned_residual", "alll_residual", "alll_group_residual"]
FIELDS = ("n_clauses", "n_literals", "n_falsified", "first_falsified", "n_vars", "pad")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_matches_the_reference(native, name):
    from alllsatisfiabilitysolver_amd import residual_instance

    c = C.case(name)
    got = residual_instance(c["n"], c["offs"], c["lits"], c["thr"])
    assert C.same(got, c["res"]) is None
    assert set(got) == set(c["res"])


@pytest.mark.parametrize("name", ["ladder", "prop_swarm", "mixed_group"])
def test_many_items_match_the_reference(native, name):
    """The items of the many-item cases under their propagated thresholds (None: no thresholds),
    clauseless items, items in conflict and the star's hub among them."""
    from alllsatisfiabilitysolver_amd import residual_instance

    c = {"ladder": P.ladder, "prop_swarm": P.prop_swarm, "mixed_group": P.mixed_group}[name]()
    for i, ((n, offs, lits), thr, want) in enumerate(zip(c["items"], c["outs"], C.many_residuals(c, c["outs"]))):
        assert C.same(residual_instance(n, offs, lits, thr), want) is None, (name, i)


def call(native, n, offs, lits, thr, n_thr=None):
    """The raw call with every output at its capacity and filled with 12345."""
    m = offs.size - 1
    prob = native.Problem(n, 0, m, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.ResidualResult(*[12345] * 6)
    out = dict(offsets=np.full(m + 1, 12345, np.uint64), literals=np.full(lits.size, 12345, np.uint32),
               var_map=np.full(n, 12345, np.uint32), clause_map=np.full(m, 12345, np.uint64),
               thr=np.full(n, 12345, np.uint32))
    rc = native.lib().alll_pinned_residual(ctypes.byref(prob), None if thr is None else thr.ctypes.data_as(u32p),
                                           (0 if thr is None else thr.size) if n_thr is None else n_thr,
                                           ctypes.byref(res), out["offsets"].ctypes.data_as(u64p),
                                           out["literals"].ctypes.data_as(u32p), out["var_map"].ctypes.data_as(u32p),
                                           out["clause_map"].ctypes.data_as(u64p), out["thr"].ctypes.data_as(u32p))
    return rc, out, res


def untouched(out, res):
    return all((a == 12345).all() for a in out.values()) and all(getattr(res, k) == 12345 for k in FIELDS)


def check_prefixes(out, res, want):
    """The used prefixes hold the residual; nothing behind them is written."""
    assert res.as_dict() == C.counts(want)
    assert res.pad == 0
    for k, used in (("offsets", want["n_clauses"] + 1), ("literals", want["n_literals"]), ("var_map", want["n_vars"]),
                    ("clause_map", want["n_clauses"]), ("thr", want["n_vars"])):
        np.testing.assert_array_equal(out[k][:used], want[k], err_msg=k)
        assert (out[k][used:] == 12345).all(), k


@pytest.mark.parametrize("case", CONFLICT_CASES, ids=[c[0] for c in CONFLICT_CASES])
def test_validation_is_that_of_pinned_conflict(native, case):
    n, offs, lits, thr, rc, _ = arrays(case)
    got, out, res = call(native, n, offs, lits, thr)
    assert got == rc
    if rc != OK:  # a refused call writes nothing
        assert native.last_error()
        assert untouched(out, res)
        return
    check_prefixes(out, res, C.residual(n, offs, lits, thr))
    # a null thr: every variable free, whatever n says; the instance is validated all the same
    got, out, res = call(native, n, offs, lits, None, n_thr=n + 5)
    assert got == OK
    check_prefixes(out, res, C.residual(n, offs, lits, None))


def test_null_arguments_and_bad_instances_without_thresholds(native):
    L = native.lib()
    c = C.case("dead")
    offs, lits, thr = c["offs"].copy(), c["lits"].copy(), c["thr"].copy()
    m = offs.size - 1
    prob = native.Problem(c["n"], 0, m, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.ResidualResult()
    t = thr.ctypes.data_as(u32p)
    none = (None,) * 5
    assert L.alll_pinned_residual(None, t, c["n"], ctypes.byref(res), *none) == INVALID_ARG and native.last_error()
    assert L.alll_pinned_residual(ctypes.byref(prob), t, c["n"], None, *none) == INVALID_ARG
    for bad in (native.Problem(c["n"], 0, m, None, lits.ctypes.data_as(u32p)),
                native.Problem(c["n"], 0, m, offs.ctypes.data_as(u64p), None)):
        assert L.alll_pinned_residual(ctypes.byref(bad), None, 0, ctypes.byref(res), *none) == INVALID_ARG
    for case in CONFLICT_CASES:
        n, o, l, _, rc, _ = arrays(case)
        if rc not in (OK, INVALID_ARG):  # (the refusals that concern the instance, not the thresholds)
            got, out, r = call(native, n, o, l, None)
            assert got == rc and untouched(out, r)
    # every array NULL: the record alone; one array alone
    assert L.alll_pinned_residual(ctypes.byref(prob), t, c["n"], ctypes.byref(res), *none) == OK
    assert res.as_dict() == {k: c["res"][k] for k in FIELDS if k != "pad"}
    vm = np.full(c["n"], 12345, np.uint32)
    assert L.alll_pinned_residual(ctypes.byref(prob), t, c["n"], ctypes.byref(res), None, None, vm.ctypes.data_as(u32p),
                                  None, None) == OK
    assert vm.tolist() == c["res"]["var_map"].tolist() + [12345] * (c["n"] - c["res"]["n_vars"])


def test_record_layout(native, tmp_path):
    R = native.ResidualResult
    assert ctypes.sizeof(R) == 40
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("n_clauses", 0), ("n_literals", 8), ("n_falsified", 16),
                                                                  ("first_falsified", 24), ("n_vars", 32), ("pad", 36)]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "alll.h"\n'
                   "_Static_assert(sizeof(alll_residual_result) == 40, \"size\");\n"
                   "_Static_assert(offsetof(alll_residual_result, n_clauses) == 0, \"n_clauses\");\n"
                   "_Static_assert(offsetof(alll_residual_result, n_literals) == 8, \"n_literals\");\n"
                   "_Static_assert(offsetof(alll_residual_result, n_falsified) == 16, \"n_falsified\");\n"
                   "_Static_assert(offsetof(alll_residual_result, first_falsified) == 24, \"first_falsified\");\n"
                   "_Static_assert(offsetof(alll_residual_result, n_vars) == 32, \"n_vars\");\n"
                   "_Static_assert(offsetof(alll_residual_result, pad) == 36, \"pad\");\n"
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
    res = native.ResidualResult()
    none = (None,) * 5
    assert L.alll_residual(None, ctypes.byref(res), *none) == INVALID_ARG and native.last_error()
    assert L.alll_group_residual(None, ctypes.byref(res), *none) == INVALID_ARG
    # (a null result is refused before the handle is looked at: any non-null value will do)
    fake = ctypes.c_void_p(8)
    assert L.alll_residual(fake, None, *none) == INVALID_ARG
    assert L.alll_group_residual(fake, None, *none) == INVALID_ARG


def test_python_surface(native):
    from alllsatisfiabilitysolver_amd import (BatchSolver, GroupSolver, Solver, lift_assignment, residual_instance,
                                              solve_cubes, solve_cubes_propagated, solve_cubes_residual,
                                              solve_cubes_split, split_cubes)

    assert list(inspect.signature(residual_instance).parameters) == ["n_vars", "offsets", "literals", "thr"]
    assert list(inspect.signature(lift_assignment).parameters) == ["n_vars", "thr", "var_map", "words_res"]
    want = ["n_vars", "offsets", "literals", "cubes", "seeds", "max_iters"]
    assert list(inspect.signature(solve_cubes_residual).parameters) == want
    assert list(inspect.signature(solve_cubes).parameters) == want  # the portfolios keep their signatures
    assert list(inspect.signature(solve_cubes_propagated).parameters) == want
    assert list(inspect.signature(split_cubes).parameters) == ["n_vars", "offsets", "literals", "depth", "base", "device"]
    assert list(inspect.signature(solve_cubes_split).parameters) == ["n_vars", "offsets", "literals", "depth", "base",
                                                                     "seeds", "max_iters"]
    assert inspect.signature(Solver.residual).parameters["with_arrays"].default is True
    assert inspect.signature(GroupSolver.residuals).parameters["with_arrays"].default is True
    assert not hasattr(BatchSolver, "residuals") and not hasattr(BatchSolver, "residual")  # (no batch form)
    r = residual_instance(3, [0], [])  # no clause: nothing is kept
    assert C.counts(r) == dict(n_vars=0, n_clauses=0, n_literals=0, n_falsified=0, first_falsified=0)
    assert r["offsets"].tolist() == [0] and r["literals"].size == r["var_map"].size == r["clause_map"].size == r["thr"].size == 0
    with pytest.raises(ValueError):  # refused before a device is touched
        solve_cubes_residual(2, [0, 2], [0, 2], [[0], [2]], seeds=[1])


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_lift(native, name):
    """Pins kept, kept variables copied, the rest 0: lift_assignment is the restatement's lift."""
    from alllsatisfiabilitysolver_amd import lift_assignment

    c = C.case(name)
    r = c["res"]
    rng = np.random.default_rng(5)
    words_res = rng.integers(0, 1 << 32, (r["n_vars"] + 31) // 32, dtype=np.uint64).astype(np.uint32)
    words = lift_assignment(c["n"], c["thr"], r["var_map"], words_res)
    np.testing.assert_array_equal(words, C.lift(c["n"], c["thr"], r["var_map"], words_res))
    assert words.dtype == np.uint32 and words.size == (c["n"] + 31) // 32
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:c["n"]]
    res_bits = np.unpackbits(words_res.view(np.uint8), bitorder="little")[:r["n_vars"]]
    np.testing.assert_array_equal(bits[r["var_map"]], res_bits)
    rest = np.ones(c["n"], bool)
    rest[r["var_map"]] = False
    if c["thr"] is not None:
        pinned = (c["thr"] == 0) | (c["thr"] == C.PIN1)
        np.testing.assert_array_equal(bits[pinned], (c["thr"][pinned] == C.PIN1).astype(np.uint8))
        rest &= ~pinned
    assert not bits[rest].any()


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_the_lift_violates_exactly_the_mapped_clauses(native, name):
    """For any residual assignment, the original clauses that the lifted assignment violates are
    clause_map[the residual clauses it violates]: a dropped clause holds a pin that is true, a kept
    clause's pinned literals are false and its free ones are copied.  On every case, the seven
    fixpoint cases among them; with n_falsified == 0 (no empty residual clause) it says that a model
    of the residual lifts to a model of the original, whatever search found it."""
    from alllsatisfiabilitysolver_amd import lift_assignment

    assert set(C.FIXPOINT_CASES) <= set(C.ALL_CASES)
    c = C.case(name)
    r = c["res"]
    if name in C.FIXPOINT_CASES:
        assert r["n_falsified"] == 0
    n_words = (r["n_vars"] + 31) // 32
    rng = np.random.default_rng(17)
    tries = [np.zeros(n_words, np.uint32), np.full(n_words, 0xFFFFFFFF, np.uint32)]
    tries += [rng.integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    for words_res in tries:
        bad_res = C.violated(r["offsets"], r["literals"], words_res)
        words = lift_assignment(c["n"], c["thr"], r["var_map"], words_res)
        np.testing.assert_array_equal(C.violated(c["offs"], c["lits"], words), r["clause_map"][bad_res].astype(np.int64))
        assert bad_res.size >= r["n_falsified"]  # (an empty residual clause is violated by everything)


@pytest.mark.parametrize("name", ["W3000p", "R", "sat_bias", "far", "repeat"])
def test_a_residual_model_lifts_to_a_model(native, name):
    """The same on models: where a search without backtracking (resid_cases.greedy_model) finds a model
    of the residual, the lifted assignment satisfies the original.  (It cannot solve the residuals of
    A and B at ratio 4; the test above covers them without a solver.)"""
    from alllsatisfiabilitysolver_amd import lift_assignment

    c = C.case(name)
    r = c["res"]
    assert r["n_falsified"] == 0
    words_res = C.greedy_model(r["n_vars"], r["offsets"], r["literals"])
    assert words_res is not None and C.satisfied(r["offsets"], r["literals"], words_res)
    words = lift_assignment(c["n"], c["thr"], r["var_map"], words_res)
    assert C.satisfied(c["offs"], c["lits"], words)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("resid_host")
    exe = str(d / "resid_host_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "resid_host_dump.cpp"), os.path.join(CSRC, "alll_host.cpp")],
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


def unpack(raw, n, m, n_lits):
    """The five arrays of the dump's output file, each at its capacity."""
    out, at = {}, 0
    for k, dt, cnt in (("offsets", "<u8", m + 1), ("literals", "<u4", n_lits), ("var_map", "<u4", n),
                       ("clause_map", "<u8", m), ("thr", "<u4", n)):
        out[k] = np.frombuffer(raw, dt, cnt, at)
        at += cnt * int(dt[2])
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_sanitized_matches_the_reference(dump, name):
    d, run = dump
    c = C.case(name)
    i = C.ALL_CASES.index(name)
    f, o = d / f"case{i}.bin", d / f"out{i}.bin"
    f.write_bytes(pack(c["n"], c["offs"], c["lits"], c["thr"]))
    rows = run(f, o)
    r = c["res"]
    assert rows == [["rc", "0"], ["res", str(r["n_vars"]), str(r["n_clauses"]), str(r["n_literals"]),
                                  str(r["n_falsified"]), str(r["first_falsified"]), "0"]]
    out = unpack(o.read_bytes(), c["n"], c["offs"].size - 1, c["lits"].size)
    for k, used in (("offsets", r["n_clauses"] + 1), ("literals", r["n_literals"]), ("var_map", r["n_vars"]),
                    ("clause_map", r["n_clauses"]), ("thr", r["n_vars"])):
        np.testing.assert_array_equal(out[k][:used], r[k], err_msg=k)
        assert (out[k][used:] == 12345).all(), k


@pytest.mark.parametrize("case", [c for c in CONFLICT_CASES if c[5] != OK], ids=lambda c: c[0])
def test_sanitized_refusals_write_nothing(dump, case):
    d, run = dump
    n, offs, lits, thr, rc, _ = arrays(case)
    f, o = d / "refused.bin", d / "refused_out.bin"
    f.write_bytes(pack(n, offs, lits, thr))
    rows = run(f, o)
    assert rows == [["rc", str(rc)], ["res"] + ["12345"] * 6]
    out = unpack(o.read_bytes(), n, offs.size - 1, lits.size)
    assert all((a == 12345).all() for a in out.values())
