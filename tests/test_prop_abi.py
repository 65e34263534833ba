"""Unit propagation of the pinned variables, the ABI: the result struct's layout in C
and in the binding, the seven entry points declared, exported and bound, their null refusals (no
device is touched), and the propagating form of solve_cubes.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

INVALID_ARG = 1
NEW = ["alll_pinned_propagate", "alll_propagate_pins", "alll_get_var_thresholds", "alll_group_propagate_pins",
       "alll_group_get_var_thresholds", "alll_batch_propagate_pins", "alll_batch_get_var_thresholds"]


def test_result_struct_layout(native, tmp_path):
    R = native.PropagateResult
    assert ctypes.sizeof(R) == 24
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("conflict_clause", 0), ("n_forced", 8), ("rounds", 16),
                                                                  ("status", 20)]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "alll.h"\n'
                   "_Static_assert(sizeof(alll_propagate_result) == 24, \"size\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, n_forced) == 8, \"n_forced\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, rounds) == 16, \"rounds\");\n"
                   "_Static_assert(offsetof(alll_propagate_result, status) == 20, \"status\");\n"
                   "_Static_assert(ALLL_PROP_FIXPOINT == 0 && ALLL_PROP_CONFLICT == 1 && ALLL_PROP_ROUND_CAP == 2 && "
                   "ALLL_PROP_NONE == 3, \"status values\");\n"
                   "_Static_assert(ALLL_ABI_VERSION == 1, \"the ABI version stays\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (native.PROP_FIXPOINT, native.PROP_CONFLICT, native.PROP_ROUND_CAP, native.PROP_NONE) == (0, 1, 2, 3)


def test_symbols_are_declared_exported_and_bound(native):
    text = open(os.path.join(ROOT, "include", "alll.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(alll_\w+)\(", text, re.M))
    for name in NEW:
        assert name in declared and name in native.EXPORTED and name in native._SIGS
        assert getattr(native.lib(), name).argtypes == native._SIGS[name][0]
    assert declared == set(native.EXPORTED)


def test_null_handles_and_null_results(native):
    L = native.lib()
    res = native.PropagateResult()
    out = np.zeros(4, np.uint32)
    o = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert L.alll_propagate_pins(None, 0, ctypes.byref(res)) == INVALID_ARG and native.last_error()
    assert L.alll_group_propagate_pins(None, 0, ctypes.byref(res)) == INVALID_ARG
    assert L.alll_batch_propagate_pins(None, 0, ctypes.byref(res)) == INVALID_ARG
    assert L.alll_get_var_thresholds(None, o, 4) == INVALID_ARG
    assert L.alll_group_get_var_thresholds(None, 0, o, 4) == INVALID_ARG
    assert L.alll_batch_get_var_thresholds(None, 0, o, 4) == INVALID_ARG
    assert L.alll_pinned_propagate(None, o, 4, 0, None) == INVALID_ARG
    # (a null result is refused before the handle is looked at: any non-null value will do)
    fake = ctypes.c_void_p(8)
    assert L.alll_propagate_pins(fake, 0, None) == INVALID_ARG
    assert L.alll_group_propagate_pins(fake, 0, None) == INVALID_ARG
    assert L.alll_batch_propagate_pins(fake, 0, None) == INVALID_ARG


def test_solve_cubes_propagated(native):
    """The propagating portfolio is a function of its own: solve_cubes keeps its signature (which
    test_best_abi pins) and its behaviour."""
    from alllsatisfiabilitysolver_amd import solve_cubes, solve_cubes_propagated

    want = ["n_vars", "offsets", "literals", "cubes", "seeds", "max_iters"]
    assert list(inspect.signature(solve_cubes).parameters) == want
    assert list(inspect.signature(solve_cubes_propagated).parameters) == want
    # every cube dead at depth 0: decided on the host, by both
    offs, lits = np.array([0, 2], np.uint64), np.array([0, 2], np.uint32)  # (x0 | x1)
    for fn in (solve_cubes, solve_cubes_propagated):
        assert fn(2, offs, lits, [[1, 3]]) == (None, None, None)


def test_solver_methods_exist(native):
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver, Solver

    for cls in (Solver, BatchSolver, GroupSolver):
        assert callable(cls.propagate_pins) and callable(cls.thresholds)
        assert inspect.signature(cls.propagate_pins).parameters["max_rounds"].default == 0
