"""The look-ahead splitter on the host and the ABI of the group probes:
split_cubes_lookahead(host=True) against the restatement of lookahead_cases.py, its refusals before
any device is touched, the Python surface, the new entry point declared, exported and bound, and its
null refusals (no device is touched).  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import lookahead_cases as L
from conftest import ROOT

OK, INVALID_ARG = 0, 1
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
NEW = "alll_group_probe_literals"


@pytest.mark.parametrize("name", ["S40_8", "S40_32", "S33_8", "random14", "crafted", "B_16"])
def test_host_splitter_matches_its_restatement(native, name):
    from alllsatisfiabilitysolver_amd import split_cubes_lookahead

    n, offs, lits, depth, base, k = L.split_input(name)
    L.same_leaves(split_cubes_lookahead(n, offs, lits, depth, base, n_candidates=k, host=True), L.split_case(name))


def test_defaults_are_those_of_the_signature(native):
    from alllsatisfiabilitysolver_amd import split_cubes_lookahead

    n, offs, lits, depth, base, _ = L.split_input("S40_32")
    L.same_leaves(split_cubes_lookahead(n, offs, lits, depth, host=True), L.split_case("S40_32"))


@pytest.mark.parametrize("host", [True, False])
def test_refusals_come_before_any_device(native, host):
    """depth 0 and 11 and n_candidates 0: ValueError on both paths (this machine has no device to touch)."""
    from alllsatisfiabilitysolver_amd import solve_cubes_lookahead, split_cubes_lookahead

    n, offs, lits, _, _, _ = L.split_input("crafted")
    for kw in (dict(depth=0), dict(depth=11), dict(depth=2, n_candidates=0)):
        with pytest.raises(ValueError):
            split_cubes_lookahead(n, offs, lits, host=host, **kw)
        with pytest.raises(ValueError):
            solve_cubes_lookahead(n, offs, lits, **kw)


def test_python_surface(native):
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver, solve_cubes_lookahead, split_cubes_lookahead

    sig = inspect.signature(split_cubes_lookahead)
    assert list(sig.parameters) == ["n_vars", "offsets", "literals", "depth", "base", "n_candidates", "device", "host"]
    assert [sig.parameters[k].default for k in ("base", "n_candidates", "device", "host")] == [(), 32, -1, False]
    sig = inspect.signature(solve_cubes_lookahead)
    assert list(sig.parameters) == ["n_vars", "offsets", "literals", "depth", "base", "n_candidates", "seeds", "max_iters"]
    assert [sig.parameters[k].default for k in ("base", "n_candidates", "seeds", "max_iters")] == [(), 32, None, 0]
    assert list(inspect.signature(GroupSolver.probes).parameters) == ["self", "probes", "max_rounds", "rows"]
    assert not hasattr(BatchSolver, "probes")  # (no batch form)
    assert not hasattr(GroupSolver, "probe") and not hasattr(BatchSolver, "probe")


def test_symbol_is_declared_exported_and_bound(native, tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include "alll.h"\n'
                   "_Static_assert(ALLL_ABI_VERSION == 1, \"the ABI version stays\");\n"
                   "int (*probes)(alll_group*, const uint32_t*, const uint64_t*, uint64_t, alll_propagate_result*, uint32_t*,\n"
                   "              uint32_t*, uint64_t) = alll_group_probe_literals;\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "alll.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(alll_\w+)\(", text, re.M))
    assert NEW in declared and NEW in native.EXPORTED and NEW in native._SIGS
    assert getattr(native.lib(), NEW).argtypes == native._SIGS[NEW][0]
    assert declared == set(native.EXPORTED)
    assert "No group or batch form" not in text


def test_null_group_results_and_offsets(native):
    """Refused before the handle is looked at or any device work, and nothing is written."""
    L_ = native.lib()
    res = (native.PropagateResult * 2)(*[native.PropagateResult(12345, 12345, 12345, 12345) for _ in range(2)])
    probes, offs = np.zeros(2, np.uint32), np.array([0, 2], np.uint64)
    rows = np.full(2, 12345, np.uint32)
    p, o, w = probes.ctypes.data_as(u32p), offs.ctypes.data_as(u64p), rows.ctypes.data_as(u32p)
    assert L_.alll_group_probe_literals(None, p, o, 0, res, None, None, 0) == INVALID_ARG and native.last_error()
    fake = ctypes.c_void_p(8)
    assert L_.alll_group_probe_literals(fake, p, o, 0, None, None, None, 0) == INVALID_ARG
    assert L_.alll_group_probe_literals(fake, p, None, 0, res, w, w, 2) == INVALID_ARG
    assert all(r.status == 12345 and r.rounds == 12345 for r in res) and (rows == 12345).all()
