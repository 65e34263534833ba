"""Per-variable probabilities in BatchSolver, the host side: alll_pinned_conflict
through the library and through tests/cpp/pinned_conflict_dump.cpp, the LDS layout with thresholds
through tests/cpp/batch_thr_layout_dump.cpp (both stand-alone programs built with a plain host compiler
under the address and undefined-behaviour sanitizers), and what solve_cubes decides before it touches
a device.  No GPU; no sanitizer on anything loaded into Python."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from bias_cases import PIN1
from conftest import ROOT

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG, BAD_INPUT, LITERAL_RANGE = 0, 1, 2, 3
HALF = 1 << 31

# the six-variable instance of test_gpu_bias.test_pins_that_cannot_be_met:
# (x0 | x1 | x2), (x3 | !x4 | x5), (!x3 | x4 | x0)
OFFS6 = np.array([0, 3, 6, 9], np.uint64)
LITS6 = np.array([0, 2, 4, 6, 9, 10, 7, 8, 0], np.uint32)
THR6 = np.array([0, 0, 0, HALF, HALF, PIN1], np.uint32)

# (name, n_vars, offsets, literals, thresholds, return code, clause or None)
CASES = [
    ("clause 0 dead", 6, OFFS6, LITS6, THR6, OK, 0),
    ("x2 unpinned", 6, OFFS6, LITS6, [0, 0, HALF, HALF, HALF, PIN1], OK, 3),
    ("x2 pinned true", 6, OFFS6, LITS6, [0, 0, PIN1, HALF, HALF, PIN1], OK, 3),
    # clause 1 = (x3 | !x4 | x5) dies with x3 = 0, x4 = 1 (a negative literal pinned false by PIN1), x5 = 0
    ("negative literal", 6, OFFS6, LITS6, [HALF, HALF, HALF, 0, PIN1, 0], OK, 1),
    ("a threshold of 1 is no pin", 6, OFFS6, LITS6, [1, 0, 0, HALF, HALF, PIN1], OK, 3),
    ("0xFFFFFFFE is no pin", 6, OFFS6, LITS6, [HALF, HALF, HALF, 0, 0xFFFFFFFE, 0], OK, 3),
    ("the first of two", 6, OFFS6, LITS6, [0, 0, 0, 0, PIN1, 0], OK, 0),
    ("empty clause", 3, [0, 2, 2, 4], [0, 3, 2, 5], [HALF] * 3, OK, 1),
    ("empty clause after a dead one", 3, [0, 1, 1], [0], [0, HALF, HALF], OK, 0),
    ("m = 0", 4, [0], [], [0, PIN1, 0, PIN1], OK, 0),  # (n_clauses = 0: "none")
    ("repeated variable", 2, [0, 3], [0, 0, 3], [0, PIN1], OK, 0),
    ("n + 1 thresholds", 6, OFFS6, LITS6, list(THR6) + [0], INVALID_ARG, None),
    ("n - 1 thresholds", 6, OFFS6, LITS6, list(THR6)[:-1], INVALID_ARG, None),
    ("literal range", 6, OFFS6, [0, 2, 4, 6, 9, 12, 7, 8, 0], THR6, LITERAL_RANGE, None),
    ("offsets[0] != 0", 6, [1, 3, 6, 9], LITS6, THR6, BAD_INPUT, None),
    ("offsets decrease", 6, [0, 3, 2, 9], LITS6, THR6, BAD_INPUT, None),
]


def arrays(case):
    _, n, offs, lits, thr, rc, want = case
    return n, np.asarray(offs, np.uint64), np.asarray(lits, np.uint32), np.asarray(thr, np.uint32), rc, want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pinned_conflict(native, case):
    n, offs, lits, thr, rc, want = arrays(case)
    m = offs.size - 1
    prob = native.Problem(n, 0, m, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                          lits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    c = ctypes.c_uint64(12345)
    got = native.lib().alll_pinned_conflict(ctypes.byref(prob), thr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                            thr.size, ctypes.byref(c))
    assert got == rc
    if rc == OK:
        assert c.value == want <= m
    else:
        assert c.value == 12345 and native.last_error()  # a refused call leaves the output alone


def test_pinned_conflict_null_arguments(native):
    L = native.lib()
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    prob = native.Problem(6, 0, 3, OFFS6.ctypes.data_as(u64p), LITS6.ctypes.data_as(u32p))
    c = ctypes.c_uint64()
    thr = THR6.ctypes.data_as(u32p)
    assert L.alll_pinned_conflict(None, thr, 6, ctypes.byref(c)) == INVALID_ARG
    assert L.alll_pinned_conflict(ctypes.byref(prob), None, 6, ctypes.byref(c)) == INVALID_ARG
    assert L.alll_pinned_conflict(ctypes.byref(prob), thr, 6, None) == INVALID_ARG
    for bad in (native.Problem(6, 0, 3, None, LITS6.ctypes.data_as(u32p)),
                native.Problem(6, 0, 3, OFFS6.ctypes.data_as(u64p), None)):
        assert L.alll_pinned_conflict(ctypes.byref(bad), thr, 6, ctypes.byref(c)) == INVALID_ARG


def test_pinned_conflict_python(native):
    from alllsatisfiabilitysolver_amd import pinned_conflict

    assert pinned_conflict(6, OFFS6, LITS6, THR6) == 0
    assert pinned_conflict(6, OFFS6, LITS6, [0, 0, HALF, HALF, HALF, PIN1]) is None
    assert pinned_conflict(4, [0], [], [0, 0, 0, 0]) is None


def test_symbols_are_declared_exported_and_bound(native):
    """The rule of test_abi (declared == exported) with the two new symbols in it."""
    text = open(os.path.join(ROOT, "include", "alll.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(alll_\w+)\(", text, re.M))
    for name in ("alll_batch_set_var_thresholds", "alll_pinned_conflict"):
        assert name in declared and name in native.EXPORTED and name in native._SIGS
        assert getattr(native.lib(), name).argtypes == native._SIGS[name][0]
    assert declared == set(native.EXPORTED)
    assert native.lib().alll_batch_set_var_thresholds(None, 0, None, 0) == INVALID_ARG  # a null batch, no device


def sanitized(tmp, name, *sources):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe, *sources],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines()}

    return run


@pytest.fixture(scope="module")
def conflict_dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("pinned_conflict")
    return d, sanitized(d, "pinned_conflict_dump", os.path.join(ROOT, "tests", "cpp", "pinned_conflict_dump.cpp"),
                        os.path.join(CSRC, "alll_host.cpp"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sanitized_pinned_conflict(conflict_dump, case):
    d, run = conflict_dump
    n, offs, lits, thr, rc, want = arrays(case)
    f = d / f"case{[c[0] for c in CASES].index(case[0])}.bin"
    f.write_bytes(struct.pack("<II", n, offs.size - 1) + offs.astype("<u8").tobytes() + struct.pack("<I", lits.size) +
                  lits.astype("<u4").tobytes() + struct.pack("<I", thr.size) + thr.astype("<u4").tobytes())
    out = run(f)
    assert out["rc"] == [rc] and out["clause"] == [want if rc == OK else 12345]


# ---------------------------------------------------------------------------------------------
# The LDS layout with thresholds (alll_batch.h).  The rule, restated: the arrays of the layout
# without thresholds, then u32[max variables]; every array starts at a multiple of 16 bytes; the
# thresholds are LDS-resident exactly when the total is within 160 KiB.

BUDGET = 160 * 1024


def up(x, a):
    return (x + a - 1) // a * a


def plain_bytes(n, m, lits):
    groups = (m + 63) // 64
    sizes = [2 * up(lits, 8), 2 * up(m + 1, 8), 8 * groups, 4 * n, 4 * ((n + 31) // 32), 4 * (groups + 1), 32,
             4 * up(m, 8)]
    return max(16, sum(up(s, 16) for s in sizes))


def rule_fits(n, m, lits):
    return plain_bytes(n, m, lits) + up(4 * n, 16) <= BUDGET


@pytest.fixture(scope="module")
def layout_dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_thr_layout")
    return sanitized(d, "batch_thr_layout_dump", os.path.join(ROOT, "tests", "cpp", "batch_thr_layout_dump.cpp"),
                     os.path.join(CSRC, "alll_batch.cpp"))


def limit_vars():
    """The largest n_vars whose thresholds fit the LDS at 8192 clauses / 24576 literals, from the rule."""
    fit = [n for n in range(1, 8193) if rule_fits(n, 8192, 24576)]
    assert fit and fit[-1] < 8192 and fit == list(range(1, fit[-1] + 1))  # (the rule is monotone in n)
    return fit[-1]


def shapes():
    top = limit_vars()
    return [(1, 1, 1), (203, 800, 2400), (200, 257, 771), (2048, 8192, 24576), (top, 8192, 24576),
            (top + 1, 8192, 24576), (8192, 8192, 24576), (8192, 1, 3), (0, 0, 0), (10, 0, 0)]


@pytest.mark.parametrize("shape", shapes())
def test_lds_layout_with_thresholds(layout_dump, shape):
    n, m, nl = shape
    out = layout_dump(n, m, nl)
    assert out["budget"] == [BUDGET]
    lits, offs, vmask, claim, A, prefix, ctl, lst, stride, total = out["with"]
    (at,) = out["thr_at"]
    groups = (m + 63) // 64
    need = [(lits, 2 * nl), (offs, 2 * (m + 1)), (vmask, 8 * groups), (claim, 4 * n), (A, 4 * ((n + 31) // 32)),
            (prefix, 4 * (groups + 1)), (ctl, 32), (lst, 2 * (stride + m)), (at, 4 * up(n, 4))]
    ends = sorted((a, a + size) for a, size in need if size)
    for (a0, a1), (b0, _) in zip(ends, ends[1:]):
        assert a1 <= b0  # no two arrays overlap
    assert all(a % 16 == 0 for a, _ in need) and ends[-1][1] <= total and at != 0
    assert total == plain_bytes(n, m, nl) + up(4 * n, 16)
    assert out["fits"] == [int(total <= BUDGET)] == [int(rule_fits(n, m, nl))]
    # the layout without thresholds is today's: the same offsets, its own total
    assert out["plain"][:9] == out["with"][:9] and out["plain"][9] == plain_bytes(n, m, nl)


def test_the_limit_of_the_lds_thresholds(layout_dump):
    """An item at all three limits does not fit (133,696 + 32,768 = 166,464 B > 160 KiB); the largest
    n_vars that fits at 8192 clauses / 24576 literals and the first that does not, from the rule."""
    top = limit_vars()
    assert layout_dump(8192, 8192, 24576)["plain"][9] == 133696
    assert layout_dump(8192, 8192, 24576)["with"][9] == 166464 > BUDGET
    assert layout_dump(top, 8192, 24576)["fits"] == [1] and layout_dump(top + 1, 8192, 24576)["fits"] == [0]
    assert layout_dump(top, 8192, 24576)["with"][9] <= BUDGET < layout_dump(top + 1, 8192, 24576)["with"][9]
    # 99,824 B of arrays that do not depend on n_vars, then 4 (claims) + 4 (thresholds) + 1/8 (assignment)
    # bytes a variable: (163,840 - 99,824) / 8.125 = 7,878 before the rounding to 16 bytes
    assert 7800 <= top <= 7900


def test_plain_layout_is_the_planners(layout_dump):
    """The three-argument layout equals the one the planner dump reports (test_batch_plan pins 133,696 B
    for an item at the limits and the thread counts)."""
    for n, m, nl in [(200, 800, 2400), (8192, 8192, 24576), (77, 7, 86)]:
        assert layout_dump(n, m, nl)["plain"][9] == plain_bytes(n, m, nl)


# ---------------------------------------------------------------------------------------------
# solve_cubes before the device


def test_solve_cubes_all_dead_needs_no_device(native):
    """Every cube pins a clause false: (None, None, None), on a machine without a GPU too."""
    from alllsatisfiabilitysolver_amd import solve_cubes

    # clause 0 = (x0 | x1 | x2): cubes that pin all three false; clause 1 = (x3 | !x4 | x5)
    cubes = [[1, 3, 5], [1, 3, 5, 6], [7, 8, 11]]
    assert solve_cubes(6, OFFS6, LITS6, cubes) == (None, None, None)
    assert solve_cubes(6, OFFS6, LITS6, []) == (None, None, None)
    # an empty clause kills every cube
    assert solve_cubes(3, [0, 2, 2], [0, 3], [[], [0]]) == (None, None, None)


def test_solve_cubes_refuses_bad_cubes(native):
    from alllsatisfiabilitysolver_amd import cube_thresholds, solve_cubes

    with pytest.raises(ValueError):
        solve_cubes(6, OFFS6, LITS6, [[1, 3, 5], [4, 5]])  # both polarities of x2
    with pytest.raises(ValueError):
        solve_cubes(6, OFFS6, LITS6, [[1, 3, 5], [12]])  # x6 of six variables
    with pytest.raises(ValueError):
        solve_cubes(6, OFFS6, LITS6, [[1, 3, 5]], seeds=[1, 2])
    assert cube_thresholds(4, [0, 3, 0]).tolist() == [PIN1, 0, HALF, HALF]  # (a literal named twice is one pin)
