"""Unit propagation of the pinned variables on the host: alll_pinned_propagate
through the library against the numpy reference of prop_cases.py on every case, its equivalence with
alll_pinned_conflict at round 0, the idempotence of a second call, the validation it shares with
alll_pinned_conflict, and the same function once more through tests/cpp/prop_host_dump.cpp, a
stand-alone program built with a plain host compiler under the address and undefined-behaviour
sanitizers.  No GPU; no sanitizer on anything loaded into Python."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import prop_cases as P
from conftest import ROOT
from test_batch_bias_host import CASES as CONFLICT_CASES, arrays

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK = 0
u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)


@pytest.mark.parametrize("name", P.ALL_CASES)
def test_matches_the_reference(native, name):
    from alllsatisfiabilitysolver_amd import propagate_pins

    c = P.case(name)
    thr, res = propagate_pins(c["n"], c["offs"], c["lits"], c["thr"], c["max_rounds"])
    assert res == c["res"]
    np.testing.assert_array_equal(thr, c["out"])
    # a second call finds what the first one left: the same status, nothing more to apply
    # (a call that stopped at its round cap is continued by the next: test_round_cap_continues_where_it_stopped)
    if c["res"]["status"] != P.ROUND_CAP:
        thr2, res2 = propagate_pins(c["n"], c["offs"], c["lits"], thr, c["max_rounds"])
        assert res2 == dict(c["res"], rounds=0, n_forced=0)
        np.testing.assert_array_equal(thr2, thr)


def test_round_cap_continues_where_it_stopped(native):
    from alllsatisfiabilitysolver_amd import propagate_pins

    c, full = P.case("C_cap"), P.case("C")
    thr, res = propagate_pins(c["n"], c["offs"], c["lits"], c["thr"], 100)
    assert res["status"] == P.ROUND_CAP
    thr, res = propagate_pins(c["n"], c["offs"], c["lits"], thr, 0)
    assert (res["status"], res["rounds"], res["n_forced"]) == (P.FIXPOINT, 199, 199)
    np.testing.assert_array_equal(thr, full["out"])


def many_cases():
    """The many-item cases of tests/test_gpu_prop_swarm.py: (name, case under max_rounds) -> the items with thresholds."""
    return {"ladder": lambda cap: P.ladder(P.N_LADDER, cap), "prop_swarm": P.prop_swarm,
            "limit": lambda cap: P.many([P.limit_instance()] * len(P.LIMIT_CUBES), [0] * len(P.LIMIT_CUBES),
                                        [P.limit_item(cs)["thr"] for cs in range(len(P.LIMIT_CUBES))], cap)}


@pytest.mark.parametrize("max_rounds", [0, 1, 10])
@pytest.mark.parametrize("name", ["ladder", "prop_swarm", "limit"])
def test_many_items_match_the_reference(native, name, max_rounds):
    """Every item with thresholds of the ladder, the prop swarm and the limit item under its four cubes,
    uncapped and capped at 1 and 10 rounds; a capped item is continued to the uncapped reference."""
    from alllsatisfiabilitysolver_amd import propagate_pins

    make = many_cases()[name]
    c, full = make(max_rounds), make(0)
    rest = P.continued(full, c)
    checked = capped = 0
    for i, ((n, offs, lits), thr) in enumerate(zip(c["items"], c["thrs"])):
        if thr is None:
            continue
        out, res = propagate_pins(n, offs, lits, thr, max_rounds)
        assert res == c["ress"][i], (name, i)
        np.testing.assert_array_equal(out, c["outs"][i], err_msg=f"{name} item {i}")
        if res["status"] == P.ROUND_CAP:
            out, res = propagate_pins(n, offs, lits, out, 0)
            assert res == rest[i], (name, i)
            np.testing.assert_array_equal(out, full["outs"][i], err_msg=f"{name} item {i}, continued")
            capped += 1
        checked += 1
    assert checked == {"ladder": 109, "prop_swarm": 669, "limit": 4}[name]
    # (no item of the prop swarm or of the limit cubes makes more than five rounds)
    assert (capped > 0) == (max_rounds == 1 or (name, max_rounds) == ("ladder", 10))


def call(native, n, offs, lits, thr, max_rounds=0):
    prob = native.Problem(n, 0, offs.size - 1, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.PropagateResult(12345, 12345, 12345, 12345)
    work = thr.copy()
    rc = native.lib().alll_pinned_propagate(ctypes.byref(prob), work.ctypes.data_as(u32p), work.size, max_rounds,
                                            ctypes.byref(res))
    return rc, work, res


@pytest.mark.parametrize("case", CONFLICT_CASES, ids=[c[0] for c in CONFLICT_CASES])
def test_validation_and_round_zero_are_those_of_pinned_conflict(native, case):
    n, offs, lits, thr, rc, want = arrays(case)
    got, work, res = call(native, n, offs, lits, thr)
    assert got == rc
    if rc != OK:  # a refused call writes nothing
        assert native.last_error()
        np.testing.assert_array_equal(work, thr)
        assert (res.conflict_clause, res.n_forced, res.rounds, res.status) == (12345,) * 4
        return
    m = offs.size - 1
    ref_thr, ref = P.propagate(n, offs, lits, thr)
    assert res.as_dict() == ref
    np.testing.assert_array_equal(work, ref_thr)
    assert (res.status == P.CONFLICT and res.rounds == 0) == (want < m)
    if want < m:
        assert res.conflict_clause == want


def test_null_arguments(native):
    L = native.lib()
    c = P.case("D")
    offs, lits, thr = c["offs"].copy(), c["lits"].copy(), c["thr"].copy()
    prob = native.Problem(4, 0, 3, offs.ctypes.data_as(u64p), lits.ctypes.data_as(u32p))
    res = native.PropagateResult()
    t = thr.ctypes.data_as(u32p)
    assert L.alll_pinned_propagate(None, t, 4, 0, ctypes.byref(res)) == 1
    assert L.alll_pinned_propagate(ctypes.byref(prob), None, 4, 0, ctypes.byref(res)) == 1
    assert L.alll_pinned_propagate(ctypes.byref(prob), t, 4, 0, None) == 1
    for bad in (native.Problem(4, 0, 3, None, lits.ctypes.data_as(u32p)), native.Problem(4, 0, 3, offs.ctypes.data_as(u64p), None)):
        assert L.alll_pinned_propagate(ctypes.byref(bad), t, 4, 0, ctypes.byref(res)) == 1
    np.testing.assert_array_equal(thr, c["thr"])


def test_python_leaves_the_callers_thresholds_alone(native):
    from alllsatisfiabilitysolver_amd import PROP_CONFLICT, PROP_FIXPOINT, PROP_NONE, PROP_ROUND_CAP, propagate_pins

    assert (PROP_FIXPOINT, PROP_CONFLICT, PROP_ROUND_CAP, PROP_NONE) == (0, 1, 2, 3)
    c = P.case("E")
    thr = c["thr"].copy()
    out, _ = propagate_pins(c["n"], c["offs"], c["lits"], thr)
    np.testing.assert_array_equal(thr, c["thr"])
    assert out is not thr and (out != thr).sum() == 3
    out, res = propagate_pins(3, [0], [], [0, P.FAIR, P.PIN1])  # no clause: a fixpoint at once
    assert res == dict(status=P.FIXPOINT, rounds=0, n_forced=0, conflict_clause=0)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("prop_host")
    exe = str(d / "prop_host_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "prop_host_dump.cpp"), os.path.join(CSRC, "alll_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return [ln.split() for ln in r.stdout.splitlines()]

    return d, run


def pack(n, offs, lits, thr):
    return (struct.pack("<II", n, offs.size - 1) + offs.astype("<u8").tobytes() + struct.pack("<I", lits.size) +
            lits.astype("<u4").tobytes() + struct.pack("<I", thr.size) + thr.astype("<u4").tobytes())


@pytest.mark.parametrize("name", P.ALL_CASES)
def test_sanitized_matches_the_reference(dump, name):
    d, run = dump
    c = P.case(name)
    i = P.ALL_CASES.index(name)
    f, o = d / f"case{i}.bin", d / f"out{i}.bin"
    f.write_bytes(pack(c["n"], c["offs"], c["lits"], c["thr"]))
    rows = run(f, c["max_rounds"], o)
    r = c["res"]
    want = [str(r["status"]), str(r["rounds"]), str(r["n_forced"]), str(r["conflict_clause"])]
    assert rows[0] == ["rc", "0"] and rows[1] == ["res", *want]
    again = ["100", "100"] if name == "C_cap" else ["0", "0"]  # (the capped chain goes on: 100 more rounds)
    assert rows[2] == ["rc", "0"] and rows[3] == ["res", want[0], *again, want[3]]
    np.testing.assert_array_equal(np.frombuffer(o.read_bytes(), "<u4"), c["out"])


@pytest.mark.parametrize("max_rounds", [0, 10])
def test_sanitized_ladder_union(dump, max_rounds):
    """The ladder's plain and clauseless items as one instance (group_cases.compose; the padding
    variables between the items are fair coins): 129 rounds in which every round ends another chain,
    and the cap at 10 with its continuation."""
    from group_cases import compose

    d, run = dump
    lad = P.ladder()
    keep = [j for j in range(P.N_LADDER) if P.ladder_kind(j) in ("plain", "clauseless")]
    n, offs, lits, places = compose([lad["items"][j] for j in keep])
    thr = np.full(n, P.FAIR, np.uint32)
    for j, p in zip(keep, places):
        thr[p["var_base"]:p["var_base"] + p["n_vars"]] = lad["thrs"][j]
    out, res = P.propagate(n, offs, lits, thr, max_rounds)
    forced = sum(min(lad["ress"][j]["rounds"], max_rounds or 129) for j in keep)
    assert res == dict(status=P.ROUND_CAP if max_rounds else P.FIXPOINT, rounds=max_rounds or 129, n_forced=forced,
                       conflict_clause=offs.size - 1)
    f, o = d / f"ladder{max_rounds}.bin", d / f"ladder_out{max_rounds}.bin"
    f.write_bytes(pack(n, offs, lits, thr))
    rows = run(f, max_rounds, o)
    assert rows[:2] == [["rc", "0"], ["res", str(res["status"]), str(res["rounds"]), str(forced), str(offs.size - 1)]]
    assert rows[2] == ["rc", "0"] and rows[3][:3] == (["res", str(P.ROUND_CAP), "10"] if max_rounds else ["res", "0", "0"])
    np.testing.assert_array_equal(np.frombuffer(o.read_bytes(), "<u4"), out)


@pytest.mark.parametrize("case", [c for c in CONFLICT_CASES if c[5] != OK], ids=lambda c: c[0])
def test_sanitized_refusals_write_nothing(dump, case):
    d, run = dump
    n, offs, lits, thr, rc, _ = arrays(case)
    f, o = d / "refused.bin", d / "refused_out.bin"
    f.write_bytes(pack(n, offs, lits, thr))
    rows = run(f, 0, o)
    assert rows[0] == ["rc", str(rc)] and rows[1] == ["res", "12345", "12345", "12345", "12345"]
    np.testing.assert_array_equal(np.frombuffer(o.read_bytes(), "<u4"), thr)
