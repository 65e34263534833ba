"""The host-only planner of alll_group_probe_literals (alll_group_probe.cpp: validation, layers, slots,
chunks under the byte budget or a forced layer count, record and row bases) through
tests/cpp/group_probe_plan_dump.cpp, a stand-alone program built with a plain host compiler under the
address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python.  Every layout is
compared with the numpy restatement lookahead_cases.plan."""
import os
import struct
import subprocess

import numpy as np
import pytest

import lookahead_cases as L
from conftest import ROOT

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG = 0, 1
BUDGET = 1 << 30


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_probe_plan")
    exe = str(d / "group_probe_plan_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "group_probe_plan_dump.cpp"),
                        os.path.join(CSRC, "alll_group_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    count = [0]

    def run(n_vars, probes, rows=False, n_row_words=None, forced=0, budget=BUDGET, offsets=None, null_offsets=False,
            null_probes=False):
        """probes: one sequence per item.  n_row_words None: the right count."""
        per = [np.asarray(p, "<u4") for p in probes]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum([p.size for p in per])])
        flat = np.concatenate(per) if per else np.zeros(0, "<u4")
        if n_row_words is None:
            n_row_words = sum(p.size * ((n + 31) // 32) for p, n in zip(per, n_vars))
        blob = (struct.pack("<I", len(n_vars)) + np.asarray(n_vars, "<u4").tobytes() + struct.pack("<I", null_offsets) +
                np.asarray(offsets, "<u8").tobytes() + struct.pack("<II", null_probes, flat.size) + flat.astype("<u4").tobytes() +
                struct.pack("<IQIQ", rows, n_row_words, forced, budget))
        count[0] += 1
        src = d / f"in{count[0]}.bin"
        src.write_bytes(blob)
        r = subprocess.run([exe, str(src)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        out = {"item": [], "chunk": [], "slot_base": [], "slot_item": [], "slot_row": []}
        for ln in r.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            if key == "err":
                out["err"] = rest
            elif key in ("item", "chunk", "slot_base", "slot_item", "slot_row"):
                out[key].append([int(x) for x in rest.split()])
            else:
                out[key] = [int(x) for x in rest.split()]
        out["rc"] = out["rc"][0]
        return out

    return run


def lits(n, count, seed=0):
    """count literals of an item of n variables, its last one among them."""
    if not count:
        return []
    rng = np.random.default_rng(seed)
    return [2 * n - 1] + rng.integers(0, 2 * n, count - 1).tolist()


def same(out, n_vars, counts, rows, forced=0, budget=BUDGET):
    want = L.plan(n_vars, counts, rows, forced, budget)
    assert out["rc"] == OK and out["err"] == ""
    assert out["shape"] == [sum(counts), want["n_layers"], want["max_item_vars"], want["nv_pad"], want["n_row_words"]]
    words = [(n + 31) // 32 for n in n_vars]
    base = np.concatenate([[0], np.cumsum(counts)]).tolist()
    wbase = np.concatenate([[0], np.cumsum(words)]).tolist()
    assert out["item"] == [[wbase[i], words[i], base[i], counts[i]] for i in range(len(n_vars))]
    assert out["row_base"] == want["row_base"]
    assert out["chunk"] == [list(c) for c in want["chunks"]]
    assert out["slot_base"] == [s[0] for s in want["slots"]]
    assert out["slot_item"] == [s[1] for s in want["slots"]]
    assert out["slot_row"] == [s[2] for s in want["slots"]]
    return want


EDGES_VARS = [70, 5, 2003, 64, 33, 1, 200]
EDGES_COUNTS = [0, 1, 63, 64, 65, 130, 0]


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("forced", [0, 1, 2, 3, 7])
def test_layer_edges(planner, rows, forced):
    """Items of 0, 1, 63, 64, 65 and 130 probes: one to three layers, the last ones ragged; forced layer
    counts make one, two and three chunks (the last ragged), whatever the budget says."""
    probes = [lits(n, k, i) for i, (n, k) in enumerate(zip(EDGES_VARS, EDGES_COUNTS))]
    out = planner(EDGES_VARS, probes, rows=rows, forced=forced, budget=1)
    want = same(out, EDGES_VARS, EDGES_COUNTS, rows, forced, 1)
    if forced:
        assert [c[1] for c in want["chunks"]] == {1: [1, 1, 1], 2: [2, 1], 3: [3], 7: [3]}[forced]
    else:  # a budget that holds nothing: a layer per chunk
        assert [c[1] for c in want["chunks"]] == [1, 1, 1]
    assert want["n_layers"] == 3 and [c[2] for c in want["chunks"]][0] >= 2
    assert sum(c[2] for c in want["chunks"]) == 1 + 1 + 1 + 2 + 3  # slots: (layer, item) pairs with probes only


def test_the_budget_cuts_the_chunks(planner):
    """As many layers as fit; without rows the rows cost nothing."""
    n_vars, counts = [2003, 100], [640, 130]
    probes = [lits(n, k, i) for i, (n, k) in enumerate(zip(n_vars, counts))]
    for rows in (False, True):
        whole = L.plan(n_vars, counts, rows)
        assert len(whole["chunks"]) == 1 and whole["chunks"][0][1] == 10
        first3 = sum(L.plan(n_vars, counts, rows, forced=1)["chunks"][l][4] for l in range(3))
        for budget in (first3 - 1, first3, BUDGET):
            want = same(planner(n_vars, probes, rows=rows, budget=budget), n_vars, counts, rows, 0, budget)
            assert want["chunks"][0][1] == {first3 - 1: 2, first3: 3, BUDGET: 10}[budget]
    # the delta tables: 32 bytes per layer and variable of the union, rounded up to whole waves
    assert L.plan(n_vars, counts, False, forced=1)["chunks"][9][4] == 32 * 2176 + L.SLOT_BYTES


def test_a_thousand_items_three_with_probes(planner):
    """Masks and records exist per (layer, item) pair with probes: 997 idle items cost their slot bases."""
    rng = np.random.default_rng(5)
    n_vars = rng.integers(1, 90, 1000).tolist()
    counts = [0] * 1000
    counts[0], counts[517], counts[999] = 3422, 64, 7
    probes = [lits(n, k, i) for i, (n, k) in enumerate(zip(n_vars, counts))]
    for rows in (False, True):
        want = same(planner(n_vars, probes, rows=rows), n_vars, counts, rows)
        assert want["n_layers"] == 54 and len(want["chunks"]) == 1 and want["chunks"][0][2] == 54 + 1 + 1
        same(planner(n_vars, probes, rows=rows, forced=5), n_vars, counts, rows, 5)


def test_no_probes(planner):
    out = planner([5, 70], [[], []], rows=True)
    assert out["rc"] == OK and out["shape"][:2] == [0, 0] and out["chunk"] == []
    out = planner([5, 70], [[], []], null_probes=True)
    assert out["rc"] == OK and out["chunk"] == []
    out = planner([], [])
    assert out["rc"] == OK and out["chunk"] == []


def test_refusals(planner):
    n_vars = [5, 70, 33]
    good = [[0, 9], [139, 1, 2], [65]]

    def refused(**kw):
        out = planner(n_vars, kw.pop("probes", good), **kw)
        assert out["rc"] == INVALID_ARG and out["err"], kw
        return out["err"]

    assert planner(n_vars, good, rows=True)["rc"] == OK
    refused(null_offsets=True)
    refused(null_probes=True)
    refused(offsets=[1, 2, 5, 6])          # do not start at 0
    refused(offsets=[0, 3, 2, 6])          # descend
    # a literal past its own item that is a valid literal of the union (whose variables reach 96 + 33)
    assert "item 0" in refused(probes=[[0, 10], [139, 1, 2], [65]])
    assert "item 2" in refused(probes=[[0, 9], [139, 1, 2], [66]])
    assert "item 1" in refused(probes=[[0, 9], [139, 140, 2], [65]])
    refused(probes=[[0, 9], [139, 1, 2], [0xFFFFFFFF]])
    # rows of the wrong size; not looked at without rows
    right = 2 * 1 + 3 * 3 + 1 * 2
    for bad in (0, right - 1, right + 1):
        refused(rows=True, n_row_words=bad)
        assert planner(n_vars, good, rows=False, n_row_words=bad)["rc"] == OK
    assert planner(n_vars, good, rows=True, n_row_words=right)["rc"] == OK
