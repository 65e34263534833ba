"""The host-only batch planner (alll_batch.cpp: validation, deduplication, 16-bit packing, LDS
layout) through tests/cpp/batch_plan_dump.cpp, a stand-alone program built with a plain host
compiler under the address and undefined-behaviour sanitizers.  No GPU, nothing loaded into
Python.  Every check restates a rule of the planner's comments; none compares recorded output."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, BAD_INPUT, LITERAL_RANGE, UNSUPPORTED = 0, 2, 3, 10


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_plan")
    exe = str(d / "batch_plan_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "batch_plan_dump.cpp"), os.path.join(CSRC, "alll_batch.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    count = [0]

    def run(problems, items, n_threads=1, world=1, stream_batch=0, flags=0):
        """problems: (n_vars, offsets, literals); items: (problem index, seed)."""
        blob = struct.pack("<I", len(problems))
        for n, offs, lits in problems:
            offs, lits = np.asarray(offs, "<u8"), np.asarray(lits, "<u4")
            blob += struct.pack("<II", n, offs.size - 1) + offs.tobytes() + struct.pack("<I", lits.size) + lits.tobytes()
        blob += struct.pack("<I", len(items)) + b"".join(struct.pack("<IQ", p, s) for p, s in items)
        blob += struct.pack("<iiQI", n_threads, world, stream_batch, flags)
        count[0] += 1
        src = d / f"in{count[0]}.bin"
        src.write_bytes(blob)
        r = subprocess.run([exe, str(src)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        out = {"item": []}
        for ln in r.stdout.splitlines():
            key, _, rest = ln.partition(" ")
            if key == "err":
                out["err"] = rest
            elif key == "item":
                out["item"].append([int(x) for x in rest.split()])
            else:
                out[key] = [int(x) for x in rest.split()]
        out["rc"] = out["rc"][0]
        return out

    return run


def ksat(n, m, k, seed):
    rng = np.random.default_rng(seed)
    lits = (rng.integers(0, n, m * k, dtype=np.uint32) << 1) | rng.integers(0, 2, m * k, dtype=np.uint32)
    return n, np.arange(m + 1, dtype=np.uint64) * k, lits


def ragged(n, widths, seed):
    rng = np.random.default_rng(seed)
    offs = np.zeros(len(widths) + 1, np.uint64)
    offs[1:] = np.cumsum(widths)
    L = int(offs[-1])
    return n, offs, (rng.integers(0, n, L, dtype=np.uint32) << 1) | rng.integers(0, 2, L, dtype=np.uint32)


def test_shared_problems_are_stored_once_and_round_trip(plan):
    P = [ksat(200, 400, 3, 1), ragged(77, [0, 1, 10, 3, 0, 70, 2], 2), (10, [0], [])]
    items = [(0, 1), (1, 5), (0, 2), (2, 9), (0, 3), (1, 6)]
    r = plan(P, items)
    assert r["rc"] == OK
    n_problems, a_words, max_vars, max_clauses, max_lits, threads = r["shape"]
    assert (n_problems, max_vars, max_clauses, max_lits) == (3, 200, 400, 1200)
    a_at = 0
    for (p, seed), it in zip(items, r["item"]):
        n, offs, lits = P[p]
        s, n_vars, n_words, m, n_lits, lits_at, offs_at, at = it
        assert (s, n_vars, n_words, m, n_lits) == (seed, n, (n + 31) // 32, len(offs) - 1, len(lits))
        assert lits_at % 8 == 0 and offs_at % 8 == 0  # 16-byte vectors of 16-bit elements
        assert at == a_at  # assignments back to back, every item its own
        a_at += n_words
        assert r["lits"][lits_at:lits_at + n_lits] == [int(x) for x in lits]
        assert r["offs"][offs_at:offs_at + m + 1] == [int(x) for x in offs]
    assert a_words == a_at
    # items of one problem point at one copy; the pools hold every problem once, padded to 8 elements
    starts = {p: set() for p in range(3)}
    for (p, _), it in zip(items, r["item"]):
        starts[p].add((it[5], it[6]))
    assert all(len(s) == 1 for s in starts.values())
    pad8 = lambda x: (x + 7) // 8 * 8
    assert len(r["lits"]) == sum(pad8(len(l)) for _, _, l in P)
    assert len(r["offs"]) == sum(pad8(len(o)) for _, o, _ in P)


@pytest.mark.parametrize("shape,want_threads", [((1, 1, 1), 64), ((200, 256, 3), 64), ((200, 257, 3), 128),
                                                ((200, 800, 3), 256), ((8192, 8192, 3), 1024)])
def test_lds_layout_and_workgroup_size(plan, shape, want_threads):
    n, m, k = shape
    r = plan([ksat(n, m, k, 3)], [(0, 1)])
    assert r["rc"] == OK and r["shape"][5] == want_threads
    lits, offs, vmask, claim, A, prefix, ctl, lst, stride, total = r["lds"]
    groups = (m + 63) // 64
    need = [(lits, 2 * m * k), (offs, 2 * (m + 1)), (vmask, 8 * groups), (claim, 4 * n), (A, 4 * ((n + 31) // 32)),
            (prefix, 4 * (groups + 1)), (ctl, 32), (lst, 2 * (stride + m))]
    assert stride >= m and stride % 8 == 0
    ends = sorted((at, at + size) for at, size in need)
    for (a0, a1), (b0, _) in zip(ends, ends[1:]):
        assert a1 <= b0  # no two arrays overlap
    assert all(at % 16 == 0 for at, _ in need) and ends[-1][1] <= total
    if shape == (8192, 8192, 3):
        assert total == 133696 and total <= 160 * 1024  # the byte budget of DESIGN.md §4.6


def test_item_errors_name_the_item(plan):
    good = ksat(50, 20, 3, 4)
    n, offs, lits = good
    for bad, code in [((n, [1] + list(offs[1:]), lits), BAD_INPUT),
                      ((n, list(offs[:5]) + [int(offs[4]) - 1] + list(offs[6:]), lits), BAD_INPUT),
                      ((n, offs, np.concatenate([lits[:-1], [2 * n]])), LITERAL_RANGE),
                      ((8193, offs, lits), UNSUPPORTED),
                      ((n, np.zeros(8194, np.uint64), []), UNSUPPORTED),
                      ((n, [0, 24577], np.zeros(24577, np.uint32)), UNSUPPORTED)]:
        r = plan([good, bad], [(0, 1), (0, 2), (1, 3)])
        assert r["rc"] == code and "item 2" in r["err"], r["err"]


def test_limits_are_accepted(plan):
    r = plan([(8192, np.arange(8193) * 3, np.full(24576, 2 * 8191 + 1, np.uint32))], [(0, 1)])
    assert r["rc"] == OK and r["lits"][:24576] == [2 * 8191 + 1] * 24576 and r["offs"][8192] == 24576


@pytest.mark.parametrize("opts", [{"n_threads": 4}, {"world": 2}, {"stream_batch": 1}, {"flags": 1 << 7}, {"flags": 1}])
def test_refused_options(plan, opts):
    assert plan([ksat(10, 5, 2, 1)], [(0, 1)], **opts)["rc"] == UNSUPPORTED
