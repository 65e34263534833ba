"""The host-only group planner (alll_group.cpp: validation, the items' places in the block-diagonal
union, the union's CSR, the per-word key table) through tests/cpp/group_plan_dump.cpp, a stand-alone
program built with a plain host compiler under the address and undefined-behaviour sanitizers.  No
GPU, nothing loaded into Python.  Every check compares with the numpy restatement in group_cases.py.

Also here, on the CPU: the union argument itself -- the oracle run on the composed
union gives, per item, the violated sets and the MIS of the oracle run on each item alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from group_cases import compose, mixed_bag, oracle_step, word_table

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG, BAD_INPUT, LITERAL_RANGE, UNSUPPORTED = 0, 1, 2, 3, 10
NULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_plan")
    exe = str(d / "group_plan_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "group_plan_dump.cpp"), os.path.join(CSRC, "alll_group.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    count = [0]

    def run(problems, items, n_threads=1, world=1, stream_batch=0, flags=0, comm=0, null_seeds=False):
        """problems: (n_vars, offsets, literals); items: (problem index or NULL, seed)."""
        blob = struct.pack("<I", len(problems))
        for n, offs, lits in problems:
            offs, lits = np.asarray(offs, "<u8"), np.asarray(lits, "<u4")
            blob += struct.pack("<II", n, offs.size - 1) + offs.tobytes() + struct.pack("<I", lits.size) + lits.tobytes()
        if null_seeds:
            blob += struct.pack("<I", NULL)
        else:
            blob += struct.pack("<I", len(items)) + b"".join(struct.pack("<IQ", p, s) for p, s in items)
        blob += struct.pack("<iiQII", n_threads, world, stream_batch, flags, comm)
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


def test_union_layout_matches_the_numpy_restatement(plan):
    """Shared arrays, a zero-clause item, n_vars = 33, n_vars a multiple of 32, ragged widths with
    empty clauses, and a zero-variable item in the middle."""
    P = [ksat(200, 400, 3, 1), ragged(33, [0, 1, 10, 3, 0, 7, 2], 2), (10, [0], []), ksat(64, 5, 2, 3), (0, [0], [])]
    order = [(0, 1), (1, 5), (0, 2 ** 40 + 7), (2, 9), (4, 8), (3, 3), (0, 3), (1, 6)]
    r = plan(P, order)
    assert r["rc"] == OK
    items = [P[p] for p, _ in order]
    seeds = [s for _, s in order]
    n_vars, offs, lits, places = compose(items)
    assert r["shape"] == [n_vars, offs.size - 1, sum(pl["n_words"] for pl in places)]
    for (p, seed), it, pl in zip(order, r["item"], places):
        s, lit_base, n, n_words, var_base, word_base, clause_base, n_clauses = it
        assert (s, n) == (seed, P[p][0])
        assert var_base % 32 == 0 and var_base == 32 * word_base  # every item starts an assignment word
        assert (lit_base, n_words, var_base, word_base, clause_base, n_clauses) == (
            pl["lit_base"], pl["n_words"], pl["var_base"], pl["word_base"], pl["clause_base"], pl["n_clauses"])
    # the item table the device searches: ascending clause bases and the union's clause count
    assert r["clause_base"] == [pl["clause_base"] for pl in places] + [offs.size - 1]
    # the union's CSR: clause order inside an item kept, literals shifted by the item's variables
    assert r["offsets"] == [int(x) for x in offs]
    assert r["literals"] == [int(x) for x in lits]
    for (n, o, l), pl in zip(items, places):
        c0, m = pl["clause_base"], pl["n_clauses"]
        got_o = np.array(r["offsets"][c0:c0 + m + 1], np.int64) - pl["lit_base"]
        assert list(got_o) == [int(x) for x in o]
        got_l = np.array(r["literals"][pl["lit_base"]:pl["lit_base"] + int(np.asarray(o)[-1])], np.int64)
        assert list(got_l - 2 * pl["var_base"]) == [int(x) for x in np.asarray(l)[:int(np.asarray(o)[-1])]]
        if got_l.size:  # an item's clauses name its own variables only
            assert (got_l >> 1).min() >= pl["var_base"] and (got_l >> 1).max() < pl["var_base"] + n
    # the word table: the item's own key, its own word index, the bits above n_vars masked
    w = r["words"]
    assert [tuple(w[4 * i:4 * i + 4]) for i in range(len(w) // 4)] == word_table(items, seeds)
    tails = {pl["word_base"] + pl["n_words"] - 1 for pl in places if pl["n_words"]}
    for i in range(len(w) // 4):
        if i not in tails:
            assert w[4 * i + 3] == 0xFFFFFFFF
    i33 = places[1]
    assert i33["n_words"] == 2 and w[4 * (i33["word_base"] + 1) + 3] == 1  # n_vars = 33: one variable in the last word


@pytest.mark.parametrize("fixed", [False, True], ids=["ragged", "fixed"])
def test_swarm_plan_matches_the_numpy_restatement(plan, native, fixed):
    """The thousand-item swarms of tests/swarm_cases.py: the clause bases with their runs of equal
    entries (clauseless items at the front, in the middle and at the end), the seed's high word in
    every word row, and the tail masks of one-word items."""
    from swarm_cases import swarm

    items, seeds = swarm(fixed=fixed)
    r = plan(items, [(i, s) for i, s in enumerate(seeds)])
    assert r["rc"] == OK
    n_vars, offs, lits, places = compose(items)
    assert r["shape"] == [n_vars, 24605, 1456]
    bases = [pl["clause_base"] for pl in places] + [offs.size - 1]
    assert r["clause_base"] == bases
    assert bases[:4] == [0, 0, 0, 0] and len(set(bases[300:342])) == 1 and len(set(bases[342:381])) == 1
    assert bases[-71:] == [24605] * 71 and bases[-72] < 24605
    for it, pl, s in zip(r["item"], places, seeds):
        assert it == [s, pl["lit_base"], pl["n_vars"], pl["n_words"], pl["var_base"], pl["word_base"], pl["clause_base"],
                      pl["n_clauses"]]
    w = r["words"]
    rows = [tuple(w[4 * i:4 * i + 4]) for i in range(len(w) // 4)]
    want = word_table(items, seeds)
    assert rows == want
    assert all(row[1] == seeds[i] >> 32 for i, pl in enumerate(places)
               for row in rows[pl["word_base"]:pl["word_base"] + pl["n_words"]])
    assert len({row[1] for row in rows}) == len(items) and {row[0] for row in rows} == {0, 1, 2, 3, 4}
    tails = {rows[pl["word_base"] + pl["n_words"] - 1][3] for pl in places}
    assert {0x7FFFFFFF, 0xFFFFFFFF, 1, 0x7F, 0xFFFFFF} <= tails  # n = 31, 32, 33 and 65, 7, 120
    assert r["offsets"] == [int(x) for x in offs]
    assert r["literals"] == [int(x) for x in lits]


def test_ladder_plan_matches_the_numpy_restatement(plan):
    """The ladder of tests/prop_cases.py (the propagation's group case): items of 1 to 5 words, clauses
    of width 2, 1 and 0, and the clause bases that a clauseless item shares with the item behind it,
    which the propagation's scan searches."""
    import prop_cases as P

    c = P.ladder()
    items, seeds = c["items"], c["seeds"]
    r = plan(items, [(i, s) for i, s in enumerate(seeds)])
    assert r["rc"] == OK
    n_vars, offs, lits, places = compose(items)
    assert r["shape"] == [n_vars, offs.size - 1, 334]
    bases = [pl["clause_base"] for pl in places] + [offs.size - 1]
    assert r["clause_base"] == bases
    for j in range(len(items)):
        assert (bases[j] == bases[j + 1]) == (P.ladder_kind(j) == "clauseless" or j == 0), j
    for it, pl, s in zip(r["item"], places, seeds):
        assert it == [s, pl["lit_base"], pl["n_vars"], pl["n_words"], pl["var_base"], pl["word_base"], pl["clause_base"],
                      pl["n_clauses"]]
    w = r["words"]
    assert [tuple(w[4 * i:4 * i + 4]) for i in range(len(w) // 4)] == word_table(items, seeds)
    assert r["offsets"] == [int(x) for x in offs] and r["literals"] == [int(x) for x in lits]


def test_item_errors_name_the_item(plan):
    good = ksat(50, 20, 3, 4)
    n, offs, lits = good
    for bad, code in [((n, [1] + list(offs[1:]), lits), BAD_INPUT),
                      ((n, list(offs[:5]) + [int(offs[4]) - 1] + list(offs[6:]), lits), BAD_INPUT),
                      ((n, offs, np.concatenate([lits[:-1], [2 * n]])), LITERAL_RANGE),
                      ((0, [0, 1], [0]), LITERAL_RANGE)]:
        r = plan([good, bad], [(0, 1), (0, 2), (1, 3)])
        assert r["rc"] == code and "item 2" in r["err"], r["err"]


def test_sizes_past_the_batch_limits_are_accepted(plan):
    r = plan([(8193, np.arange(8194) * 3, np.full(3 * 8193, 2 * 8192 + 1, np.uint32))], [(0, 1), (0, 2)])
    assert r["rc"] == OK and r["shape"] == [32 * 257 + 8193, 2 * 8193, 2 * 257]
    assert r["literals"][-1] == 2 * (32 * 257 + 8192) + 1


def test_union_past_the_loop_limits_is_refused(plan):
    # 2^30 variables are 2^25 words; one word more is refused, and the message names the item that overflows
    # (refused while the items are placed: nothing of that size is allocated)
    r = plan([(1 << 30, [0], []), (1, [0], [])], [(0, 1), (1, 2)])
    assert r["rc"] == UNSUPPORTED and "item 1" in r["err"]


@pytest.mark.parametrize("opts", [{"n_threads": 4}, {"n_threads": 0}, {"world": 2}, {"stream_batch": 1}, {"comm": 9},
                                  {"flags": 1 << 7}, {"flags": 1 << 6}, {"flags": 1 << 1}, {"flags": 1 << 8}])
def test_refused_options(plan, opts):
    assert plan([ksat(10, 5, 2, 1)], [(0, 1)], **opts)["rc"] == UNSUPPORTED
    # refused before the items are looked at
    assert plan([(3, [0, 1], [6])], [(0, 1)], **opts)["rc"] == UNSUPPORTED


@pytest.mark.parametrize("flags", [1 << 0, 1 << 2, 1 << 3, 1 << 4, 1 << 5, 0b111101])
def test_honoured_flags(plan, flags):
    assert plan([ksat(10, 5, 2, 1)], [(0, 1)], flags=flags)["rc"] == OK


def test_null_and_empty(plan):
    P = [ksat(10, 5, 2, 1)]
    assert plan(P, [])["rc"] == INVALID_ARG
    assert plan(P, [(NULL, 1)])["rc"] == INVALID_ARG
    assert plan(P, [], null_seeds=True)["rc"] == INVALID_ARG


def test_union_argument_on_the_oracle(oracle_mod):
    """The union of the mixed bag, with every item's own initial assignment imposed and every item's
    own resample stream, against the oracle on each item alone, for three iterations: the violated
    set of the union is the union of the items' (shifted by their clause bases), and so is its
    lexicographically-first MIS."""
    o = oracle_mod
    items, seeds = mixed_bag()
    n_u, offs_u, lits_u, places = compose(items)
    A_i = [o.init_assignment(s, n) for (n, _, _), s in zip(items, seeds)]
    assert sum(a.size for a in A_i) == (n_u + 31) // 32
    m_u = offs_u.size - 1
    for it in range(3):
        A_u = np.concatenate(A_i)
        _, vm = o.eval_mask(offs_u, lits_u, A_u)
        U_u = o.mask_to_list(m_u, vm)
        M_u = o.lfmis(n_u, offs_u, lits_u, U_u)
        for i, ((n, offs, lits), s, pl) in enumerate(zip(items, seeds, places)):
            U, M, A_next = oracle_step(o, n, offs, lits, A_i[i], s, it)
            c0, c1 = pl["clause_base"], pl["clause_base"] + pl["n_clauses"]
            np.testing.assert_array_equal(U_u[(U_u >= c0) & (U_u < c1)] - c0, U, err_msg=f"violated, item {i}, it {it}")
            np.testing.assert_array_equal(M_u[(M_u >= c0) & (M_u < c1)] - c0, M, err_msg=f"MIS, item {i}, it {it}")
            A_i[i] = A_next
        assert U_u.size > 0  # (the bag is not solved this early: the comparison is not vacuous)
