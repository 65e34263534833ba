"""The facts of the probe cases, pinned on the numpy reference alone
(probe_cases.py over prop_cases.propagate): nothing of the code under test runs here but the instance
generators.  The host tests and the GPU tests compare against these cases; this module says what the
cases are there for."""
from collections import Counter

import numpy as np

import probe_cases as C
import prop_cases as P

FIX, CON, CAP, NONE = P.FIXPOINT, P.CONFLICT, P.ROUND_CAP, P.NONE


def rec(c):
    return [(int(l), r["status"], r["rounds"], r["n_forced"], r["conflict_clause"]) for l, r in zip(c["probes"], c["res"])]


def bit(rows, p, v):
    return int(rows[p, v >> 5] >> (v & 31)) & 1


def test_rows_are_well_formed():
    for name in C.ALL_CASES:
        c = C.case(name)
        n, nw = c["n"], (c["n"] + 31) // 32
        assert c["pm"].shape == c["pv"].shape == (len(c["probes"]), nw)
        assert not (c["pv"] & ~c["pm"]).any()
        if n & 31:
            assert not (c["pm"][:, -1] >> (n & 31)).any()
        base = np.full(n, P.FAIR, np.uint32) if c["thr"] is None else c["thr"]
        bm, bv = C.pack_rows(base)
        assert not (bm & ~c["pm"]).any() and ((c["pv"] & bm) == bv).all()  # the base's pins stay in every row
        for p, (l, r) in enumerate(zip(c["probes"].tolist(), c["res"])):
            if r["status"] == NONE:
                assert (c["pm"][p] == bm).all() and (c["pv"][p] == bv).all()
            else:  # the probe's own pin, and n_forced more
                assert bit(c["pm"], p, l >> 1) == 1 and bit(c["pv"], p, l >> 1) == 1 - (l & 1)
                assert int(np.unpackbits((c["pm"][p] & ~bm).view(np.uint8)).sum()) == 1 + r["n_forced"]


def test_crafted_corners():
    # (!a | b)(!a | !b): a fails after one round -- b forced both ways, pinned 1, then clause 1 falsified
    c = C.case("fail_a")
    assert rec(c) == [(0, CON, 1, 1, 1), (1, FIX, 0, 0, 2), (2, FIX, 1, 1, 2), (3, FIX, 1, 1, 2)]
    assert bit(c["pm"], 0, 1) == 1 and bit(c["pv"], 0, 1) == 1  # the row is the start of the conflict round
    # with (a | c)(a | !c): both polarities of a fail, and every other probe runs into one of them
    c = C.case("fail_both")
    assert rec(c)[:2] == [(0, CON, 1, 1, 1), (1, CON, 1, 1, 3)] and all(r["status"] == CON for r in c["res"])
    # (!a | c)(a | c): c is pinned 1 under a and under !a; !c fails
    c = C.case("necessary")
    assert rec(c) == [(0, FIX, 1, 1, 2), (1, FIX, 1, 1, 2), (2, FIX, 0, 0, 2), (3, CON, 1, 1, 0)]
    assert [bit(c["pm"], p, 1) & bit(c["pv"], p, 1) for p in (0, 1)] == [1, 1]
    # case E of prop_cases, every literal: x1, x5 are pinned (NONE), x2 has a bias and is probed like a free one
    c = C.case("E_all")
    assert [r["status"] for r in c["res"]] == [FIX, CON, NONE, NONE, FIX, FIX, FIX, CON, FIX, CON, NONE, NONE]
    assert rec(c)[0] == (0, FIX, 2, 2, 4) and rec(c)[1] == (1, CON, 0, 0, 0) and rec(c)[9] == (9, CON, 1, 2, 3)
    assert c["thr"][2] == 0x40000000 and rec(c)[4][3] == 3  # (probing x2 repeats the base's own implications)
    # case F: the empty clause is a conflict at round 0 whatever is probed, the unit clause first where it is falsified
    assert rec(C.case("F_all")) == [(0, CON, 0, 0, 1), (1, CON, 0, 0, 0)]
    # a pinned 0 in the base: its probes are NONE; the others run under it
    c = C.case("pinned")
    assert rec(c) == [(0, NONE, 0, 0, 4), (1, NONE, 0, 0, 4), (2, CON, 1, 1, 3), (3, CON, 1, 1, 3), (4, CON, 0, 0, 3),
                      (5, CON, 0, 0, 2)]
    c = C.case("duplicate")
    assert c["probes"].tolist() == [0, 0, 1, 0, 5, 0] and rec(c)[0] == rec(c)[1] == rec(c)[3] == rec(c)[5]
    assert all(r["status"] == NONE for r in C.case("none_free")["res"])


def test_chain():
    """Probe i of chain C ends after 299 - 7 i rounds, as many forced: 43 different rounds in one slab."""
    c = C.case("C")
    assert c["thr"] is None and len(c["probes"]) == 43
    assert rec(c) == [(int(l), FIX, 299 - 7 * i, 299 - 7 * i, 299) for i, l in enumerate(c["probes"])]
    c = C.case("C_cap")
    assert c["max_rounds"] == 100 and len(c["probes"]) == 44
    want = [(CAP, 100) if 299 - 7 * i > 100 else (FIX, 299 - 7 * i) for i in range(43)] + [(FIX, 100)]
    assert [(r["status"], r["rounds"]) for r in c["res"]] == want  # (the last: a fixpoint found at the cap)
    assert Counter(s for s, _ in want) == {CAP: 29, FIX: 15}


def test_b_fail():
    base, res = C.b_fail_base()
    assert res == dict(status=FIX, rounds=14, n_forced=122, conflict_clause=8000)
    assert C.free_vars(base).size == 1711
    c = C.case("B_fail")
    assert len(c["probes"]) == 3422 and 3422 == 53 * 64 + 30
    failed = {int(l): (r["rounds"], r["n_forced"]) for l, r in zip(c["probes"], c["res"]) if r["status"] == CON}
    assert failed == {P.pos(350): (5, 19), P.pos(630): (6, 20), P.neg(1060): (8, 30), P.neg(1097): (7, 21),
                      P.pos(1172): (8, 22), P.pos(1815): (8, 27), P.pos(1894): (8, 22), P.pos(1993): (9, 31)}
    assert len({l >> 1 for l in failed}) == 8  # no variable fails both ways
    assert Counter(r["status"] for r in c["res"]) == {FIX: 3414, CON: 8}
    assert max(r["rounds"] for r in c["res"]) == 30 and max(r["n_forced"] for r in c["res"]) == 138
    sl = C.b_slices()
    assert [len(s["probes"]) for s in sl] == [1, 63, 64, 65, 130]
    assert all(s["res"][0]["status"] == CON and int(s["probes"][0]) == P.pos(350) for s in sl)
    c = C.case("B_free")  # no thresholds, width 3: pinning one literal makes no unit
    assert c["thr"] is None and all(r == dict(status=FIX, rounds=0, n_forced=0, conflict_clause=8000) for r in c["res"])


def test_a4_g2_h2():
    c = C.case("A4")
    assert len(c["probes"]) == 140 and Counter(r["status"] for r in c["res"]) == {FIX: 140}
    assert (min(r["rounds"] for r in c["res"]), max(r["rounds"] for r in c["res"])) == (0, 4)
    assert max(r["n_forced"] for r in c["res"]) == 7
    # G2's cube conflicts after three rounds; its first 200 pins propagate to a fixpoint
    g = P.case("G2")
    assert g["res"]["status"] == CON and C.fixpoint_prefix(g["n"], g["offs"], g["lits"], g["thr"])[1] == 200
    c = C.case("G2")
    hot = set(P.hot_variables(c["n"], c["lits"]).tolist())
    assert hot & {int(l) >> 1 for l in c["probes"]}  # hot-flagged variables are probed
    assert Counter(r["status"] for r in c["res"]) == {CON: 91, FIX: 39} and max(r["rounds"] for r in c["res"]) == 6
    assert max(r["n_forced"] for r in c["res"]) == 371
    h = P.case("H2")
    assert h["res"]["status"] == FIX and C.fixpoint_prefix(h["n"], h["offs"], h["lits"], h["thr"])[1] == 300
    c = C.case("H2")
    w = np.diff(c["offs"].astype(np.int64))
    assert (w.min(), w.max()) == (2, 9)
    assert Counter(r["status"] for r in c["res"]) == {FIX: 130} and max(r["rounds"] for r in c["res"]) == 4


def test_reduce_cases():
    def facts(name):
        r = C.reduce_case(name)
        return r["status"], r["passes"], r["n_failed"], r["n_necessary"], r["lookahead_var"]

    assert facts("B_fail") == ("open", 2, 1, 7, 1620)
    assert facts("fail_a") == ("satisfied", 2, 1, 0, 2)       # !a pinned; the pins then satisfy both clauses
    assert facts("fail_both") == ("conflict", 1, 0, 0, 3)
    assert facts("necessary") == ("satisfied", 2, 1, 0, 2)    # c is a candidate itself: !c fails
    assert facts("necessary1") == ("satisfied", 2, 0, 1, 2)   # a alone is: c is necessary
    assert facts("E_all") == ("open", 1, 0, 0, 2)
    assert facts("F_all") == ("conflict", 1, 0, 0, 1)         # the propagation of the base conflicts
    assert facts("pinned") == ("conflict", 1, 0, 0, 3)
    assert facts("random14") == ("open", 2, 3, 3, 6)
    assert facts("random14_one_pass") == ("open", 1, 3, 3, 6)
    assert facts("random14_3") == ("open", 2, 1, 5, 6)
    n, offs, lits = C.small_random()
    assert len(C.consistent_models(n, offs, lits, np.full(n, P.FAIR, np.uint32))) == 17
    # the restatement is sound by brute force on its own
    for name in C.BRUTE_CASES:
        n, offs, lits, thr, _ = C.reduce_input(name)
        before = C.consistent_models(n, offs, lits, np.full(n, P.FAIR, np.uint32) if thr is None else thr)
        r = C.reduce_case(name)
        if r["status"] == "conflict":
            assert not before, name
        else:
            assert C.consistent_models(n, offs, lits, r["thr"]) == before, name
