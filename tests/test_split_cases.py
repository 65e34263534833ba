"""The facts of the split cases, pinned on the numpy reference alone (tests/split_cases.py; DESIGN.md
§4.11): what the host and the GPU tests then compare the library against.  No GPU."""
import collections

import numpy as np
import pytest

import prop_cases as P
import split_cases as C

# name -> (var, score_pos, score_neg, n_open, variables that tie for the maximum or None: not pinned)
FACTS = {
    "B": (563, 98304, 106496, 8000, 2),
    "B1p": (563, 98304, 122880, 7100, None),
    "B4p": (818, 122880, 98304, 7228, 2),
    "B5p": (563, 98304, 114688, 7321, 3),
    "A": (1473, 114688, 106496, 80000, 2),
    "A1p": (1473, 122880, 131072, 71631, None),
    "A4p": (7193, 114688, 106496, 72758, None),
    "PL": (0, 118177792, 118112256, 80000, None),
    "R": (6067, 87168, 35584, 20000, None),
}


@pytest.mark.parametrize("name", list(FACTS))
def test_instance_facts(native, name):
    var, pos, neg, n_open, ties = FACTS[name]
    c = C.case(name)
    print(name, c["rec"], C.n_ties(c["S"]))
    assert c["rec"] == dict(var=var, score_pos=pos, score_neg=neg, n_open=n_open)
    if ties is not None:
        assert C.n_ties(c["S"]) == ties
    assert int(c["S"].max()) < 1 << 47


def test_the_hub_of_the_power_law_instance(native):
    """Literal 0 collects 14,426 clauses of three free literals; its variable is one the device flags hot."""
    c = C.case("PL")
    assert int(c["S"][0]) == 14426 * 8192
    assert 0 in P.hot_variables(c["n"], c["lits"])


def test_crafted_corners():
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("wide20"))
    assert S.tolist() == [1, 0] * 20 and rec == dict(var=0, score_pos=1, score_neg=0, n_open=1)
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("repeat"))
    assert S.tolist() == [2 * 16384, 0, 0, 0] and rec == dict(var=0, score_pos=32768, score_neg=0, n_open=1)
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("taut"))
    assert S.tolist() == [16384, 16384] and rec == dict(var=0, score_pos=16384, score_neg=16384, n_open=1)
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("dead"))
    assert S.tolist() == [0, 0, 16384, 0, 16384, 0] and rec == dict(var=1, score_pos=16384, score_neg=0, n_open=3)
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("sat_bias"))
    assert S.tolist() == [0, 0, 16384, 0, 0, 16384] and rec == dict(var=1, score_pos=16384, score_neg=0, n_open=1)
    S, rec = (lambda c: (c["S"], c["rec"]))(C.case("all_sat"))
    assert not S.any() and rec == dict(var=4, score_pos=0, score_neg=0, n_open=0)
    c = C.case("tie_far")
    assert c["rec"] == dict(var=C.TIE_LOW, score_pos=16384, score_neg=0, n_open=1) and C.n_ties(c["S"]) == 2
    assert int(c["S"][2 * C.TIE_HIGH]) == 16384 and C.TIE_HIGH // 32 == 300


def test_no_thresholds_is_all_fair(native):
    c = C.case("B")
    S, rec = C.scores(c["n"], c["offs"], c["lits"], np.full(c["n"], C.FAIR, np.uint32))
    np.testing.assert_array_equal(S, c["S"])
    assert rec == c["rec"]


def summary(leaves, n_base=0):
    return (len(leaves), dict(collections.Counter(l["status"] for l in leaves)),
            dict(collections.Counter(len(l["cube"]) - n_base for l in leaves)))


def test_split_facts(native):
    n, st, ln = summary(C.split_case("S40")["leaves"])
    assert (n, st, ln) == (60, dict(open=39, conflict=17, satisfied=4), {6: 56, 5: 4})
    n, st, ln = summary(C.split_case("S33")["leaves"])
    assert (n, st) == (15, dict(open=1, conflict=14)) and (min(ln), max(ln)) == (2, 6)
    c = C.split_case("B_base")
    n, st, ln = summary(c["leaves"], len(c["base"]))
    assert (n, st, ln) == (32, dict(open=32), {5: 32})
    pinned = [int((l["thr"] != C.FAIR).sum()) for l in c["leaves"]]
    assert (min(pinned), max(pinned)) == (141, 155)
    n, st, ln = summary(C.split_case("PL")["leaves"])
    assert (n, st, ln) == (4, dict(conflict=4), {2: 4})


def test_split_leaves_are_a_partition(native):
    """The cubes of a split are distinct, open and satisfied leaves carry fixpoint thresholds that hold
    their cube, and `var == n_vars` holds exactly when no clause is open."""
    c = C.split_case("S40")
    cubes = [tuple(l["cube"]) for l in c["leaves"]]
    assert len(set(cubes)) == len(cubes)
    for l in c["leaves"]:
        if l["status"] == "conflict":
            assert l["thr"] is None
            continue
        for d in l["cube"]:
            assert l["thr"][d >> 1] == (0 if d & 1 else C.PIN1)
        again, res = P.propagate(c["n"], c["offs"], c["lits"], l["thr"])
        assert res["status"] == P.FIXPOINT and res["rounds"] == 0
        _, rec = C.scores(c["n"], c["offs"], c["lits"], l["thr"])
        assert (rec["var"] == c["n"]) == (rec["n_open"] == 0) == (l["status"] == "satisfied")
