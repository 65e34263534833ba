"""The facts of the residual cases, pinned on the numpy restatement alone (tests/resid_cases.py;
DESIGN.md §4.12): what the host and the GPU tests then compare the library against.  No GPU."""
import numpy as np
import pytest

import prop_cases as P
import resid_cases as C
import split_cases as S

# name -> (residual variables, clauses, literals, n_falsified, first_falsified or None: none)
FACTS = {
    "A": (20002, 80000, 240000, 0, None),
    "A1p": (18621, 71631, 207654, 0, None),
    "A4": (19002, 74124, 216552, 0, None),
    "A4p": (18793, 72758, 211740, 0, None),
    "A2c": (18793, 72749, 211775, 1, 75696),
    "A3": (19002, 73988, 216255, 2, 6684),
    "B1p": (1850, 7100, 20495, 0, None),
    "B4p": (1872, 7228, 20987, 0, None),
    "B5p": (1883, 7321, 21342, 0, None),
    "PL": (19511, 80000, 240000, 0, None),
    "PLG2": (19091, 78235, 232950, 0, None),
    "W": (6596, 2500, 7500, 0, None),
    "W64": (6568, 2492, 7468, 0, None),
    "W3000p": (5413, 2122, 6065, 0, None),
}
# name -> residual clauses of 0, 1, 2 and 3 literals
WIDTHS = {"A1p": [0, 0, 7239, 64392], "A4": [0, 143, 5534, 68447]}


@pytest.mark.parametrize("name", list(FACTS))
def test_instance_facts(native, name):
    nv, nc, nl, nf, first = FACTS[name]
    c = C.case(name)
    r = c["res"]
    print(name, C.counts(r), C.widths(r))
    m = c["offs"].size - 1
    assert C.counts(r) == dict(n_vars=nv, n_clauses=nc, n_literals=nl, n_falsified=nf,
                               first_falsified=m if first is None else first)
    if name in WIDTHS:
        assert C.widths(r) == WIDTHS[name]


def test_further_facts(native):
    a = C.case("A")
    assert np.setdiff1d(np.arange(a["n"]), a["res"]["var_map"]).size == 1     # one variable never occurs
    assert C.widths(C.case("A4")["res"])[1] == 143                             # units are still present
    assert C.widths(C.case("A4p")["res"])[:2] == [0, 0]                        # and gone at the fixpoint
    pl = C.case("PL")
    assert 0 in P.hot_variables(pl["n"], pl["lits"])                           # hot-flagged literals
    r = C.case("R")
    assert np.unique(np.diff(r["offs"].astype(np.int64))).tolist() == list(range(2, 10))  # the ragged layout
    assert P.case("H2")["res"]["status"] == P.FIXPOINT and r["res"]["n_falsified"] == 0
    assert max(np.diff(r["res"]["offsets"].astype(np.int64))) == 9 and C.widths(r["res"])[1] == 0
    z = C.case("Z")["res"]
    print("Z", C.counts(z))
    assert z["n_falsified"] > C.TILE and z["n_clauses"] > C.TILE * C.TILE // 2  # falsified clauses in many tiles
    assert (np.diff(z["var_map"].astype(np.int64) // (32 * C.TILE)) > 0).sum() == 256  # kept variables in all 257 word tiles


@pytest.mark.parametrize("name", ["A1p", "A4p", "B1p", "B4p", "B5p", "W3000p"])
def test_clauses_under_propagated_thresholds_are_the_open_clauses(native, name):
    """The residual's clause count equals n_open of the split scores (§4.11) under the same thresholds."""
    c = C.case(name)
    _, rec = S.scores(c["n"], c["offs"], c["lits"], c["thr"])
    assert c["res"]["n_clauses"] == rec["n_open"]


def test_crafted_corners():
    def parts(name):
        r = C.case(name)["res"]
        return (r["offsets"].tolist(), r["literals"].tolist(), r["var_map"].tolist(), r["clause_map"].tolist(),
                r["thr"].tolist(), r["n_falsified"], r["first_falsified"])

    F = C.FAIR
    assert parts("repeat") == ([0, 2], [0, 0], [0], [0], [F], 0, 1)                      # x x !y, y = 1 -> x x
    assert parts("taut") == ([0, 2], [0, 1], [0], [0], [F], 0, 1)                        # x !x stays
    assert parts("dead") == ([0, 2, 2, 2, 3], [0, 2, 3], [1, 2], [0, 1, 2, 3], [F, F], 2, 1)
    assert parts("sat_bias") == ([0, 1], [1], [3], [2], [0x40000000], 0, 3)              # the bias is carried
    assert parts("all_sat") == ([0], [], [], [], [], 0, 3)                               # 0 / 0 / 0
    assert parts("far") == ([0, 2], [2, 1], [C.FAR_LOW, C.FAR_HIGH], [0], [F, F], 0, 2)
    assert C.FAR_LOW // 32 == 0 and C.FAR_HIGH // 32 == 300
    assert parts("null_thr") == ([0, 2, 3, 3], [4, 1, 2], [0, 1, 3], [0, 1, 2], [F, F, F], 1, 2)


def test_no_thresholds_is_all_fair(native):
    c = C.case("W")
    r = C.residual(c["n"], c["offs"], c["lits"], np.full(c["n"], C.FAIR, np.uint32))
    assert C.same(r, c["res"]) is None


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_shape_of_every_case(native, name):
    """Maps ascend, offsets start at 0, literals stay in range, and the residual clause j is the free
    part of the original clause clause_map[j]."""
    c = C.case(name)
    r = c["res"]
    assert r["offsets"][0] == 0 and r["offsets"].size == r["n_clauses"] + 1 and int(r["offsets"][-1]) == r["n_literals"]
    assert (np.diff(r["var_map"].astype(np.int64)) > 0).all() and (np.diff(r["clause_map"].astype(np.int64)) > 0).all()
    assert r["literals"].size == 0 or int(r["literals"].max()) >> 1 < r["n_vars"]
    assert np.unique(r["literals"] >> 1).size == r["n_vars"]  # every kept variable occurs
    back = 2 * r["var_map"][r["literals"] >> 1].astype(np.int64) + (r["literals"] & 1)
    for j in (0, r["n_clauses"] // 2, r["n_clauses"] - 1):
        if 0 <= j < r["n_clauses"]:
            o = int(r["clause_map"][j])
            orig = c["lits"][int(c["offs"][o]):int(c["offs"][o + 1])].astype(np.int64)
            free = orig if c["thr"] is None else orig[(c["thr"][orig >> 1] != 0) & (c["thr"][orig >> 1] != C.PIN1)]
            assert back[int(r["offsets"][j]):int(r["offsets"][j + 1])].tolist() == free.tolist()


def test_lift_of_a_residual_model():
    """A model of the residual lifts to a model of the original; pins kept, the rest 0."""
    c = C.case("sat_bias")
    words = C.lift(c["n"], c["thr"], c["res"]["var_map"], np.array([0], np.uint32))  # x3 = 0 satisfies (!x3)
    assert words.tolist() == [0b0001] and C.satisfied(c["offs"], c["lits"], words)
    assert not C.satisfied(c["offs"], c["lits"], C.lift(c["n"], c["thr"], c["res"]["var_map"], np.array([1], np.uint32)))
    c = C.case("far")
    words = C.lift(c["n"], c["thr"], c["res"]["var_map"], np.array([0b10], np.uint32))
    assert words.size == 301 and words[0] == 1 << 5 and words[300] == 1 << 10 and not words[1:300].any()
