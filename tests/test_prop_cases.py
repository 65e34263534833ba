"""The facts of the propagation cases (tests/prop_cases.py), asserted on the numpy reference alone:
what every case is there to show, before any code under test is compared with it.  No GPU."""
import numpy as np
import pytest

import prop_cases as P

# name -> (status, rounds, forced, conflict clause or None)
FACTS = {
    "A1": (P.FIXPOINT, 8, 280, None),
    "A2": (P.CONFLICT, 2, 208, 75696),
    "A3": (P.CONFLICT, 0, 0, 6684),
    "A4": (P.FIXPOINT, 5, 209, None),
    "B1": (P.FIXPOINT, 6, 33, None),
    "B2": (P.CONFLICT, 1, 15, 7109),
    "B3": (P.CONFLICT, 0, 0, 7419),
    "C": (P.FIXPOINT, 299, 299, None),
    "C_cap": (P.ROUND_CAP, 100, 100, None),
    "C'": (P.FIXPOINT, 99, 99, None),
    "D": (P.CONFLICT, 1, 1, 1),
    "E": (P.FIXPOINT, 2, 3, None),
    "F": (P.CONFLICT, 0, 0, 1),
    "G": (P.CONFLICT, 1, 77, 129),
    "G2": (P.CONFLICT, 3, 228, 840),
    "H": (P.CONFLICT, 1, 2048, 412),
    "H2": (P.FIXPOINT, 6, 102, None),
}


def test_every_case_has_its_facts():
    assert sorted(FACTS) == sorted(P.ALL_CASES)


@pytest.mark.parametrize("name", P.ALL_CASES)
def test_facts(name):
    c = P.case(name)
    status, rounds, forced, clause = FACTS[name]
    m = len(c["offs"]) - 1
    assert c["res"] == dict(status=status, rounds=rounds, n_forced=forced, conflict_clause=m if clause is None else clause)
    changed = np.flatnonzero(c["out"] != c["thr"])
    assert changed.size == forced
    assert np.isin(c["out"][changed], (0, P.PIN1)).all() and (c["thr"][changed] == P.FAIR).all()


def test_sizes_leave_the_first_workgroup():
    """32 variables per lane of the pack and apply kernels, 256 lanes: 20003 variables are three
    workgroups with a ragged last word, 80000 clauses 313 workgroups of the scan."""
    n, offs, _ = P.a_instance()
    assert (n + 31) // 32 > 2 * 256 and n % 32 != 0 and (len(offs) - 1) > 256 * 256


def test_chain_crosses_workgroups_every_round():
    """Case C: consecutive links of the chain lie in different apply workgroups (8192 variables) for
    most rounds, and the clauses are stored against the direction of the implications."""
    _, _, _, p = P.chain(20003, 4099, 299)
    assert np.unique(p).size == 300
    assert np.mean((p[1:] // 8192) != (p[:-1] // 8192)) > 0.4
    _, _, _, q = P.chain(2003, 409, 99)
    assert np.unique(q).size == 100


def test_semantic_corners():
    d = P.case("D")
    assert d["out"][1] == P.PIN1  # forced both ways in one round: pinned to 1, the next round finds the conflict
    e = P.case("E")
    assert e["out"].tolist() == [P.PIN1, P.PIN1, 0x40000000, P.PIN1, P.PIN1, 0]  # x !x is no unit; a bias is free
    assert int(np.diff(e["offs"].astype(np.int64)).max()) == 10  # wider than the fixed-width layouts: generic CSR
    f = P.case("F")
    assert (f["out"] == f["thr"]).all()  # the conflict's round applies nothing, not even the unit next to it


def test_hot_and_ragged_cases():
    for name in ("G", "G2"):
        c = P.case(name)
        hot = P.hot_variables(c["n"], c["lits"])
        assert hot.size == 10  # what the device's planner flags: the ABI has no query for it
        forced = np.flatnonzero(c["out"] != c["thr"])
        assert np.intersect1d(forced, hot).size >= 6  # hot variables are among the forced ones
    for name in ("H", "H2"):
        w = np.diff(P.case(name)["offs"].astype(np.int64))
        assert w.min() == (1 if name == "H" else 2) and w.max() == 9


def test_round_zero_conflicts_are_the_pinned_conflicts(native):
    from alllsatisfiabilitysolver_amd import pinned_conflict

    for name in P.ALL_CASES:
        c = P.case(name)
        pc = pinned_conflict(c["n"], c["offs"], c["lits"], c["thr"])
        if c["res"]["status"] == P.CONFLICT and c["res"]["rounds"] == 0:
            assert pc == c["res"]["conflict_clause"], name
        else:
            assert pc is None, name


def test_live_cubes_of_the_portfolio():
    for name in P.B_LIVE_CUBES:
        assert P.case(name)["res"]["status"] == P.FIXPOINT
