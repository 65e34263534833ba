"""The facts of the propagation cases (tests/prop_cases.py), asserted on the numpy reference alone:
what every case is there to show, before any code under test is compared with it.  No GPU."""
import numpy as np
import pytest

import prop_cases as P
from group_cases import compose

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


# ---------------------------------------------------------------------------------------------
# The many-item cases of tests/test_gpu_prop_swarm.py: conditions on the reference, not measurements


def test_ladder_closed_form():
    """Item j ends after j rounds with j forced (a fixpoint, or the conflict at clause j); the items
    without thresholds and the clauseless ones apply nothing."""
    c = P.ladder()
    assert len(c["items"]) == P.N_LADDER == 130 and P.ladder_kind(0) == "plain"
    for j, ((n, offs, lits), thr, out, res) in enumerate(zip(c["items"], c["thrs"], c["outs"], c["ress"])):
        kind = P.ladder_kind(j)
        assert n == j + 2 and 1 <= (n + 31) // 32 <= 5
        assert res == P.ladder_closed_form(j), j
        assert (thr is None) == (kind == "none") and (offs.size == 1) == (kind == "clauseless" or j == 0)
        if thr is not None:
            want = thr.copy()
            if kind != "clauseless":
                want[1:j + 1] = P.PIN1  # the chain, and nothing else: the bias of the spare variable stays
            np.testing.assert_array_equal(out, want)
    assert c["ress"][0] == dict(status=P.FIXPOINT, rounds=0, n_forced=0, conflict_clause=0)
    assert {(n + 31) // 32 for n, _, _ in c["items"]} == {1, 2, 3, 4, 5}


def test_ladder_ends_in_every_round():
    """Every item that propagates ends in a round of its own, from 0 to 129; the round counts of the
    130 items cannot all differ (the 21 items without thresholds and the 12 clauseless ones make no
    round), so what is asserted is: every j whose item propagates occurs as a round count, 97 of them,
    the first and the last among them."""
    c = P.ladder()
    kinds = [P.ladder_kind(j) for j in range(P.N_LADDER)]
    rounds = {r["rounds"] for r in c["ress"]}
    assert rounds == {0} | {j for j, k in enumerate(kinds) if k in ("plain", "conflict")}
    assert len(rounds) == 97 and {0, 1, 2, 126, 129} <= rounds
    assert kinds.count("conflict") >= 15 and kinds.count("none") >= 20 and kinds.count("clauseless") >= 10
    assert sum(1 for r in c["ress"] if r["status"] == P.CONFLICT) >= 15
    assert sum(1 for r in c["ress"] if r["status"] == P.NONE) >= 20
    # a conflict item directly behind a clauseless one: its clauses start at a base that two items share
    assert (kinds[39], kinds[40]) == (kinds[116], kinds[117]) == ("clauseless", "conflict")
    places = compose(c["items"])[3]
    assert places[39]["clause_base"] == places[40]["clause_base"] and c["ress"][40]["status"] == P.CONFLICT
    # every wave of 64 words holds many items, which end in different rounds
    word_item = np.repeat(np.arange(P.N_LADDER), [p["n_words"] for p in places])
    assert word_item.size == 334  # (31 items of one word, 32 each of two, three and four, 3 of five: six waves)
    assert all(np.unique(word_item[w:w + 64]).size >= 12 for w in range(0, word_item.size - 63, 64))  # (full waves)


def test_mixed_group_facts():
    """The first wave of k_prop_apply is 64 distinct one-word items and the ladder's waves span items
    (the per-lane atomics); the chain of 4099 variables holds a whole wave (the shuffle sum) and forces
    variables in it and in the waves it shares with its neighbours; the hub of the star is hot in the
    union, far from variable 0."""
    c = P.mixed_group()
    places = compose(c["items"])[3]
    assert [p["n_words"] for p in places[:64]] == [1] * 64 and len(c["items"]) == 64 + P.N_LADDER + 5
    assert len({r["rounds"] for r in c["ress"][:64]}) >= 20
    word_item = np.repeat(np.arange(len(places)), [p["n_words"] for p in places])
    one_item = [w for w in range(0, word_item.size - 63, 64) if np.unique(word_item[w:w + 64]).size == 1]
    k = len(places) - 2  # the chain of 4099 variables
    assert len(one_item) == 1 and int(word_item[one_item[0]]) == k
    forced_words = places[k]["word_base"] + np.flatnonzero(c["outs"][k] != c["thrs"][k]) // 32
    inside = (forced_words >= one_item[0]) & (forced_words < one_item[0] + 64)
    assert inside.sum() >= 10 and (~inside).sum() >= 10
    b1, b2, c1, c4, star = c["ress"][-5:]
    assert (b1["status"], b1["rounds"]) == (P.FIXPOINT, 6) and (b2["status"], b2["rounds"]) == (P.CONFLICT, 1)
    assert (c1["status"], c1["rounds"]) == (P.FIXPOINT, 99) and (c4["status"], c4["rounds"]) == (P.FIXPOINT, 40)
    assert star == dict(status=P.FIXPOINT, rounds=1, n_forced=2000, conflict_clause=2000)
    n_u, offs_u, lits_u, _ = compose(c["items"])
    assert P.hot_variables(n_u, lits_u).tolist() == [places[-1]["var_base"]] and places[-1]["var_base"] > 15000


def test_ladder_caps():
    """max_rounds = 10: item 10 has exactly ten applying rounds and is a fixpoint (rule 4 before rule 5),
    item 11 is capped at 10 / 10.  1 and 129 likewise; under 129 nobody is capped."""
    for cap in P.LADDER_CAPS:
        c = P.ladder(P.N_LADDER, cap)
        for j, r in enumerate(c["ress"]):
            full = P.ladder_closed_form(j)
            if full["rounds"] <= cap:
                assert r == full, (cap, j)
            else:
                assert r == dict(status=P.ROUND_CAP, rounds=cap, n_forced=cap, conflict_clause=full["conflict_clause"] if
                                 full["status"] != P.CONFLICT else len(c["items"][j][1]) - 1), (cap, j)
    c = P.ladder(P.N_LADDER, 10)
    assert c["ress"][10] == dict(status=P.FIXPOINT, rounds=10, n_forced=10, conflict_clause=10)
    assert c["ress"][11] == dict(status=P.ROUND_CAP, rounds=10, n_forced=10, conflict_clause=11)
    assert P.ladder(P.N_LADDER, 129)["ress"][129] == dict(status=P.FIXPOINT, rounds=129, n_forced=129, conflict_clause=129)
    assert sum(1 for r in c["ress"] if r["status"] == P.ROUND_CAP) >= 80
    assert any(r["status"] == P.CONFLICT for r in c["ress"])  # (item 5 conflicts below the cap)
    rest = P.continued(P.ladder(), c)
    assert rest[11]["rounds"] == 1 and rest[129] == dict(status=P.FIXPOINT, rounds=119, n_forced=119, conflict_clause=129)


def test_prop_swarm_facts():
    from swarm_cases import swarm_case, swarm_thresholds

    c = P.prop_swarm()
    items = c["items"]
    assert items is swarm_case()["items"] and c["seeds"] is swarm_case()["seeds"]
    biased = [i for i, t in enumerate(c["thrs"]) if t is not None]
    assert 640 <= len(biased) <= 700  # about two thirds
    res = [c["ress"][i] for i in biased]
    count = lambda status, ok: sum(1 for r in res if r["status"] == status and ok(r["rounds"]))  # noqa: E731
    kinds = (count(P.FIXPOINT, lambda r: r == 0), count(P.FIXPOINT, lambda r: r == 1), count(P.FIXPOINT, lambda r: r >= 2),
             count(P.CONFLICT, lambda r: r == 0), count(P.CONFLICT, lambda r: r >= 1))
    print(kinds)
    assert min(kinds) >= 5, kinds
    widths = [np.diff(it[1].astype(np.int64)) for it in items]
    unbiased = [i for i, t in enumerate(c["thrs"]) if t is None]
    assert sum(1 for i in unbiased if (widths[i] == 1).any()) >= 100
    assert sum(1 for i in unbiased if (widths[i] == 0).any()) >= 1
    assert sum(1 for i in biased if items[i][1].size == 1) >= 50  # clauseless items with thresholds
    # a conflict at round 0 in clause 0 of the first item behind each run of clauseless items: in the
    # union that clause's index is the base the run shares
    places = compose(items)[3]
    for i in P.PROP_SWARM_AFTER_RUNS:
        assert c["ress"][i] == dict(status=P.CONFLICT, rounds=0, n_forced=0, conflict_clause=0)
        assert places[i - 2]["clause_base"] == places[i - 1]["clause_base"] == places[i]["clause_base"]
        assert places[i]["n_clauses"] > 0
    # swarm_thresholds is as it was
    assert swarm_thresholds(0, 5) is None and swarm_thresholds(4, 33)[0] == 0 and swarm_thresholds(4, 33)[32] == P.PIN1
    # the pins of the conflicts at round 0 are the host's pinned conflicts
    assert all(r["conflict_clause"] < len(items[i][1]) - 1 for i, r in zip(biased, res) if r["status"] == P.CONFLICT)


def test_limit_item_facts(native):
    from alllsatisfiabilitysolver_amd import batch_fits

    n, offs, lits = P.limit_instance()
    assert (n, offs.size - 1, lits.size) == (native.BATCH_MAX_VARS, native.BATCH_MAX_CLAUSES, native.BATCH_MAX_LITERALS)
    assert (n + 31) // 32 == 256 and batch_fits(n, offs.size - 1, lits.size) and not batch_fits(n + 1, offs.size - 1, lits.size)
    assert (np.diff(offs.astype(np.int64)) == 3).all()
    assert 16382 in lits.tolist() and 16383 in lits.tolist() and int(lits.max()) == 16383
    assert all(v // 32 == 255 for v in P.LIMIT_CHAIN + (P.LIMIT_TAIL,))
    want = [(P.FIXPOINT, 4, 15), (P.FIXPOINT, 5, 13), (P.CONFLICT, 0, 0), (P.FIXPOINT, 4, 32)]
    for cs, (status, rounds, forced) in enumerate(want):
        c = P.limit_item(cs)
        assert (c["res"]["status"], c["res"]["rounds"], c["res"]["n_forced"]) == (status, rounds, forced)
        assert c["thr"][8191] == P.FAIR and c["thr"][P.LIMIT_CHAIN[0]] == P.PIN1
        if status == P.FIXPOINT:  # variable 8191 is forced, not pinned, and the tail link behind it too
            assert c["res"]["rounds"] >= 2
            assert c["out"][8191] == P.PIN1 and c["out"][P.LIMIT_TAIL] == P.PIN1
    outs = [P.limit_item(cs)["out"] for cs in range(4)]
    assert all(not np.array_equal(outs[a], outs[b]) for a in range(4) for b in range(a))


@pytest.mark.parametrize("name", ["ladder", "prop_swarm", "mixed_group"])
def test_many_item_references(native, oracle_mod, name):
    """What the GPU tests compare the words with: the host's biased fill of the propagated thresholds
    is the oracle's, at the items' 64-bit seeds; every item fits a batch (the mixed group need not);
    the three iterations after the propagation are not idle."""
    from alllsatisfiabilitysolver_amd import batch_fits, biased_initial_assignment

    c = getattr(P, name)()
    refs = getattr(P, name + "_references")()
    for i, ((n, offs, lits), seed, out, ref) in enumerate(zip(c["items"], c["seeds"], c["outs"], refs)):
        if out is not None:
            bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
            bits[:n] = biased_initial_assignment(seed, n, out)
            np.testing.assert_array_equal(np.packbits(bits, bitorder="little").view(np.uint32), ref[0], err_msg=f"item {i}")
            pinned = np.flatnonzero(np.isin(out, (0, P.PIN1)))
            for A in [ref[0]] + [r[4] for r in ref[1]]:  # the pins hold through the run
                got = np.unpackbits(A.view(np.uint8), bitorder="little")[pinned]
                np.testing.assert_array_equal(got, (out[pinned] == P.PIN1).astype(np.uint8), err_msg=f"item {i}")
        assert name == "mixed_group" or batch_fits(n, offs.size - 1, lits.size)
    assert sum(1 for ref in refs if ref[1] and ref[1][0][1] > 0) >= len(refs) // 4  # items that resample
