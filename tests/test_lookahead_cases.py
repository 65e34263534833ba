"""The facts of the look-ahead splitter's cases, pinned on the restatement alone (lookahead_cases.split:
probe_cases.reduce, split_cases.scores, split_cases.cube_thr -- nothing of the code under test), the
soundness of its trees by brute force, and the group-probe cases' own shape.  No GPU, no library call
but the instance generators."""
import collections

import numpy as np
import pytest

import lookahead_cases as L
import probe_cases as C
import prop_cases as P
import split_cases as S


def census(leaves):
    return dict(collections.Counter(leaf["status"] for leaf in leaves))


def total(leaves, key):
    return sum(leaf[key] for leaf in leaves)


def test_s40_with_8_candidates():
    leaves = L.split_case("S40_8")
    assert len(S.split_case("S40")["leaves"]) == 60  # the splitter without look-ahead
    assert len(leaves) == 49 and census(leaves) == dict(open=32, conflict=3, satisfied=14)
    assert total(leaves, "n_failed") == 32 and total(leaves, "n_necessary") == 10
    assert max(leaf["passes"] for leaf in leaves) == 3


def test_s40_with_32_candidates():
    leaves = L.split_case("S40_32")
    assert len(leaves) == 56 and census(leaves) == dict(open=40, conflict=2, satisfied=14)


def test_s33_is_refuted_with_three_leaves():
    leaves = L.split_case("S33_8")
    assert len(S.split_case("S33")["leaves"]) == 15
    assert len(leaves) == 3 and census(leaves) == dict(conflict=3)
    assert all(leaf["thr"] is None for leaf in leaves)


def test_b_under_its_cube():
    """B under the cube of B_FAIL_CUBE at depth 3: the splitter without look-ahead returns 8 open leaves."""
    n, offs, lits, depth, base, _ = L.split_input("B_16")
    plain = S.split(n, offs, lits, depth, base)
    assert len(plain) == 8 and all(leaf["status"] == "open" for leaf in plain)
    leaves = L.split_case("B_16")
    assert len(leaves) == 7 and census(leaves) == dict(conflict=1, open=6)
    assert [len(leaf["cube"]) - len(base) for leaf in leaves if leaf["status"] == "conflict"] == [2]
    assert total(leaves, "n_necessary") == 8 and [leaf["passes"] for leaf in leaves].count(2) == 1
    assert max(leaf["passes"] for leaf in leaves) == 2
    leaves = L.split_case("B_32")
    assert len(leaves) == 7 and census(leaves) == dict(conflict=3, open=4)
    assert total(leaves, "n_failed") == 15 and total(leaves, "n_necessary") == 29


def test_the_tree_is_split_cubes_tree():
    """The leaf order is depth first, preferred literal first; the cubes extend the base; a leaf above
    `depth` is never open."""
    for name in ("S40_8", "crafted", "random14"):
        n, _, _, depth, base, _ = L.split_input(name)
        leaves = L.split_case(name)
        cubes = [tuple(leaf["cube"]) for leaf in leaves]
        assert len(set(cubes)) == len(cubes)
        for leaf in leaves:
            assert tuple(leaf["cube"][:len(base)]) == tuple(base) and len(leaf["cube"]) - len(base) <= depth
            assert leaf["status"] != "open" or len(leaf["cube"]) - len(base) == depth
            assert (leaf["thr"] is None) == (leaf["status"] == "conflict")
        # no cube is a prefix of another, and siblings differ in their last literal's sign only
        for a in cubes:
            assert not any(b != a and b[:len(a)] == a for b in cubes)


@pytest.mark.parametrize("name", ["random14", "crafted"])
def test_soundness_by_brute_force(name):
    n, offs, lits, _, base, _ = L.split_input(name)
    leaves = L.split_case(name)
    models = C.consistent_models(n, offs, lits, S.cube_thr(n, base))
    seen = set()
    for leaf in leaves:
        of_cube = C.consistent_models(n, offs, lits, S.cube_thr(n, leaf["cube"]))
        if leaf["status"] == "conflict":
            assert not of_cube  # a dead leaf's cube has no model
            continue
        own = C.consistent_models(n, offs, lits, leaf["thr"])
        assert own == of_cube          # the reduction loses and adds no model of the cube
        assert not (own & seen)        # the leaves are pairwise disjoint
        seen |= own
        if leaf["status"] == "satisfied":
            assert own
    assert seen == models              # and together they are the instance's models
    if name == "random14":
        assert len(models) == 17 and census(leaves) == dict(satisfied=6)


def test_the_crafted_conflict_is_found_by_failed_literals():
    """Under g = 1 unit propagation alone ends in a fixpoint; both literals of a then fail."""
    n, offs, lits, depth, _, k = L.split_input("crafted")
    leaves = L.split_case("crafted")
    dead = [leaf for leaf in leaves if leaf["status"] == "conflict"]
    assert len(dead) == 1 and dead[0]["cube"] == [2 * L.G] and dead[0]["passes"] == 1
    assert P.propagate(n, offs, lits, S.cube_thr(n, dead[0]["cube"]))[1]["status"] == P.FIXPOINT
    r = C.reduce(n, offs, lits, S.cube_thr(n, dead[0]["cube"]), k)
    assert r["status"] == "conflict" and [(v, a["status"], b["status"]) for v, a, b in r["candidates"]] == [
        (0, P.CONFLICT, P.CONFLICT)]


def test_the_group_probe_cases():
    """What the cases are there for."""
    c = L.one_word()
    assert len(c["items"]) == 130 and all(n <= 32 for n, _, _ in c["items"])
    assert all(len(p) == (6 if n == 3 else 4) for (n, _, _), p in zip(c["items"], c["probes"]))
    statuses = {r["status"] for res, _, _ in c["want"] for r in res}
    assert statuses == {P.NONE, P.FIXPOINT, P.CONFLICT}
    r = L.one_word(reverse=True)
    assert [n for n, _, _ in r["items"]] == [n for n, _, _ in c["items"]][::-1]
    c = L.ragged()
    assert [len(p) for p in c["probes"]][:6] == [1, 63, 64, 65, 130, 0]
    assert c["thrs"][6] is None and [n for n, _, _ in c["items"]][:7] == [2003] * 7
    assert c["want"][0][0][0]["status"] == P.CONFLICT  # the slices start at a failed literal
    c = L.capped()
    statuses = [r["status"] for r in c["want"][0][0]]
    assert c["max_rounds"] == 100 and P.ROUND_CAP in statuses and P.FIXPOINT in statuses
    assert any(r["status"] == P.FIXPOINT and r["rounds"] == 100 for r in c["want"][0][0])  # a fixpoint at the cap
    assert all(r["status"] != P.ROUND_CAP for r in c["want"][1][0])


def test_the_swarm():
    c = L.swarm()
    counts = [len(p) for p in c["probes"]]
    assert len(counts) == 1000 and set(counts) == {0, 3}
    assert {r["status"] for res, _, _ in c["want"] for r in res} >= {P.FIXPOINT, P.CONFLICT}
