"""The facts tests/test_gpu_group_swarm.py relies on, from the oracle alone (no GPU): the sizes of the
swarms, when their items end, how many distinct items a tile and a 64-clause mask word hold in pass 1,
the empty clauses in the MIS, and that the high seed word matters.  Were one of them to fail, the GPU
cases would still pass but no longer run the loop trips they are there for."""
import numpy as np
import pytest

import swarm_cases as sc
from group_cases import compose
from swarm_cases import CAP, N_SWARM, TILE


@pytest.fixture(scope="module", params=[False, True], ids=["ragged", "fixed"])
def case(request, native, oracle_mod):
    return request.param, sc.swarm_case(request.param)


def test_sizes(case):
    """24,605 clauses (six full tiles of 4096 and a seventh of 29), 1,456 assignment words, and
    1000 = 3 * 256 + 232 items: four workgroups of k_group_best, the last one ragged."""
    fixed, c = case
    n_vars, offs, lits, places = compose(c["items"])
    assert len(c["items"]) == N_SWARM == 3 * 256 + 232
    assert offs.size - 1 == 24605 and (offs.size - 1 + TILE - 1) // TILE == 7
    assert sum(p["n_words"] for p in places) == 1456
    assert sum(1 for p in places if p["n_words"] == 1) >= 500  # one-word items: 32 of them share a wbias word
    # runs of clauseless items at the front, in the middle and (longer than a wave) at the end
    m = [p["n_clauses"] for p in places]
    assert m[:3] == [0, 0, 0] and m[3] > 0 and not any(m[300:341]) and not any(m[342:380]) and not any(m[-70:])
    assert m[341] == sc.HARD_M and m[-71] > 0
    widths = np.diff(offs.astype(np.int64))
    if fixed:
        assert (widths == 3).all()
    else:
        assert set(np.unique(widths).tolist()) == {0, 1, 2, 3, 4}


def test_ends(case):
    """Items end at every pass from 1 to CAP, and many are unsolved at the cap: the group keeps advancing
    while group_finish freezes more items at every pass."""
    fixed, c = case
    ends = {t.st["n_iterations"] for t in c["traces"] if t.st["solved"]}
    assert ends == set(range(1, CAP + 1))
    unsolved = sum(1 for t in c["traces"] if not t.st["solved"])
    assert unsolved >= (150 if fixed else 300)
    assert all(t.st["n_iterations"] == CAP for t in c["traces"] if not t.st["solved"])
    hard = [t for i, t in enumerate(c["traces"]) if i % 97 == 50]
    assert len(hard) == 10 and not any(t.st["solved"] for t in hard)


def test_distinct_items_per_tile_and_mask_word(case, oracle_mod):
    """Pass 1: every full tile has violated clauses and MIS clauses of at least 64 distinct items (a wave's
    merge sees more than one or two items, and wave 0's lanes several each), and some 64-clause mask
    word holds violated clauses of at least 5 items (a lane's run crosses items inside one word)."""
    fixed, c = case
    per_tile_U, per_tile_M, per_word = sc.first_pass_spread(oracle_mod, c["items"], [t.A0 for t in c["traces"]])
    assert len(per_tile_U) == len(per_tile_M) == 6
    assert min(per_tile_U) >= 64 and min(per_tile_M) >= 64, (per_tile_U, per_tile_M)
    assert per_word >= 5, per_word


def test_empty_clauses_sit_in_the_mis(native, oracle_mod):
    """Every emptied-clause item has its empty clause violated and in the MIS of every pass -- the oracle
    counts no resample for it -- and is unsolved at the cap."""
    o = oracle_mod
    c = sc.swarm_case()
    found = 0
    for i, ((n, offs, lits), t) in enumerate(zip(c["items"], c["traces"])):
        m = offs.size - 1
        if not (sc.emptied(i) and m):
            continue
        found += 1
        e = m // 2
        assert offs[e] == offs[e + 1] and not t.st["solved"] and len(t.rows) == CAP - 1
        A = t.A0
        for _, nu, nm, dres, A_next in t.rows:
            U, M = sc.pass_sets(o, (n, offs, lits), A)
            assert e in U.tolist() and e in M.tolist() and (U.size, M.size) == (nu, nm)
            Mi = M.astype(np.int64)
            assert dres == int((offs[Mi + 1] - offs[Mi]).sum())  # (the empty clause adds nothing)
            A = A_next
    assert found == 4
    some = [t for i, t in enumerate(c["traces"]) if sc.emptied(i) and c["items"][i][1].size > 1]
    assert any(r[2] == 1 and r[3] == 0 for t in some for r in t.rows)  # a pass whose whole MIS is the empty clause


def test_high_seed_word_matters(case, oracle_mod):
    """A kernel that ignored the high key word would not pass: the initial fill of every item with clauses
    and n >= 31 differs from that of the low word alone, and items of one shape and one low word have
    different traces."""
    o = oracle_mod
    fixed, c = case
    checked = 0
    for (n, offs, _), s in zip(c["items"], c["seeds"]):
        if offs.size > 1 and n >= 31:
            assert s >> 32 and not np.array_equal(o.init_assignment(s, n), o.init_assignment(s & 0xFFFFFFFF, n))
            checked += 1
    assert checked >= 400
    assert len({s & 0xFFFFFFFF for s in c["seeds"]}) == 5 and len({s >> 32 for s in c["seeds"]}) == N_SWARM
    # i and i + 385 (= 5 * 7 * 11) have the same variable and clause counts and the same low word
    pairs = 0
    for i in range(N_SWARM - 385):
        a, b = c["items"][i], c["items"][i + 385]
        if a[1].size > 1 and b[1].size > 1 and (a[0], a[1].size) == (b[0], b[1].size):
            assert c["seeds"][i] & 0xFFFFFFFF == c["seeds"][i + 385] & 0xFFFFFFFF
            ta, tb = c["traces"][i], c["traces"][i + 385]
            pairs += not np.array_equal(ta.A0, tb.A0) or [r[:4] for r in ta.rows] != [r[:4] for r in tb.rows]
    assert pairs >= 100
    # the resample stream too: the hard items, re-run from their own initial words under the low word alone
    for i in (50, 147):
        it, s, t = c["items"][i], c["seeds"][i], c["traces"][i]
        _, A_low, _ = o.solve(*it, s & 0xFFFFFFFF, max_iters=CAP, A0=t.A0)
        assert not np.array_equal(A_low, t.A)


def test_lockstep(native, oracle_mod):
    """130 items of 64 copies of one clause from all-false: pass 1 of every item has 64 violated clauses,
    one MIS clause and three resamples; in clause order, mask word j is item j and a full tile's MIS list
    holds one clause of each of 64 items.  The seeds differ in the high word only within a low word, and
    the three bits drawn in pass 1 differ among them."""
    c = sc.lockstep_case()
    assert len(c["items"]) == 130 and all(s >> 32 for s in c["seeds"])
    assert all(t.rows[0][1:4] == (64, 1, 3) for t in c["traces"])
    places = compose(c["items"])[3]
    assert [p["clause_base"] for p in places] == [64 * j for j in range(130)]  # mask word j is item j
    assert 130 * 64 == 2 * TILE + 128                                          # two full tiles and two words
    for low in range(5):
        after = {int(t.rows[0][4][0]) for t, s in zip(c["traces"], c["seeds"]) if s & 0xFFFFFFFF == low}
        assert len(after) >= 2
    assert max(len(t.rows) for t in c["traces"]) >= 2  # (somebody is still unsolved after pass 2)
    trajs = sc.lockstep_trajectories()
    assert all(tr[0][0] == 64 and not tr[0][1].any() for tr in trajs)


def test_structures_bag(native, oracle_mod):
    """The hub of star(2000, 1) is union variable 3 * 2016 = 6048, of degree 2000 >= HOT_THR_MIN = 1024;
    pass 1 from all-false has the known sets of tests/lfmis_structures.py."""
    c = sc.bag_case()
    places = compose(c["items"])[3]
    assert places[3]["var_base"] == 6048 and places[3]["n_clauses"] == 2000
    assert [t.rows[0][1:3] for t in c["traces"][3:]] == [(2000, 1), (300, 1), c["traces"][5].rows[0][1:3], (513, 257)]
    assert all(not t.st["solved"] for t in c["traces"][:3])  # the random items keep the group advancing
    assert all(len(t.rows) >= 9 or t.st["solved"] for t in c["traces"])


def test_rows_after_agrees_with_the_traces(native, oracle_mod):
    """rows_after (the biased references' rows) and Trace.after state one thing: on unbiased items, rows
    built with the oracle's own step give what the oracle's solve gives."""
    import bias_cases

    c = sc.swarm_case()
    for i in (3, 7, 50, 100, 218, 400, 929):
        A0, rows = bias_cases.unbiased_reference(oracle_mod, *c["items"][i], c["seeds"][i], 8)
        for steps in (1, 2, 5, 8):
            want, A = c["traces"][i].after(steps)
            got, B = sc.rows_after(A0, rows, steps)
            assert got == want, (i, steps)
            np.testing.assert_array_equal(A, B)


def test_thresholds_case(native, oracle_mod):
    """Every third item is biased, one-word items among them; the pins hold in the reference."""
    c, t = sc.swarm_case(), sc.thresholds_case()
    biased = [i for i, thr in enumerate(t["thrs"]) if thr is not None]
    assert biased == list(range(1, N_SWARM, 3))
    assert sum(1 for i in biased if c["items"][i][0] <= 32 and c["items"][i][1].size > 1) >= 100
    for i in biased:
        n, thr = c["items"][i][0], t["thrs"][i]
        assert thr[0] == 0 and (n == 1 or thr[n - 1] == sc.PIN1)
        for A in [t["refs"][i][0]] + [r[4] for r in t["refs"][i][1]]:
            assert not int(A[0]) & 1 and (n == 1 or (int(A[(n - 1) >> 5]) >> ((n - 1) & 31)) & 1)
    assert sum(1 for i in biased if len(t["refs"][i][1]) == sc.THR_STEPS and t["refs"][i][1][-1][1] > 0) >= 50
