"""The cases of tests/test_gpu_bias_blocks.py on the CPU (tests/bias_cases.py): the
facts the GPU comparisons rely on, so that a failure there is never a broken input and a change of
generate_ksat or mixed_thresholds cannot quietly shrink a case below the second workgroup of the
biased kernels.  No GPU; the references are computed once and shared with the GPU module."""
import numpy as np

import bias_cases as bc
from bias_cases import PIN1


def unsolved(rows, k):
    return len(rows) == k and all(r[1] > 0 and r[2].size > 0 for r in rows)


def test_sizes_leave_the_first_workgroup(native):
    """Words per case against the kernels' workgroups: 128 words per resample workgroup, 256 per fill
    workgroup."""
    words = lambda n: (n + 31) // 32
    wgs = lambda n, per: (words(n) + per - 1) // per
    assert (wgs(20003, bc.RESAMPLE_WG_WORDS), wgs(20003, bc.FILL_WG_WORDS)) == (5, 3) and 20003 % 32
    assert 20001 == 625 * 32 + 1 and wgs(20001, bc.RESAMPLE_WG_WORDS) == 5
    assert wgs(5003, bc.RESAMPLE_WG_WORDS) == 2 and wgs(9001, bc.RESAMPLE_WG_WORDS) == 3
    assert wgs(9001, bc.FILL_WG_WORDS) == 2


def test_blocks_case(native, oracle_mod):
    """1. Every `must` variable has its threshold, both pins are plentiful, and the reference is unsolved
    for its ten iterations, |U| 10139 -> 6878."""
    c = bc.blocks_case()
    assert (c["n"], c["offs"].size - 1, c["A0"].size) == (20003, 80000, 626)
    for v, t in bc.BLOCKS_MUST:
        assert int(c["thr"][v]) == t, v
    assert {v // 4096 for v, _ in bc.BLOCKS_MUST} == {0, 1, 2, 3, 4}  # a `must` variable in every resample workgroup
    assert ((c["thr"] == 0).sum(), (c["thr"] == PIN1).sum()) == (1922, 2047)
    assert unsolved(c["rows"], 10)
    s = bc.sizes(c["rows"])
    assert (s[0], s[-1]) == ((10139, 3349), (6878, 2524))
    # every resample workgroup redraws something in every iteration
    for r in c["rows"]:
        v = oracle_mod.clause_vars(c["offs"], c["lits"], r[2])
        assert set((v // 4096).tolist()) == {0, 1, 2, 3, 4}


def test_cover_all(native, oracle_mod):
    """2. cover_all: from all-false every clause is violated and in the MIS, so the assignment after
    iteration 0 is the draw of every variable; the later iterations are sparse."""
    o = oracle_mod
    offs, lits = bc.cover_all(12)
    assert offs.tolist() == [0, 3, 6, 9, 12] and lits.tolist() == list(range(0, 24, 2))
    c = bc.cover_all_case()
    n, thr = c["n"], c["thr"]
    assert n == 20001 and c["offs"].size - 1 == n // 3 and not c["A0"].any()
    assert bc.sizes(c["rows"]) == [(6667, 6667), (836, 836), (328, 328), (175, 175)]
    every = o.pack_bools(bc.biased_bits(o, c["seed"], 0, np.arange(n), thr))
    np.testing.assert_array_equal(c["rows"][0][4], every)
    assert ((thr == 0).sum(), (thr == PIN1).sum()) == (1958, 2008)
    a = o.unpack_words(every, n)
    assert (a[thr == PIN1] == 1).all() and (a[thr == 0] == 0).all()
    # the sparse side: in the last iteration most lanes (16 variables each) cover nothing
    v = o.clause_vars(c["offs"], c["lits"], c["rows"][-1][2])
    lanes = np.unique(v // 16).size
    assert 0 < lanes < (n + 15) // 16 // 2


def test_wrap_case(native):
    """3. Unsolved for the 260 iterations (min |U| = 1434), so every checkpoint compares a running loop."""
    c = bc.wrap_case()
    assert unsolved(c["rows"], bc.WRAP_ITERS)
    assert min(r[1] for r in c["rows"]) == 1434
    assert bc.WRAP_STOPS[0] < 255 and bc.WRAP_STOPS[-1] > 256 and {255, 256} <= set(bc.WRAP_STOPS)
    assert (c["thr"] == 0).sum() > 400 and (c["thr"] == PIN1).sum() > 400


def test_rr_cases(native):
    """4. T = 2 and T = 16: unsolved for the eight iterations; the round robin's MIS is not the LFMIS."""
    ends = {2: (2516, 1706), 16: (2516, 1696)}
    lfmis = bc.wrap_case()["rows"]
    for T, (first, last) in ends.items():
        rows = bc.rr_case(T)["rows"]
        assert unsolved(rows, 8) and (rows[0][1], rows[-1][1]) == (first, last)
        assert not np.array_equal(rows[0][2], lfmis[0][2])
    assert not np.array_equal(bc.rr_case(2)["rows"][0][2], bc.rr_case(16)["rows"][0][2])


def test_mixed_case(native):
    """5. Violated clauses at the start, and MIS clauses that repeat a variable (the draw is per variable)."""
    c = bc.mixed_case()
    w = np.diff(c["offs"].astype(np.int64))
    assert (w.min(), w.max()) == (1, 9)
    assert c["rows"][0][1] > 0 and len(c["rows"]) == 8
    assert bc.repeated_in_mis(c["offs"], c["lits"], c["rows"]) >= 1


def test_group_layout(native):
    """6. The table of the group: union words, words of the per-word bits and resample workgroups per item."""
    g = bc.group_case()
    assert [it[0] for it in g["items"]] == [1500, 5003, 33, 4097, 9001]
    assert [t is not None for t in g["thrs"]] == [False, True, True, False, True]
    assert bc.word_ranges(g["items"]) == [((0, 46), (0, 1), (0, 0)), ((47, 203), (1, 6), (0, 1)), ((204, 205), (6, 6), (1, 1)),
                                          ((206, 334), (6, 10), (1, 2)), ((335, 616), (10, 19), (2, 4))]
    # item 4 alone is longer than one workgroup of the fill
    assert (9001 + 31) // 32 > bc.FILL_WG_WORDS
    r = bc.group_case("ragged")
    assert r["items"][2][0] == 300 and np.diff(r["items"][2][1].astype(np.int64)).max() == 5
    assert bc.word_ranges(r["items"])[4] == ((343, 624), (10, 19), (2, 4))
    f = bc.group_case("fixed")  # every clause of the union has three literals, the words are the table's
    assert all((np.diff(it[1].astype(np.int64)) == 3).all() for it in f["items"])
    assert bc.word_ranges(f["items"]) == bc.word_ranges(g["items"])


def test_group_references(native):
    """6. No item is solved within the six steps (three for the ragged union and the restored item)."""
    g = bc.group_case()
    assert [len(rows) for _, rows in g["refs"]] == [6] * 5
    assert [rows[-1][1] for _, rows in g["refs"]] == [539, 1820, 1, 1392, 3284]
    assert all(r[1] > 0 for _, rows in g["refs"] for r in rows)
    for variant in ("ragged", "fixed"):
        assert all(unsolved(rows, 3) for _, rows in bc.group_case(variant)["refs"]), variant
    A0, rows = bc.group_item4_unbiased()
    assert len(rows) == 3 and rows[-1][1] > 0
    assert not np.array_equal(A0, g["refs"][4][0])  # the unbiased fill is another one


def test_blocks_unbiased(native):
    """7. The 20003-variable case without thresholds: four unsolved steps from another fill."""
    A0, rows = bc.blocks_unbiased()
    assert unsolved(rows, 4) and not np.array_equal(A0, bc.blocks_case()["A0"])
