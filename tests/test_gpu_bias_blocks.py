"""The biased fill and resample beyond one workgroup of variables (DESIGN.md §4.8 "Tests").
k_resample_biased and k_group_resample_biased give a lane 16 variables, so a workgroup of 256 lanes
holds 4096 variables (128 assignment words); k_init_biased holds 256 words (8192 variables) per
workgroup; a word of a group's per-word bits covers 32 words (1024 variables).  Every case here is the
smallest that reaches the second and later workgroups -- the global lane index in the threshold
pointer and the Philox counter, the fill's counter, a group item's local word against the union's,
the per-word bits past their second word -- and is compared bit for bit (assignment words, violated
mask, MIS, statistics) with tests/bias_cases.py, which composes the oracle's own primitives.  The
facts each case relies on are pinned without a GPU in tests/test_bias_cases.py and asserted again
here on the shared reference before the GPU is compared with it."""
import numpy as np
import pytest

import bias_cases as bc
from bias_cases import PIN1, follow, stats_after

pytestmark = pytest.mark.gpu

NO_GRAPH, GENERIC_CSR, ATOMIC_CLAIMS = 1 << 0, 1 << 2, 1 << 5
STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def unsolved(rows, k):
    return len(rows) == k and all(r[1] > 0 and r[2].size > 0 for r in rows)


def solver(c, **kw):
    from alllsatisfiabilitysolver_amd import Solver

    return Solver(c["n"], c["offs"], c["lits"], seed=c["seed"], **kw)


def pins_hold(s, thr):
    a = s.assignment()
    assert (a[thr == PIN1] == 1).all() and (a[thr == 0] == 0).all()


def check_stats(st, rows, k, what):
    want = stats_after(rows, k)
    assert {key: st[key] for key in want} == want, what


# name: (flags, environment around the creation)
BLOCK_VARIANTS = {"default": (0, {}), "csr": (GENERIC_CSR, {}), "no_graph": (NO_GRAPH, {}), "atomic_claims": (ATOMIC_CLAIMS, {}),
                  "buckets": (0, {"ALLL_BUCKET_MIN_U": "0"})}


@pytest.mark.parametrize("variant", list(BLOCK_VARIANTS))
def test_several_workgroups(gpu, oracle_mod, variant, monkeypatch):
    """1. n = 20003: five workgroups of the resample, three of the fill, pins and a bias on the
    workgroups' edges and on the last variable.  Ten single iterations under the layout flags, eager
    launches and the bucketed LFMIS round 0."""
    c = bc.blocks_case()
    thr, rows = c["thr"], c["rows"]
    assert unsolved(rows, 10) and (rows[0][1], rows[-1][1]) == (10139, 6878)
    assert all(int(thr[v]) == t for v, t in bc.BLOCKS_MUST)
    flags, env = BLOCK_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = solver(c, flags=flags)
    for k in env:
        monkeypatch.delenv(k)
    with s:
        s.set_thresholds(thr)
        follow(s, c["A0"], rows, variant)
        pins_hold(s, thr)


def test_several_workgroups_in_one_run(gpu, oracle_mod):
    """1b. The same ten iterations as one run(10): the replayed graphs without a host round trip per step."""
    c = bc.blocks_case()
    assert unsolved(c["rows"], 10)
    with solver(c) as s:
        s.set_thresholds(c["thr"])
        check_stats(s.run(10), c["rows"], 10, "run(10)")
        np.testing.assert_array_equal(s.assignment_words(), c["rows"][9][4])
        pins_hold(s, c["thr"])


def test_every_lane_draws(gpu, oracle_mod):
    """2. cover_all(20001) from the all-false assignment: iteration 0 redraws every variable, so one step
    compares all 16 draws of every lane of all five workgroups; the three sparse iterations after it
    have most lanes cover (and so load and draw) nothing."""
    o = oracle_mod
    c = bc.cover_all_case()
    n, thr, rows = c["n"], c["thr"], c["rows"]
    assert bc.sizes(rows) == [(6667, 6667), (836, 836), (328, 328), (175, 175)]
    every = o.pack_bools(bc.biased_bits(o, c["seed"], 0, np.arange(n), thr))
    np.testing.assert_array_equal(rows[0][4], every)
    assert ((thr == 0).sum(), (thr == PIN1).sum()) == (1958, 2008)
    with solver(c) as s:
        s.set_thresholds(thr)
        np.testing.assert_array_equal(s.assignment_words(), bc.biased_init(o, c["seed"], n, thr), err_msg="fill")
        s.set_assignment_words(c["A0"])
        follow(s, c["A0"], rows, "cover_all")
        pins_hold(s, thr)


def test_stamp_wrap(gpu, oracle_mod):
    """3. 260 iterations across the wrap of the 8-bit cover stamps (the cover array is cleared there): a
    pinned variable covered before the wrap is not redrawn after it, a covered one is.  Assignment
    and statistics at 250, 254, 255, 256, 257 and 260."""
    c = bc.wrap_case()
    rows = c["rows"]
    assert unsolved(rows, bc.WRAP_ITERS) and min(r[1] for r in rows) == 1434
    with solver(c) as s:
        s.set_thresholds(c["thr"])
        np.testing.assert_array_equal(s.assignment_words(), c["A0"], err_msg="fill")
        done = 0
        for stop in bc.WRAP_STOPS:
            st = s.run(stop - done)
            done = stop
            check_stats(st, rows, stop, stop)
            np.testing.assert_array_equal(s.assignment_words(), rows[stop - 1][4], err_msg=f"after {stop} iterations")
        pins_hold(s, c["thr"])


RR_MODES = {"fp": {}, "fp_cap1": {"ALLL_RR_FP_MAX": "1"}, "fp_cap2": {"ALLL_RR_FP_MAX": "2"}, "mw": {"ALLL_RR_FP": "0"}}


@pytest.mark.parametrize("mode", list(RR_MODES))
@pytest.mark.parametrize("T", [2, 16])
def test_round_robin_modes(gpu, oracle_mod, T, mode, monkeypatch):
    """4. The round robin of T sets under thresholds with every way of deciding its MIS: the fixpoint
    passes, the passes capped at one or two per iteration (a fall-back to the batch kernel mid-run)
    and the batch kernel alone.  Eight single iterations."""
    c = bc.rr_case(T)
    assert unsolved(c["rows"], 8) and (c["rows"][0][1], c["rows"][-1][1]) == {2: (2516, 1706), 16: (2516, 1696)}[T]
    for k in ("ALLL_RR_FP", "ALLL_RR_FP_MAX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in RR_MODES[mode].items():
        monkeypatch.setenv(k, v)
    with solver(c, n_threads=T) as s:
        s.set_thresholds(c["thr"])
        follow(s, c["A0"], c["rows"], f"T = {T}, {mode}")
        pins_hold(s, c["thr"])


def test_mixed_widths(gpu, oracle_mod):
    """5. generate_mixed(5, 9001, 20000, 1, 9): the ragged layout past one workgroup, with MIS clauses that
    repeat a variable (drawn once).  Generator seed 5 as first chosen: both conditions hold for it."""
    c = bc.mixed_case()
    assert c["rows"][0][1] > 0 and bc.repeated_in_mis(c["offs"], c["lits"], c["rows"]) >= 1
    with solver(c) as s:
        assert s.layout() == 0
        s.set_thresholds(c["thr"])
        follow(s, c["A0"], c["rows"], "mixed widths")
        pins_hold(s, c["thr"])


def own_solvers(g):
    from alllsatisfiabilitysolver_amd import Solver

    ones = []
    for item, seed, thr in zip(g["items"], g["seeds"], g["thrs"]):
        ones.append(Solver(*item, seed=seed))
        if thr is not None:
            ones[-1].set_thresholds(thr)
    return ones


def follow_group(gs, g, ones, steps, what, refs=None):
    """Every item of group gs after each run(1): assignment and statistics against its CPU reference
    and against a Solver of its own.  -> comparisons of items that still had violated clauses."""
    refs = g["refs"] if refs is None else refs
    for i, (A0, _) in enumerate(refs):
        np.testing.assert_array_equal(gs.assignment_words(i), A0, err_msg=f"{what}: fill, item {i}")
        if ones:
            np.testing.assert_array_equal(ones[i].assignment_words(), A0, err_msg=f"{what}: fill, solver {i}")
    busy = 0
    for it in range(steps):
        res = gs.run(1)
        for i, (_, rows) in enumerate(refs):
            check_stats(res[i], rows, it + 1, (what, i, it))
            np.testing.assert_array_equal(gs.assignment_words(i), rows[it][4], err_msg=f"{what}: item {i}, iteration {it}")
            if ones:
                st = ones[i].run(1)
                assert {k: res[i][k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (what, i, it)
                np.testing.assert_array_equal(gs.assignment_words(i), ones[i].assignment_words(),
                                              err_msg=f"{what}: item {i} against its solver, iteration {it}")
            busy += rows[it][1] > 0
    return busy


GROUP_WORDS = [((0, 46), (0, 1), (0, 0)), ((47, 203), (1, 6), (0, 1)), ((204, 205), (6, 6), (1, 1)), ((206, 334), (6, 10), (1, 2)),
               ((335, 616), (10, 19), (2, 4))]


@pytest.mark.parametrize("variant", ["table", "ragged", "fixed"])
def test_group_straddles_workgroups(gpu, oracle_mod, variant):
    """6. Five items, three of them biased: item 1's local words differ from the union's and cross a
    workgroup of the resample, words 1, 6 and 10 of the per-word bits hold biased and unbiased words,
    item 4 is longer than a workgroup of the fill.  The fill of every item, then six steps.  The
    2-SAT item among 3-SAT ones already makes the union generic CSR; three steps each repeat it with a
    mixed-width item 2 ("ragged") and with a 3-SAT item 2, the fixed-width layout ("fixed")."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    g = bc.group_case(variant)
    steps = g["steps"]
    assert steps == (6 if variant == "table" else 3) and all(unsolved(rows, steps) for _, rows in g["refs"])
    if variant == "ragged":
        assert bc.word_ranges(g["items"])[:2] == GROUP_WORDS[:2] and bc.word_ranges(g["items"])[4] == ((343, 624), (10, 19), (2, 4))
    else:
        assert bc.word_ranges(g["items"]) == GROUP_WORDS
    if variant == "table":
        assert [rows[-1][1] for _, rows in g["refs"]] == [539, 1820, 1, 1392, 3284]
    ones = own_solvers(g)
    try:
        with GroupSolver(g["items"], g["seeds"]) as gs:
            assert gs.layout() == (3 if variant == "fixed" else 0)
            for i in (1, 2, 4):
                gs.set_thresholds(i, g["thrs"][i])
            assert follow_group(gs, g, ones, steps, variant) >= 5 * steps
            for i in (1, 2, 4):
                a, thr = oracle_mod.unpack_words(gs.assignment_words(i), g["items"][i][0]), g["thrs"][i]
                assert (a[thr == PIN1] == 1).all() and (a[thr == 0] == 0).all(), i
    finally:
        for one in ones:
            one.close()


def test_group_restore_then_set(gpu, oracle_mod):
    """6b. Thresholds on item 4 set and taken back (its per-word bits, words 10-19, are cleared while
    other items stay biased), then items 1 and 2 set: item 4 follows the oracle's unbiased run, item 1
    the biased reference, as do the others."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    g = bc.group_case()
    refs = [(A0, rows[:3]) for A0, rows in g["refs"]]
    refs[4] = bc.group_item4_unbiased()
    assert all(unsolved(rows, 3) for _, rows in refs)
    with GroupSolver(g["items"], g["seeds"]) as gs:
        gs.set_thresholds(4, g["thrs"][4])
        np.testing.assert_array_equal(gs.assignment_words(4), g["refs"][4][0], err_msg="biased fill, item 4")
        gs.set_thresholds(4, None)
        gs.set_thresholds(1, g["thrs"][1])
        gs.set_thresholds(2, g["thrs"][2])
        assert follow_group(gs, g, None, 3, "restore", refs) == 15


def test_verify_before_thresholds(gpu, oracle_mod):
    """7a. verify() (an evaluation and a reduce) before the thresholds are set, at n_iterations == 0."""
    c = bc.blocks_case()
    A_plain, rows_plain = bc.blocks_unbiased()
    with solver(c) as s:
        assert s.verify() == (False, rows_plain[0][1])
        s.set_thresholds(c["thr"])
        follow(s, c["A0"], c["rows"][:4], "verify first")


def test_verify_after_thresholds(gpu, oracle_mod):
    """7b. verify() between set_thresholds and the first iteration counts the biased fill's violated clauses."""
    c = bc.blocks_case()
    with solver(c) as s:
        s.set_thresholds(c["thr"])
        assert s.verify() == (False, c["rows"][0][1])
        assert s.stats()["n_iterations"] == 0
        follow(s, c["A0"], c["rows"][:4], "verify after")


def test_assignment_imposed_then_thresholds_taken_back(gpu, oracle_mod):
    """7c. set_thresholds, an imposed assignment, set_thresholds(None): the unbiased fill replaces the
    imposed words, and four steps are those of a plain Solver (and of the oracle)."""
    c = bc.blocks_case()
    A_plain, rows_plain = bc.blocks_unbiased()
    assert unsolved(rows_plain, 4)
    W = oracle_mod.init_assignment(999, c["n"])
    assert not np.array_equal(W, A_plain) and not np.array_equal(W, c["A0"])
    with solver(c) as plain, solver(c) as s:
        s.set_thresholds(c["thr"])
        s.set_assignment_words(W)
        np.testing.assert_array_equal(s.assignment_words(), W)
        s.set_thresholds(None)
        np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words())
        np.testing.assert_array_equal(s.assignment_words(), A_plain)
        for it in range(4):
            assert s.run(1) == plain.run(1), it
            np.testing.assert_array_equal(s.assignment_words(), plain.assignment_words(), err_msg=f"iteration {it}")
            np.testing.assert_array_equal(s.mis(), plain.mis(), err_msg=f"MIS, iteration {it}")
            np.testing.assert_array_equal(s.violated_mask(), plain.violated_mask())
            np.testing.assert_array_equal(s.assignment_words(), rows_plain[it][4], err_msg=f"oracle, iteration {it}")
        assert plain.stats()["n_resamples"] > 0
