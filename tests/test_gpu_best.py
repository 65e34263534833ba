"""Best-assignment tracking on the GPU: the record -- fewest violated clauses of an
eval pass, the first pass that found them, the words it evaluated -- of a context, of every item of a
group and of every item of a batch, compared bit for bit with the CPU trajectories of
tests/best_cases.py (the oracle's primitives; the GPU is never compared with itself except where a
group or batch item is also held against a tracking Solver of its own).  The facts a case relies on are
pinned without a GPU in tests/test_best_cases.py and asserted again here before the comparison."""
import ctypes

import numpy as np
import pytest

import best_cases as bc
from best_cases import counts, record

pytestmark = pytest.mark.gpu

NO_GRAPH, ALLREDUCE, GENERIC_CSR, ATOMIC_CLAIMS, LFMIS, REFERENCE_RNG = 1 << 0, 1 << 1, 1 << 2, 1 << 5, 1 << 6, 1 << 7
STAT_KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
U64_MAX = 2**64 - 1


@pytest.fixture(scope="module")
def gpu(native, oracle_mod):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def solver(c, **kw):
    from alllsatisfiabilitysolver_amd import Solver

    return Solver(c["n"], c["offs"], c["lits"], seed=c["seed"], **kw)


def same(got, want, what):
    """A record from the GPU against one from the reference: both numbers and every word."""
    assert (got["n_violated"], got["iteration"]) == (want["n_violated"], want["iteration"]), what
    np.testing.assert_array_equal(got["words"], want["words"], err_msg=f"{what}: words")


def is_empty(got, n):
    assert (got["n_violated"], got["iteration"]) == (U64_MAX, 0) and not got["words"].any()
    assert got["words"].size == (n + 31) // 32


def code_of(exc):
    return exc.value.code


# ----------------------------------------------------------------------------- 1. one context
@pytest.mark.parametrize("flags", [0, NO_GRAPH, GENERIC_CSR, ATOMIC_CLAIMS], ids=["default", "no_graph", "csr", "atomic_claims"])
def test_record_of_solve_run_and_split_runs(gpu, flags):
    """1. n = 203, 60 passes as one solve(max_iters = 60), as run(60) and as run(7); run(1); run(52):
    the same record, the reference's; everything else is that of a context that does not track."""
    c = bc.main_case()
    want = record(c["traj"])
    assert (want["n_violated"], want["iteration"]) == (37, 58) and want["iteration"] != c["passes"]
    with solver(c, flags=flags, max_iters=c["passes"], track_best=True) as s:
        is_empty(s.best(), c["n"])
        st = s.solve()
        assert st["n_iterations"] == c["passes"] and not st["solved"]
        same(s.best(), want, "solve")
        np.testing.assert_array_equal(s.assignment_words(), c["traj"][-1][1])
        final = st, s.assignment_words(), s.violated_mask(), s.mis()
        assert s.solve()["n_iterations"] == c["passes"]  # (a second call: nothing left to run)
        same(s.best(), want, "solve twice")
    with solver(c, flags=flags, max_iters=c["passes"]) as s:  # the same arguments without tracking
        st = s.solve()
        assert {k: st[k] for k in STAT_KEYS} == {k: final[0][k] for k in STAT_KEYS}
        for got, ref in zip((s.assignment_words(), s.violated_mask(), s.mis()), final[1:]):
            np.testing.assert_array_equal(got, ref)
    for split in ((60,), (7, 1, 52)):
        with solver(c, flags=flags) as s:
            s.track_best()
            done = 0
            for k in split:
                st = s.run(k)
                done += k
                assert st["n_iterations"] == done and st["n_violated"] == c["traj"][done - 1][0]
                same(s.best(), record(c["traj"][:done]), f"run {split} after {done}")


def test_tie_keeps_the_first_pass(gpu):
    """2. n = 33: the minimum 8 is found at passes 10 and 12; the record is pass 10."""
    c = bc.tie_case()
    us = counts(c["traj"])
    assert [p for p, u in enumerate(us, 1) if u == min(us)] == [10, 12]
    with solver(c, track_best=True) as s:
        s.run(11)
        same(s.best(), record(c["traj"][:11]), "before the tie")
        s.run(c["passes"] - 11)
        same(s.best(), record(c["traj"]), "after the tie")
        assert s.best()["iteration"] == 10


def test_solved_pass_is_the_record(gpu):
    """2b. n = 1, one unit clause against the initial bit: the record is the final assignment with 0."""
    c = bc.unit_case()
    want = record(c["traj"])
    assert want["n_violated"] == 0 and want["iteration"] == len(c["traj"]) >= 2
    with solver(c, track_best=True) as s:
        st = s.solve()
        assert st["solved"] and st["n_iterations"] == len(c["traj"])
        same(s.best(), want, "solved")
        np.testing.assert_array_equal(s.best()["words"], s.assignment_words())
        s.run(3)  # (a solved context stays as it is)
        same(s.best(), want, "after the end")


def test_capped_pass_is_the_record_and_survives_the_continuation(gpu):
    """3. max_iters = 58: the capped pass, which does not resample, is the strict minimum; run(5) lifts
    the cap and resamples the live assignment, the record keeps pass 58's words."""
    c = bc.capped_case()
    cap, traj = c["cap"], c["traj"]
    assert record(traj[:cap])["iteration"] == cap == 58 and record(traj)["iteration"] == cap
    with solver(c, max_iters=cap, track_best=True) as s:
        st = s.solve()
        assert st["n_iterations"] == cap and st["n_violated"] == 37
        same(s.best(), record(traj[:cap]), "capped")
        np.testing.assert_array_equal(s.best()["words"], s.assignment_words())
        for p in range(cap + 1, cap + bc.CAP_RUN + 1):
            st = s.run(1)
            assert st["n_violated"] == traj[p - 1][0]
            same(s.best(), record(traj[:p]), f"continuation, pass {p}")
        assert not np.array_equal(s.best()["words"], s.assignment_words())
    with solver(c, max_iters=cap, track_best=True) as s:  # the continuation as one run
        s.solve()
        s.run(bc.CAP_RUN)
        same(s.best(), record(traj), "continuation in one run")


def test_past_one_resample_workgroup(gpu):
    """4. n = 5003 (157 words: two resample workgroups), 40 passes: 1471 at pass 38."""
    c = bc.blocks_case()
    want = record(c["traj"])
    assert (want["n_violated"], want["iteration"]) == (1471, 38)
    with solver(c, track_best=True) as s:
        s.run(c["passes"])
        same(s.best(), want, "n = 5003")


def test_five_workgroups_with_pins_on_their_edges(gpu):
    """4b. n = 20003 under thresholds, pins and a bias on variables 4095 / 4096 and 16383 / 16384, until
    the reference's record is not the last pass."""
    c = bc.big_case()
    want = record(c["traj"])
    assert 2 <= want["iteration"] < c["passes"] <= bc.BIG_MAX_PASSES
    assert all(int(c["thr"][v]) == t for v, t in bc.BIG_MUST)
    with solver(c, track_best=True) as s:
        s.set_thresholds(c["thr"])
        s.run(c["passes"])
        assert s.stats()["n_violated"] == c["traj"][-1][0]
        same(s.best(), want, "n = 20003")
        a = np.unpackbits(s.best()["words"].view(np.uint8), bitorder="little")[:c["n"]]
        assert (a[c["thr"] == bc.PIN1] == 1).all() and (a[c["thr"] == 0] == 0).all()  # the record obeys the pins


def test_round_robin_and_biased_resample(gpu):
    """5. The round robin at T = 4 goes through the same resample kernel; thresholds with pins take the
    biased one."""
    c = bc.rr_case()
    assert record(c["traj"])["iteration"] != c["passes"]
    with solver(c, n_threads=c["T"], track_best=True) as s:
        s.run(c["passes"])
        assert s.stats()["n_violated"] == c["traj"][-1][0]
        same(s.best(), record(c["traj"]), "round robin")
    c = bc.biased_case()
    assert record(c["traj"])["iteration"] != c["passes"]
    with solver(c, track_best=True) as s:
        s.set_thresholds(c["thr"])
        s.run(c["passes"])
        same(s.best(), record(c["traj"]), "biased")
    with solver(c, n_threads=1, flags=LFMIS, track_best=True) as s:  # (a flag that does not change results)
        s.set_thresholds(c["thr"])
        s.run(c["passes"])
        same(s.best(), record(c["traj"]), "biased, ALLL_FLAG_LFMIS")


# ----------------------------------------------------------------------------- 6. the rules
def test_set_assignment_leaves_the_record(gpu):
    """6. An assignment set from outside is evaluated by the next pass and replaces the record only if
    it is strictly better."""
    c = bc.inject_case()
    traj = c["traj"]
    w, b = bc.INJECT_WORSE_AT, bc.INJECT_BETTER_AT
    before = record(traj[:w - 1])
    assert traj[w - 1][0] > before["n_violated"] > traj[b - 1][0]
    with solver(c, track_best=True) as s:
        s.run(w - 1)
        s.set_assignment_words(c["worse"])
        same(s.best(), before, "after set_assignment_words")
        s.run(1)
        assert s.stats()["n_violated"] == traj[w - 1][0]
        same(s.best(), before, "a worse assignment")
        s.run(b - 1 - w)
        same(s.best(), record(traj[:b - 1]), "before the better assignment")
        s.set_assignment_words(c["better"])
        same(s.best(), record(traj[:b - 1]), "after the second set_assignment_words")
        s.run(1)
        same(s.best(), record(traj[:b]), "a better assignment")
        assert s.best()["iteration"] == b
        s.run(c["passes"] - b)
        same(s.best(), record(traj), "the end")


def test_thresholds_and_tracking_in_either_order(gpu):
    c = bc.biased_case()
    want = record(c["traj"][:25])
    for first in ("thresholds", "tracking"):
        with solver(c) as s:
            if first == "thresholds":
                s.set_thresholds(c["thr"])
                s.track_best()
            else:
                s.track_best()
                s.set_thresholds(c["thr"])
            is_empty(s.best(), c["n"])
            s.run(25)
            same(s.best(), want, first + " first")


def test_switching_is_refused_after_the_first_iteration(gpu, native):
    from alllsatisfiabilitysolver_amd import AlllError

    c = bc.main_case()
    with solver(c) as s:  # not tracking: best() is refused, and says why
        with pytest.raises(AlllError) as e:
            s.best()
        assert code_of(e) == native.ALLL_ERR_INVALID_ARG and "track" in str(e.value)
        s.track_best()
        s.track_best(False)  # (off again before the first iteration)
        with pytest.raises(AlllError) as e:
            s.best()
        assert code_of(e) == native.ALLL_ERR_INVALID_ARG
        s.run(3)
        with pytest.raises(AlllError) as e:
            s.track_best()
        assert code_of(e) == native.ALLL_ERR_INVALID_ARG
        with pytest.raises(AlllError):
            s.best()
        s.run(2)
        np.testing.assert_array_equal(s.assignment_words(), c["traj"][5][1])
    with solver(c, track_best=True) as s:
        s.run(3)
        with pytest.raises(AlllError) as e:
            s.track_best(False)
        assert code_of(e) == native.ALLL_ERR_INVALID_ARG
        s.run(2)
        same(s.best(), record(c["traj"][:5]), "still tracking")
        # a wrong word count
        nv, it = ctypes.c_uint64(), ctypes.c_uint64()
        w = np.zeros(8, np.uint32)
        for n_words in (6, 8):
            rc = native.lib().alll_get_best(s._ctx, ctypes.byref(nv), ctypes.byref(it), w.ctypes.data_as(native._u32p), n_words)
            assert rc == native.ALLL_ERR_INVALID_ARG and not w.any()
        assert native.lib().alll_get_best(s._ctx, ctypes.byref(nv), ctypes.byref(it), None, 0) == native.ALLL_OK
        assert (nv.value, it.value) == (record(c["traj"][:5])["n_violated"], record(c["traj"][:5])["iteration"])


@pytest.mark.parametrize("kw, reason", [(dict(flags=REFERENCE_RNG), "REFERENCE_RNG"), (dict(stream_batch=64), "stream")],
                         ids=["reference_rng", "streaming"])
def test_unsupported_contexts(gpu, native, kw, reason):
    """The contexts alll_set_var_thresholds refuses are refused here too, with the reason."""
    from alllsatisfiabilitysolver_amd import AlllError, Solver

    c = bc.main_case()
    with solver(c, **kw) as s:
        with pytest.raises(AlllError) as e:
            s.track_best()
        assert code_of(e) == native.ALLL_ERR_UNSUPPORTED and reason in str(e.value) and "tracking" in str(e.value)
        with pytest.raises(AlllError) as e:
            s.set_thresholds(np.full(c["n"], 1 << 31, np.uint32))
        assert code_of(e) == native.ALLL_ERR_UNSUPPORTED and reason in str(e.value)
        s.run(2)  # (the context works as before)
    with pytest.raises(AlllError) as e:
        Solver(c["n"], c["offs"], c["lits"], seed=c["seed"], track_best=True, **kw)
    assert code_of(e) == native.ALLL_ERR_UNSUPPORTED


def test_unsupported_sharded_contexts(gpu, native):
    """world = 2 over a host exchange (rank 0 of two on one GPU), with and without the allreduce exchange:
    refused before any device work.  (A non-zero comm_id opens an RCCL communicator at create and takes the
    same branch of the helper as world != 1; it is not created here.)"""
    from alllsatisfiabilitysolver_amd import AlllError

    c = bc.main_case()
    for kw, reason in ((dict(world=2, rank=0, flags=ALLREDUCE, exchange=lambda *a: None), "ALLREDUCE"),
                       (dict(world=2, rank=0, exchange=lambda *a: None), "one GPU")):
        with solver(c, **kw) as s:
            with pytest.raises(AlllError) as e:
                s.track_best()
            assert code_of(e) == native.ALLL_ERR_UNSUPPORTED and reason in str(e.value)


# ----------------------------------------------------------------------------- 7. group
def test_group_records_per_item(gpu):
    """7. Five items (1500, 5003, 33, 4097 and 200 variables; the second and third biased).  The last one
    solves at pass 38 while the others go on to the cap; ten more passes follow.  Every item's record
    is the reference's and that of a tracking Solver of its own."""
    from alllsatisfiabilitysolver_amd import AlllError, GroupSolver, Solver

    g = bc.group_case()
    cap, n_items = g["cap"], len(g["items"])
    assert g["solved_at"] == 38 and len(g["trajs"][4]) == 38 < cap
    assert all(record(tr[:cap])["iteration"] != cap for tr in g["trajs"][:4])
    with GroupSolver(g["items"], g["seeds"], max_iters=cap) as s:
        with pytest.raises(AlllError):
            s.best(0)
        for i, thr in enumerate(g["thrs"]):
            if i == 1 and thr is not None:
                s.set_thresholds(i, thr)  # (one before the switch, one after)
        s.track_best()
        if g["thrs"][2] is not None:
            s.set_thresholds(2, g["thrs"][2])
        for i, (n, _, _) in enumerate(g["items"]):
            is_empty(s.best(i), n)
        with pytest.raises(AlllError):
            s.best(n_items)
        res = s.solve()
        assert [r["solved"] for r in res] == [0, 0, 0, 0, 1] and res[4]["n_iterations"] == 38
        assert all(r["n_iterations"] == cap for r in res[:4])
        for i, tr in enumerate(g["trajs"]):
            same(s.best(i), record(tr[:cap]), f"group item {i} at the cap")
        ended = s.best(4)
        assert (ended["n_violated"], ended["iteration"]) == (0, res[4]["n_iterations"])
        np.testing.assert_array_equal(ended["words"], s.assignment_words(4))
        s.run(bc.GROUP_MORE)
        for i, tr in enumerate(g["trajs"]):
            same(s.best(i), record(tr), f"group item {i} after {bc.GROUP_MORE} more passes")
        same(s.best(4), ended, "the solved item")
        with pytest.raises(AlllError):
            s.track_best(False)
    for i, ((n, offs, lits), seed, thr, tr) in enumerate(zip(g["items"], g["seeds"], g["thrs"], g["trajs"])):
        with Solver(n, offs, lits, seed=seed, max_iters=cap, track_best=True) as one:
            if thr is not None:
                one.set_thresholds(thr)
            one.solve()
            same(one.best(), record(tr[:cap]), f"a Solver for item {i} at the cap")
            one.run(bc.GROUP_MORE)
            same(one.best(), record(tr), f"a Solver for item {i} after the run")


# ----------------------------------------------------------------------------- 8. batch
@pytest.mark.parametrize("slice_", [1, 7, 0], ids=["slice1", "slice7", "default_slice"])
def test_batch_records_per_item(gpu, slice_):
    """8. n = 203 under four seeds and the 200-variable item that solves, under three slicings; a
    first_solved solve returns early and a second solve finishes: the records are the reference's."""
    from alllsatisfiabilitysolver_amd import AlllError, BatchSolver

    b = bc.batch_case()
    want = [record(tr) for tr in b["trajs"]]
    assert [len(tr) for tr in b["trajs"]] == [b["cap"]] * 4 + [38]
    with BatchSolver(b["items"], b["seeds"], max_iters=b["cap"]) as s:
        with pytest.raises(AlllError):
            s.best(0)
        s.track_best()
        s.set_slice(slice_)
        for i, (n, _, _) in enumerate(b["items"]):
            is_empty(s.best(i), n)
        res = s.solve(first_solved=True)
        assert res[4]["solved"] and res[4]["n_iterations"] == 38
        for i, tr in enumerate(b["trajs"]):
            k = res[i]["n_iterations"]
            same(s.best(i), record(tr[:k]), f"batch item {i} after the first solve ({k} passes)")
        if slice_:  # (a short slice: the others have not reached the cap yet)
            assert all(r["n_iterations"] < b["cap"] for r in res[:4])
        res = s.solve()
        assert [r["n_iterations"] for r in res] == [b["cap"]] * 4 + [38]
        for i in range(len(want)):
            same(s.best(i), want[i], f"batch item {i}")
        np.testing.assert_array_equal(s.best(4)["words"], s.assignment_words(4))
        with pytest.raises(AlllError):
            s.track_best(False)
        with pytest.raises(AlllError):
            s.best(len(want))


def test_batch_records_match_a_solver_per_item(gpu):
    from alllsatisfiabilitysolver_amd import Solver

    b = bc.batch_case()
    for i, ((n, offs, lits), seed, tr) in enumerate(zip(b["items"], b["seeds"], b["trajs"])):
        with Solver(n, offs, lits, seed=seed, max_iters=b["cap"], track_best=True) as one:
            one.solve()
            same(one.best(), record(tr), f"a Solver for batch item {i}")
