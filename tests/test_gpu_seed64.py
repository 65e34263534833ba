"""Seeds with a high word on the GPU.  The high key word travels separately everywhere on the device
(k1 = seed >> 32 in the fill, the resample, the allreduce delta and the batch kernel), and every other
GPU test uses a seed below 2^32: a kernel that dropped or swapped the high word would pass them all.
Every case here first asserts on the CPU that the reference's trajectory differs from that of the low
word alone, then compares the GPU with the reference bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import bias_cases
import swarm_cases as sc
from best_cases import record, trajectory

pytestmark = pytest.mark.gpu

SEEDS = [(7 << 32) | 5, 0xFFFFFFFF00000000]
LOW = 0xFFFFFFFF
K = 6
KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "solved")
seeds = pytest.mark.parametrize("seed", SEEDS, ids=["7_5", "ffffffff_0"])


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


@functools.lru_cache(maxsize=None)
def instance():
    """n = 2000, m = 8000: not solved within the steps here."""
    from alllsatisfiabilitysolver_amd import generate_ksat

    return (2000, *generate_ksat(1, 2000, 8000, 3))


def differs(run):
    """The reference run at the seed and at its low word alone: different first and last assignments."""
    (full, low) = run
    assert full[2] and low[2]
    assert not np.array_equal(full[2][0][4], low[2][0][4]) and not np.array_equal(full[1], low[1])


def follow_rows(s, rows, what, stream=False):
    """Every run(1) against the oracle's rows (it, |U|, |M|, resamples, assignment after).  stream: the
    streaming solve sums the MIS size after every batch, so the MIS itself is counted."""
    for it, nu, nm, dres, A_after in rows:
        before = s.stats()
        after = s.run(1)
        assert after["n_violated"] == nu and (stream or after["n_iterations"] == it), (what, it)
        assert (s.mis().size if stream else after["sum_mis_size"] - before["sum_mis_size"]) == nm, (what, it)
        assert after["n_resamples"] - before["n_resamples"] == dres, (what, it)
        np.testing.assert_array_equal(s.assignment_words(), A_after, err_msg=f"{what}: after iteration {it}")


def check_solve(s, st_o, A_o, what):
    st = s.solve()
    assert {k: st[k] for k in KEYS} == {k: st_o[k] for k in KEYS}, what
    np.testing.assert_array_equal(s.assignment_words(), A_o, err_msg=what)


@seeds
@pytest.mark.parametrize("T", [1, 4])
def test_solver(gpu, oracle_mod, seed, T):
    """Solver at T = 1 (the fill and k_resample_vars) and under the round robin of four sets."""
    from alllsatisfiabilitysolver_amd import Solver

    o, (n, offs, lits) = oracle_mod, instance()
    full, low = (o.solve(n, offs, lits, s, max_iters=K, trace=True, T=T) for s in (seed, seed & LOW))
    differs((full, low))
    assert not np.array_equal(o.init_assignment(seed, n), o.init_assignment(seed & LOW, n))
    with Solver(n, offs, lits, seed=seed, n_threads=T) as s:
        np.testing.assert_array_equal(s.assignment_words(), o.init_assignment(seed, n))
        follow_rows(s, full[2], f"T = {T}")
    with Solver(n, offs, lits, seed=seed, n_threads=T, max_iters=K) as s:
        check_solve(s, full[0], full[1], f"T = {T}, solve")


@seeds
def test_streaming_solver(gpu, oracle_mod, seed):
    """Solver(stream_batch = 64) against the oracle's streaming solve."""
    from alllsatisfiabilitysolver_amd import Solver

    o, (n, offs, lits) = oracle_mod, instance()
    full, low = (o.solve_stream(n, offs, lits, s, 64, max_iters=K, trace=True) for s in (seed, seed & LOW))
    differs((full, low))
    with Solver(n, offs, lits, seed=seed, stream_batch=64) as s:
        follow_rows(s, full[2], "stream", stream=True)
    with Solver(n, offs, lits, seed=seed, stream_batch=64, max_iters=K) as s:
        check_solve(s, full[0], full[1], "stream, solve")


@functools.lru_cache(maxsize=None)
def biased_case(seed):
    import oracle as o

    n, offs, lits, _, thr = bias_cases._small_instance()
    return n, offs, lits, thr, bias_cases.reference(o, n, offs, lits, seed, thr, 4)


@seeds
def test_solver_with_thresholds(gpu, oracle_mod, seed):
    """n = 5003 (two workgroups of k_resample_biased, the biased fill) against bias_cases.reference."""
    from alllsatisfiabilitysolver_amd import Solver

    n, offs, lits, thr, (A0, rows) = biased_case(seed)
    A0_low, rows_low = biased_case(seed & LOW)[4]
    assert not np.array_equal(A0, A0_low) and not np.array_equal(rows[-1][4], rows_low[-1][4])
    assert len(rows) == 4 and rows[-1][1] > 0
    with Solver(n, offs, lits, seed=seed) as s:
        s.set_thresholds(thr)
        bias_cases.follow(s, A0, rows, "thresholds")


@seeds
def test_solver_track_best(gpu, oracle_mod, seed):
    """The record of a tracking Solver (k_resample_vars_best) after every pass."""
    from alllsatisfiabilitysolver_amd import Solver

    o, (n, offs, lits) = oracle_mod, instance()
    traj, traj_low = (trajectory(o, n, offs, lits, s, K) for s in (seed, seed & LOW))
    assert [u for u, _ in traj] != [u for u, _ in traj_low] and len(traj) == K
    with Solver(n, offs, lits, seed=seed, track_best=True) as s:
        for p in range(1, K + 1):
            s.run(1)
            got, want = s.best(), record(traj[:p])
            assert (got["n_violated"], got["iteration"]) == (want["n_violated"], want["iteration"]), p
            np.testing.assert_array_equal(got["words"], want["words"], err_msg=f"record after pass {p}")


@seeds
def test_rccl_one_rank_allreduce(gpu, native, oracle_mod, seed):
    """The allreduce exchange over a one-rank RCCL communicator: k_resample_delta draws per clause
    (delta_clause) with the key handed in as two words."""
    from alllsatisfiabilitysolver_amd import Solver, comm_unique_id

    o, (n, offs, lits) = oracle_mod, instance()
    full, low = (o.solve(n, offs, lits, s, max_iters=K, trace=True) for s in (seed, seed & LOW))
    differs((full, low))
    with Solver(n, offs, lits, seed=seed, device=0, rank=0, world=1, comm_id=comm_unique_id(),
                flags=native.FLAG_EXCHANGE_ALLREDUCE) as s:
        assert s.comm_size() == 1
        for it, _, _, _, A_after in full[2]:
            s.run(1)
            np.testing.assert_array_equal(s.assignment_words(), A_after, err_msg=f"allreduce: after iteration {it}")
        assert s.stats()["n_resamples"] == sum(r[3] for r in full[2])


BATCH_SEEDS = [(7 << 32) | 5, (9 << 32) | 5, 0xFFFFFFFF00000000, 1 << 32]  # two pairs equal in the low word
BATCH_STEPS = 8


@functools.lru_cache(maxsize=None)
def batch_case():
    """Four items of one instance (n = 203, m = 812); the second one has thresholds."""
    import oracle as o
    from alllsatisfiabilitysolver_amd import generate_ksat

    item = (203, *generate_ksat(7, 203, 812, 3))
    thrs = [None, bias_cases.mixed_thresholds(203, 9), None, None]
    refs = [bias_cases.unbiased_reference(o, *item, s, BATCH_STEPS) if t is None
            else bias_cases.reference(o, *item, s, t, BATCH_STEPS) for s, t in zip(BATCH_SEEDS, thrs)]
    return item, thrs, refs


@pytest.mark.parametrize("slice_", [1, 0], ids=["slice1", "default_slice"])
def test_batch_solver(gpu, oracle_mod, slice_):
    """BatchSolver (the batch kernel's own fill and resample): per item the oracle's run at its seed."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    item, thrs, refs = batch_case()
    for a, b in ((0, 1), (2, 3)):
        assert BATCH_SEEDS[a] & LOW == BATCH_SEEDS[b] & LOW
    assert not np.array_equal(refs[2][0], refs[3][0])  # unbiased, one low word: the fills differ
    assert not np.array_equal(refs[2][1][-1][4], refs[3][1][-1][4])
    assert not np.array_equal(refs[0][0], oracle_mod.init_assignment(BATCH_SEEDS[0] & LOW, item[0]))
    assert all(len(rows) == BATCH_STEPS and rows[-1][1] > 0 for _, rows in refs)
    with BatchSolver([item] * 4, BATCH_SEEDS) as b:
        b.set_thresholds(1, thrs[1])
        b.set_slice(slice_)
        for i, (A0, _) in enumerate(refs):
            np.testing.assert_array_equal(b.assignment_words(i), A0, err_msg=f"fill, item {i}")
        done = 0
        for k in (1, 3, 4):
            res = b.run(k)
            done += k
            for i, (A0, rows) in enumerate(refs):
                want, A = sc.rows_after(A0, rows, done)
                assert {key: res[i][key] for key in want} == want, (i, done)
                np.testing.assert_array_equal(b.assignment_words(i), A, err_msg=f"item {i} after {done} iterations")


@seeds
@pytest.mark.parametrize("n", [1, 33, 5003])
def test_host_fills_equal_the_device_fills(gpu, native, oracle_mod, seed, n):
    """alll_initial_assignment and alll_biased_initial_assignment (host helpers) against the device's
    fill for the same seed, and both against the oracle's."""
    from alllsatisfiabilitysolver_amd import Solver, biased_initial_assignment

    o = oracle_mod
    offs, lits = np.array([0, 1], np.uint64), np.array([0], np.uint32)
    host = np.zeros(n, np.uint8)
    native.check(native.lib().alll_initial_assignment(seed, n, host.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "fill")
    thr = bias_cases.mixed_thresholds(n, 4)
    with Solver(n, offs, lits, seed=seed) as s:
        np.testing.assert_array_equal(s.assignment(), host)
        np.testing.assert_array_equal(s.assignment_words(), o.init_assignment(seed, n))
        s.set_thresholds(thr)
        np.testing.assert_array_equal(s.assignment(), biased_initial_assignment(seed, n, thr))
        np.testing.assert_array_equal(s.assignment_words(), bias_cases.biased_init(o, seed, n, thr))
    if n >= 33:
        assert not np.array_equal(o.init_assignment(seed, n), o.init_assignment(seed & LOW, n))
        assert not np.array_equal(bias_cases.biased_init(o, seed, n, thr), bias_cases.biased_init(o, seed & LOW, n, thr))
