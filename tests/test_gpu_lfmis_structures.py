"""The one-instance LFMIS (T = 1: bucketed or atomic round 0, k_wclaim / k_wjoin, the
one-workgroup k_tail, the ALLL_SMALL_U variant, the hot table) on crafted conflict graphs whose
exact MIS and dependency depth are known (tests/lfmis_structures.py; the CPU side is
tests/test_lfmis_structures.py), bit-exact against the oracle under every layout that changes
the LFMIS.

Random instances settle in a handful of rounds; these need up to 10000 dependent rounds in one
iteration (chains), keep long lists live for 150 rounds (combs), hand a large survivor list to
the tail (wide combs), or put thousands of claims on one address at the hot-table thresholds
(stars, dense, copies).
"""
import functools

import numpy as np
import pytest

from lfmis_structures import DEEP, STRUCTURES, all_false, structure
from test_gpu_parity import LAYOUTS, gpu, make_solver  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu

SEED, K = 12345, 12
LFMIS_LAYOUTS = ["hybrid", "fixed", "csr", "atomic_claims", "buckets", "bscatter", "positions", "tail_all",
                 "no_small_u"]
assert all(k in LAYOUTS for k in LFMIS_LAYOUTS + ["small_windows"])


def _cases():
    out = []
    for name in STRUCTURES:
        if name == "star513hubs":  # the one big instance
            lays = ["hybrid", "atomic_claims", "buckets"]
        else:
            lays = LFMIS_LAYOUTS + (["small_windows"] if name in ("chain20000", "star20000", "star20000x7") else [])
        out += [(name, lay) for lay in lays]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    """Oracle values of one structure, computed once and shared by every layout: the three map
    steps from all-false (iteration indices 0, 1, 2), the K-iteration trace and the final
    state of the free run."""
    import oracle as o

    n, offs, lits = structure(name)
    m = offs.size - 1
    A0 = all_false(n)
    nu, vm = o.eval_mask(offs, lits, A0)
    M = o.lfmis(n, offs, lits, o.mask_to_list(m, vm))
    assert (nu, M.size) == STRUCTURES[name][2]
    dres = int((offs[M.astype(np.int64) + 1] - offs[M.astype(np.int64)]).sum())
    mv = o.clause_vars(offs, lits, M)
    steps = [o.resample_words(A0.copy(), SEED, it, mv) for it in range(3)]
    st_o, A_o, rows = o.solve(n, offs, lits, SEED, max_iters=K, A0=A0, trace=True)
    return dict(nu=nu, vm=vm[: max(1, (m + 63) // 64)], M=M, dres=dres, steps=steps, st=st_o, A=A_o, rows=rows)


def map_steps(s, e, n):
    """Three times: impose all-false, run one iteration; mask, MIS, statistics deltas and the
    resampled assignment are the oracle's.  Re-imposing the assignment makes the steps
    independent of the seed's draws and drives the same deep set through the launch variants
    of iterations > 0."""
    for it in range(3):
        s.set_assignment_words(all_false(n))
        before = s.stats()
        s.run(1)
        after = s.stats()
        assert after["n_violated"] == e["nu"], f"step {it}"
        np.testing.assert_array_equal(s.violated_mask(), e["vm"], err_msg=f"U, step {it}")
        np.testing.assert_array_equal(s.mis(), e["M"], err_msg=f"M, step {it}")
        assert after["sum_mis_size"] - before["sum_mis_size"] == e["M"].size, f"step {it}"
        assert after["n_resamples"] - before["n_resamples"] == e["dres"], f"step {it}"
        np.testing.assert_array_equal(s.assignment_words(), e["steps"][it], err_msg=f"A after step {it}")


def free_run(make, e, n):
    """K iterations from all-false, every one against the oracle's trace; then one solve()."""
    with make() as s:
        s.set_assignment_words(all_false(n))
        for it, nu, nm, dres, A_after in e["rows"]:
            before = s.stats()
            s.run(1)
            after = s.stats()
            assert after["n_violated"] == nu, f"iter {it}"
            assert after["sum_mis_size"] - before["sum_mis_size"] == nm, f"iter {it}"
            assert after["n_resamples"] - before["n_resamples"] == dres, f"iter {it}"
            np.testing.assert_array_equal(s.assignment_words(), A_after, err_msg=f"A after iter {it}")
    with make(max_iters=K) as s:
        s.set_assignment_words(all_false(n))
        st = s.solve()
        for k in ("n_iterations", "n_resamples", "avg_mis_size", "sum_mis_size", "solved"):
            assert st[k] == e["st"][k], k
        np.testing.assert_array_equal(s.assignment_words(), e["A"])


@pytest.mark.parametrize("name,layout", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_structure_matches_oracle(gpu, oracle_mod, name, layout, monkeypatch):
    """Map steps and free run of one structure under one layout.

    Coverage guard (chains and combs): lfmis_rounds_max >= the claim rounds of the instance
    (claim_rounds, pinned on the CPU).  If a later algorithm settles a chain in fewer rounds
    this assertion fails: the instance then no longer drives the tail through its deep rounds
    and must be replaced by one that does.  No upper bound: the tail kills dead clauses one
    round after the join that covered them."""
    n, offs, lits = structure(name)
    e = expected(name)

    def make(**kw):
        return make_solver(layout, monkeypatch, n, offs, lits, seed=SEED, **kw)

    with make() as s:
        map_steps(s, e, n)
        if name in DEEP:
            assert s.stats()["lfmis_rounds_max"] >= STRUCTURES[name][3]
    free_run(make, e, n)


@pytest.mark.parametrize("grid_rounds", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["chain4097", "combs64x300"])
def test_grid_round_split_on_deep_sets(gpu, oracle_mod, name, grid_rounds, monkeypatch):
    """The split between grid rounds and the tail on a deep set, round 0 bucketed (including
    the last-round hand-off at one grid round)."""
    from alllsatisfiabilitysolver_amd import Solver

    n, offs, lits = structure(name)
    e = expected(name)
    monkeypatch.setenv("ALLL_BUCKET_MIN_U", "0")

    def make(**kw):
        return Solver(n, offs, lits, seed=SEED, grid_rounds=grid_rounds, **kw)

    with make() as s:
        map_steps(s, e, n)
    free_run(make, e, n)
