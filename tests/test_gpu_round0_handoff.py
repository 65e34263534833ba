"""The bucketed LFMIS round 0 hands its run layout from the scatter to the join: the fused
evaluation kernel takes a run's tile counts from its own LDS counters, the scatter writes one
record per run (entries, pairs, prefix of the tile counts) and k_bjoin reads that record instead
of deriving it again; pairs move 16 bytes at a time.  Every case below runs six iterations with
the bucketed round 0 forced (ALLL_BUCKET_MIN_U=0) and compares the statistics, the assignment
(words and digest), mis() and violated_mask() with the oracle after every iteration.

The shapes are the smallest at which those paths differ:
  two_tiles         5,000 clauses: two evaluation workgroups of one tile each, two one-tile runs
  empty_first_tile  one workgroup, one run of three tiles whose first tile has no violated clause
                    in the first iteration: a prefix with a zero inside
  one_wg            1.1M clauses in one evaluation workgroup (ALLL_PLAN_CUS=1): 269 tiles, so two
                    passes of the per-tile LDS counters and 17 runs; the runs of the first pass read
                    their counts back from memory, the last run starts in the first pass; a run
                    holds ~8k entries and ~24k pairs: several sweeps, pairs not staged in LDS
  two_wgs           the same in two workgroups: nine runs each, one pass, the last run of each at
                    an offset inside the LDS counters
  one_wg_bscatter   one_wg with the stand-alone scatter kernel (ALLL_FUSE_SCATTER=0), which must
                    write the record that the join reads
  hot               power-law 3-SAT, 200k clauses: 26 hot variables (claims through the LDS hash
                    table and the owner keys) next to bucketed pairs; with its hubs flagged hot the
                    remaining pair load is not skewed, so the planner does bucket this instance
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 6
TILE = 4096
SEED = 11
BIG = (275_000, 1_100_000, 3, 0)
CASES = {
    "two_tiles": ("two_tiles", {}),
    "empty_first_tile": ("empty_first_tile", {"ALLL_PLAN_CUS": "1"}),
    "one_wg": ("big", {"ALLL_PLAN_CUS": "1"}),
    "two_wgs": ("big", {"ALLL_PLAN_CUS": "2"}),
    "one_wg_bscatter": ("big", {"ALLL_PLAN_CUS": "1", "ALLL_FUSE_SCATTER": "0"}),
    "hot": ("hot", {}),
}


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def first_tile_clauses(offs, lits):
    """Clauses that may lie in the first evaluation tile: the first TILE in clause order and the
    first TILE in the planner's order of a fixed-width instance without windows (by largest, then
    second largest variable, then id)."""
    m = offs.size - 1
    v = np.sort(lits.reshape(m, 3) >> 1, axis=1)
    ids = np.arange(m)
    return np.union1d(ids[:TILE], ids[np.lexsort([ids, v[:, 1], v[:, 2]])][:TILE])


def make_instance(o, name):
    from alllsatisfiabilitysolver_amd import generate_ksat

    if name == "two_tiles":
        n = 1250
        return (n,) + generate_ksat(1, n, 5000, 3, 0)
    if name == "big":
        return (BIG[0],) + generate_ksat(1, *BIG)
    if name == "hot":
        n = 50_000
        return (n,) + generate_ksat(1, n, 200_000, 3, 1)
    assert name == "empty_first_tile"
    # three tiles; every clause of the first tile is satisfied by the seed's initial assignment:
    # a violated one has the sign of its first literal flipped
    n, m = 3000, 12000
    offs, lits = generate_ksat(1, n, m, 3, 0)
    lits = lits.copy()
    first = first_tile_clauses(offs, lits)
    A0 = o.init_assignment(SEED, n)
    _, vm = o.eval_mask(offs, lits, A0)
    viol = np.intersect1d(o.mask_to_list(m, vm), first)
    lits[3 * viol.astype(np.int64)] ^= 1
    nu, vm = o.eval_mask(offs, lits, A0)
    U = o.mask_to_list(m, vm)
    assert np.intersect1d(U, first_tile_clauses(offs, lits)).size == 0 and nu > 0
    return n, offs, lits


_REF = {}


def reference(o, name):
    """(instance, [(|U|, mask, MIS, resampled literals, A after)] of ITERS iterations): computed
    once per instance and shared by the cases that run it."""
    if name not in _REF:
        n, offs, lits = make_instance(o, name)
        m = offs.size - 1
        _, _, rows = o.solve(n, offs, lits, SEED, max_iters=ITERS + 2, trace=True)
        assert len(rows) >= ITERS
        A = o.init_assignment(SEED, n)
        steps = []
        for it in range(ITERS):
            nu, vm = o.eval_mask(offs, lits, A)
            M = o.lfmis(n, offs, lits, o.mask_to_list(m, vm))
            A = o.resample_words(A.copy(), SEED, it, o.clause_vars(offs, lits, M))
            assert (nu, M.size) == rows[it][1:3] and np.array_equal(A, rows[it][4])  # (the oracle's two routes agree)
            assert nu > 0
            for x in (vm, M, A):
                x.setflags(write=False)
            steps.append((nu, vm, M, rows[it][3], A))
        _REF[name] = ((n, offs, lits), steps)
    return _REF[name]


@pytest.mark.parametrize("case", list(CASES))
def test_round0_handoff_matches_oracle(gpu, oracle_mod, case, monkeypatch):
    from alllsatisfiabilitysolver_amd import Solver, assignment_digest

    name, env = CASES[case]
    (n, offs, lits), steps = reference(oracle_mod, name)
    m = offs.size - 1
    monkeypatch.setenv("ALLL_BUCKET_MIN_U", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Solver(n, offs, lits, seed=SEED) as s:
        np.testing.assert_array_equal(s.assignment_words(), oracle_mod.init_assignment(SEED, n))
        for it, (nu, vm, M, dres, A_after) in enumerate(steps):
            before = s.stats()
            s.run(1)
            after = s.stats()
            assert after["n_violated"] == nu, f"iteration {it}"
            assert after["sum_mis_size"] - before["sum_mis_size"] == M.size, f"iteration {it}"
            assert after["n_resamples"] - before["n_resamples"] == dres, f"iteration {it}"
            np.testing.assert_array_equal(s.violated_mask(), vm[: (m + 63) // 64], err_msg=f"mask, iteration {it}")
            np.testing.assert_array_equal(s.mis(), M, err_msg=f"MIS, iteration {it}")
            words = s.assignment_words()
            assert assignment_digest(words) == assignment_digest(A_after), f"iteration {it}"
            np.testing.assert_array_equal(words, A_after, err_msg=f"assignment, iteration {it}")
