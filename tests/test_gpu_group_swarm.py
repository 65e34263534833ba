"""Groups past one workgroup of items on the GPU: a thousand tiny items in one group,
130 items in lock step with 64 distinct items per wave, a bag of structured conflict graphs, all with
seeds whose high word is the one that differs.  Every item is compared bit for bit, at every checked
step, with the oracle's run of the item alone at the item's seed (tests/swarm_cases.py, whose facts
tests/test_swarm_cases.py pins on the CPU).  The statistics come from the list run() / solve() return
(one read for all items), the assignments per item."""
import numpy as np
import pytest

import swarm_cases as sc
from best_cases import EMPTY, record
from swarm_cases import CAP, N_SWARM, THR_STEPS
from test_gpu_group import NO_GRAPH, STAT_KEYS, oracle_stats
from test_gpu_parity import LAYOUTS

pytestmark = pytest.mark.gpu

GENERIC_CSR = 1 << 2


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


def same_words(got, want, what):
    if not np.array_equal(got, want):
        np.testing.assert_array_equal(got, want, err_msg=what)


def check_wants(g, res, wants, what):
    """Every item: the statistics of res (the list run() returned) and the assignment words."""
    assert len(res) == len(wants)
    for i, (want, A) in enumerate(wants):
        assert {k: res[i][k] for k in want} == want, (what, i)
        same_words(g.assignment_words(i), A, f"{what}: item {i}")


def check_steps(g, res, traces, steps, what):
    check_wants(g, res, [t.after(steps) for t in traces], f"{what} after {steps} iterations")


def check_solved(g, res, traces, native, what):
    """Every item after a solve() under the traces' cap: statistics, status and assignment."""
    assert len(res) == len(traces)
    for i, t in enumerate(traces):
        assert {k: res[i][k] for k in STAT_KEYS} == oracle_stats(t.st), (what, i)
        assert res[i]["status"] == (native.ALLL_OK if t.st["solved"] else native.ALLL_ERR_MAX_ITERS), (what, i)
        assert res[i]["gpu_resamples"] == [t.st["n_resamples"]], (what, i)
        same_words(g.assignment_words(i), t.A, f"{what}: item {i}")


def check_records(g, trajs, passes, what):
    """Every item's record after the group has made `passes` passes (an ended item: its own)."""
    for i, tr in enumerate(trajs):
        got, want = g.best(i), record(tr[:passes])
        assert (got["n_violated"], got["iteration"]) == (want["n_violated"], want["iteration"]), (what, i)
        same_words(got["words"], want["words"], f"{what}: record of item {i}")


# ----------------------------------------------------------------------------- a. steps
@pytest.mark.parametrize("fixed", [False, True], ids=["ragged", "fixed"])
def test_swarm_steps(gpu, native, oracle_mod, fixed):
    """a. Eight single steps of the thousand items (group_finish takes its stride four times, its last
    trip ragged; wave merges of dozens of items; runs across items inside a mask word; the empty clauses
    in the MIS), then a fresh group solved under max_iters = 12, and a second solve that changes nothing."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.swarm_case(fixed)
    items, seeds, traces = c["items"], c["seeds"], c["traces"]
    with GroupSolver(items, seeds) as g:
        assert g.layout() == (3 if fixed else 0)
        for i, t in enumerate(traces):
            same_words(g.assignment_words(i), t.A0, f"initial assignment, item {i}")
        for step in range(1, 9):
            check_steps(g, g.run(1), traces, step, "run(1)")
    with GroupSolver(items, seeds, max_iters=CAP) as g:
        res = g.solve()
        check_solved(g, res, traces, native, "solve")
        again = g.solve()
        keys = STAT_KEYS + ("status",)
        assert [{k: r[k] for k in keys} for r in again] == [{k: r[k] for k in keys} for r in res]
        check_solved(g, again, traces, native, "second solve")


# ----------------------------------------------------------------------------- b. variants
@pytest.mark.parametrize("variant", ["csr", "fixed", "positions", "buckets", "atomic_claims", "no_graph"])
def test_swarm_variants(gpu, oracle_mod, variant, monkeypatch):
    """b. The fixed swarm under the layouts (k_group_account with and without the evaluation order's
    permutation), the bucketed LFMIS, the atomic claims and eager launches: four steps, then run(4)."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.swarm_case(True)
    flags, env = (NO_GRAPH, {}) if variant == "no_graph" else LAYOUTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with GroupSolver(c["items"], c["seeds"], flags=flags) as g:
        assert g.layout() == (0 if variant == "csr" else 3)
        for step in range(1, 5):
            check_steps(g, g.run(1), c["traces"], step, variant)
        check_steps(g, g.run(4), c["traces"], 8, f"{variant}, run(4)")


# ----------------------------------------------------------------------------- c. item counts
@pytest.mark.parametrize("n", [255, 256, 257, 513, 1000])
def test_item_count_boundary(gpu, native, oracle_mod, n):
    """c. The first n items of the ragged swarm: one short of a workgroup of items, exactly one, one over,
    two strides plus one, and the ragged last workgroup.  run(3), then a fresh group solved under
    max_iters = 6."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.swarm_case()
    items, seeds = c["items"][:n], c["seeds"][:n]
    with GroupSolver(items, seeds) as g:
        check_steps(g, g.run(3), c["traces"][:n], 3, f"{n} items, run(3)")
    with GroupSolver(items, seeds, max_iters=6) as g:
        check_solved(g, g.solve(), sc.swarm_traces_capped(6)[:n], native, f"{n} items, solve")


# ----------------------------------------------------------------------------- d. lock step
@pytest.mark.parametrize("flags", [0, GENERIC_CSR], ids=["default", "generic_csr"])
def test_lockstep(gpu, oracle_mod, flags):
    """d. 130 items of 64 copies of one clause from all-false.  Pass 1: every item has 64 violated clauses,
    one MIS clause, three resamples; in clause order wave 0 of a full tile merges 64 distinct items and
    the tile's MIS list holds one clause of each of 64 items.  Four more steps against the traces; the
    same with tracking, where every item's record after pass 1 is {64, 1, all-false}."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.lockstep_case()
    n = len(c["items"])
    trajs = sc.lockstep_trajectories()
    for track in (False, True):
        with GroupSolver(c["items"], c["seeds"], flags=flags) as g:
            assert g.layout() == (0 if flags else 3)
            if track:
                g.track_best()
            for i, A0 in enumerate(c["A0s"]):
                g.set_assignment_words(i, A0)
            res = g.run(1)
            assert [(r["n_iterations"], r["n_violated"], r["sum_mis_size"], r["n_resamples"], r["solved"])
                    for r in res] == [(1, 64, 1, 3, 0)] * n
            check_steps(g, res, c["traces"], 1, "lock step")
            if track:
                for i in range(n):
                    b = g.best(i)
                    assert (b["n_violated"], b["iteration"]) == (64, 1) and not b["words"].any(), i
            for step in range(2, 6):
                check_steps(g, g.run(1), c["traces"], step, "lock step")
                if track:
                    check_records(g, trajs, step, f"lock step, pass {step}")


# ----------------------------------------------------------------------------- e. records
def test_swarm_records(gpu, native, oracle_mod):
    """e. Tracking on the ragged swarm (k_group_best on four workgroups, the last one ragged; one-word
    items, whose flags neighbouring lanes load from 32 different entries): run(5), run(1) and a solve to
    max_iters = 12, every item's record after each; statistics and assignments as without tracking."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.swarm_case()
    traces, trajs = c["traces"], sc.swarm_trajectories()
    with GroupSolver(c["items"], c["seeds"], max_iters=CAP) as g:
        g.track_best()
        got = g.best(0)
        assert (got["n_violated"], got["iteration"]) == (EMPTY["n_violated"], 0)
        check_steps(g, g.run(5), traces, 5, "tracking, run(5)")
        check_records(g, trajs, 5, "after run(5)")
        check_steps(g, g.run(1), traces, 6, "tracking, run(1)")
        check_records(g, trajs, 6, "after run(1)")
        check_solved(g, g.solve(), traces, native, "tracking, solve")
        check_records(g, trajs, CAP, "after solve")
        for i, (n, offs, _) in enumerate(c["items"]):
            if offs.size == 1:  # no clause: the first pass is the record, on the initial words
                b = g.best(i)
                assert (b["n_violated"], b["iteration"]) == (0, 1), i
                same_words(b["words"], traces[i].A0, f"record of clauseless item {i}")


# ----------------------------------------------------------------------------- f. thresholds
@pytest.mark.parametrize("track", [False, True], ids=["plain", "track_best"])
def test_swarm_thresholds(gpu, oracle_mod, track):
    """f. Thresholds with pins on every third item of the ragged swarm: 32 one-word items share a word of
    the per-word bits, biased and unbiased ones mixed.  Six steps: the biased items against
    bias_cases.reference, the others against their unbiased traces; with tracking
    (k_group_resample_biased_best) every item's record as well."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c, t = sc.swarm_case(), sc.thresholds_case()
    with GroupSolver(c["items"], c["seeds"]) as g:
        if track:
            g.track_best()
        for i, thr in enumerate(t["thrs"]):
            if thr is not None:
                g.set_thresholds(i, thr)
        for i, tr in enumerate(c["traces"]):
            same_words(g.assignment_words(i), tr.A0 if t["refs"][i] is None else t["refs"][i][0], f"fill, item {i}")
        for step in range(1, THR_STEPS + 1):
            check_wants(g, g.run(1), sc.wants_after(c, step, t["refs"]), f"thresholds, step {step}")
            if track:
                check_records(g, t["trajs"], step, f"thresholds, pass {step}")


# ----------------------------------------------------------------------------- g. first solved
def test_first_solved_among_many(gpu, native, oracle_mod):
    """g. The fixed swarm's items that have clauses under one max_iters: first_solved returns with the
    oracle's winner (fewest iterations, lowest index on a tie -- several items tie at pass 1), everybody
    else on their own trajectory; a plain solve() then ends as a fresh full solve."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.swarm_case(True)
    keep = [i for i, it in enumerate(c["items"]) if it[1].size > 1]
    items, seeds, traces = [c["items"][i] for i in keep], [c["seeds"][i] for i in keep], [c["traces"][i] for i in keep]
    assert 700 <= len(keep) < N_SWARM - 152  # (the three runs of clauseless items, and every i % 11 == 0)
    iters = [t.st["n_iterations"] if t.st["solved"] else None for t in traces]
    winner = min((i for i, k in enumerate(iters) if k), key=lambda i: (iters[i], i))
    assert sum(1 for k in iters if k == iters[winner]) >= 3 and sum(1 for k in iters if k == 2) >= 3
    with GroupSolver(items, seeds, max_iters=CAP) as g:
        res = g.solve(first_solved=True)
        solved = [i for i, r in enumerate(res) if r["solved"]]
        assert solved and min(solved, key=lambda i: (res[i]["n_iterations"], i)) == winner
        passes = max(r["n_iterations"] for r in res)
        for i, (r, t) in enumerate(zip(res, traces)):
            assert r["solved"] == int(iters[i] is not None and iters[i] <= passes), i
            want, A = t.after(passes)
            assert {k: r[k] for k in want} == want, i
            same_words(g.assignment_words(i), A, f"first_solved: item {i}")
        check_solved(g, g.solve(), traces, native, "after first_solved")


# ----------------------------------------------------------------------------- h. structures
def test_structures_bag(gpu, oracle_mod):
    """h. Three random items, then a hub of degree 2000 at union variable 6048, 300 copies of a clause, a
    dense item and chain(513), all from all-false: three single steps, then run(6)."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    c = sc.bag_case()
    with GroupSolver(c["items"], c["seeds"]) as g:
        for i, A0 in enumerate(c["A0s"]):
            g.set_assignment_words(i, A0)
        for step in range(1, 4):
            check_steps(g, g.run(1), c["traces"], step, "structures")
        check_steps(g, g.run(6), c["traces"], 9, "structures, run(6)")


# ----------------------------------------------------------------------------- i. no clause at all
def test_all_items_clauseless(gpu, oracle_mod):
    """i. 300 items of 1 to 65 variables and no clause: one pass, every item solved at n_iterations = 1, the
    assignments the initial fills of the items' own 64-bit seeds."""
    from alllsatisfiabilitysolver_amd import GroupSolver

    ns = [1 + i % 65 for i in range(300)]
    seeds = [sc.swarm_seed(3000 + i) for i in range(300)]
    with GroupSolver([(n, *sc.NO_CLAUSE) for n in ns], seeds) as g:
        res = g.run(1)
        for extra in (0, 1):  # (a second pass counts nothing)
            assert [(r["n_iterations"], r["n_violated"], r["sum_mis_size"], r["n_resamples"], r["solved"])
                    for r in res] == [(1, 0, 0, 0, 1)] * 300
            for i, (n, s) in enumerate(zip(ns, seeds)):
                same_words(g.assignment_words(i), oracle_mod.init_assignment(s, n), f"clauseless item {i}")
            if not extra:
                res = g.run(1)
