"""The two ends of the owner epochs ("Tests at the epochs' ends"), bit-exact
against the oracle after every iteration: assignment, violated count, MIS, statistics deltas.

  * Round robin, fixpoint passes: the epoch budget of the claim keys is 2^31 - 1 at every size the
    rest of the suite uses, so the owner-epoch restart (k_fp_guess clears fp_owner) and the
    FP_FAIL of an iteration whose epochs ran out never happen there.  ALLL_RR_EP_BUDGET caps the
    budget so that 2,000-clause instances do both.
  * One-set loop (T = 1, groups): 32-bit epochs.  ALLL_EPOCH0 starts them just under 2^32, so
    that a 60-iteration run crosses the point where k_tail clears the owner keys and starts the
    epochs over.

Every case asserts on Solver.epoch_counters() that the path it names ran: the trajectory is the
same whether or not it did.
"""
import functools

import numpy as np
import pytest

import bias_cases as bc
from lfmis_structures import all_false, structure

pytestmark = pytest.mark.gpu

KNOBS = ("ALLL_RR_EP_BUDGET", "ALLL_EPOCH0", "ALLL_RR_INC", "ALLL_RR_REP_CAP", "ALLL_RR_FP", "ALLL_RR_FP_MAX",
         "ALLL_SMALL_U", "ALLL_BUCKET_MIN_U")


@pytest.fixture(scope="module")
def gpu(native, oracle_mod):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def make(monkeypatch, env, n, offs, lits, **kw):
    """A Solver created under the knobs of env (read at create), which are unset again after."""
    from alllsatisfiabilitysolver_amd import Solver

    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    s = Solver(n, offs, lits, **kw)
    for k in env:
        monkeypatch.delenv(k)
    return s


@functools.lru_cache(maxsize=None)
def reference(key, T, seed, K, from_false=False):
    """The oracle's K iterations (or to the solve) of instance `key` under T sets, once for every
    budget / epoch start: rows (|U|, sorted MIS, literals of the MIS, assignment after), the
    first assignment and the final statistics."""
    import oracle as o

    n, offs, lits = instance(key)
    m = offs.size - 1
    A0 = all_false(n) if from_false else o.init_assignment(seed, n)
    st, A_end, trace = o.solve(n, offs, lits, seed, max_iters=K, A0=A0, trace=True, T=T)
    rows, A = [], A0
    for it, nu, nm, dres, A_after in trace:
        _, vm = o.eval_mask(offs, lits, A)
        U = o.mask_to_list(m, vm)
        M = np.sort(o.lfmis(n, offs, lits, U) if T == 1 else o.rr_mis(n, offs, lits, U, T))
        assert (U.size, M.size) == (nu, nm)
        rows.append((nu, M, dres, A_after))
        A = A_after
    return bc._frozen(dict(A0=A0, rows=rows, st=st, A=A_end))


def follow(s, ref, what, every=None):
    """run(1) per oracle row: |U|, MIS, the statistics deltas and the assignment after; then the
    final statistics.  every(s, it) runs after each iteration."""
    np.testing.assert_array_equal(s.assignment_words(), ref["A0"], err_msg=f"{what}: first assignment")
    sum_mis = n_res = 0
    for it, (nu, M, dres, A_after) in enumerate(ref["rows"]):
        st = s.run(1)
        assert (st["n_iterations"], st["n_violated"]) == (it + 1, nu), (what, it)
        if nu:
            np.testing.assert_array_equal(s.mis(), M, err_msg=f"{what}: MIS, iteration {it}")
        sum_mis += M.size
        n_res += dres
        assert (st["sum_mis_size"], st["n_resamples"]) == (sum_mis, n_res), (what, it)
        np.testing.assert_array_equal(s.assignment_words(), A_after, err_msg=f"{what}: assignment after iteration {it}")
        if every:
            every(s, it)
    # the oracle ends with one more evaluation pass, which does not resample: the one that finds
    # nothing violated, or the capped one (which the solver is not asked for)
    want = dict(ref["st"])
    if want["solved"]:
        s.run(1)
    else:
        want["n_iterations"] -= 1
    st = s.stats()
    assert st["n_violated"] == 0 or not want["solved"], what
    for k in ("n_iterations", "n_resamples", "sum_mis_size", "solved"):
        assert st[k] == want[k], (what, k)
    assert st["avg_mis_size"] == want["sum_mis_size"] // want["n_iterations"], what
    np.testing.assert_array_equal(s.assignment_words(), ref["A"], err_msg=f"{what}: final assignment")


def n_hot(n, lits):
    """Variables the layout flags hot: degree >= max(1024, 32 x mean degree) (alll_internal.h)."""
    d = np.bincount(lits >> np.uint32(1), minlength=n)
    return int((d >= max(1024, 32 * lits.size / n)).sum())


@functools.lru_cache(maxsize=None)
def instance(key):
    from alllsatisfiabilitysolver_amd import generate_ksat, generate_mixed

    if key == "u3":          # uniform 3-SAT: the narrow path (KW == 4)
        return (2000,) + generate_ksat(1, 2000, 4000, 3)
    if key == "k8":          # KW == 0, the v1 slots
        return (4000,) + generate_ksat(1, 4000, 6000, 8)
    if key == "mixed":       # widths 1 .. 12: variables past the 8 inline slots come from cv.lits
        return (600,) + generate_mixed(3, 600, 900, 1, 12)
    if key == "powerlaw":    # hot variables: fp_hot, FP_G_HOT, long claimant lists
        return (4000,) + generate_ksat(1, 4000, 12000, 3, 1)
    if key == "ratio4":      # does not solve
        return (3000,) + generate_ksat(1, 3000, 12000, 3)
    if key == "wrap":        # bias_cases.wrap_case's instance: five tiles
        c = bc.wrap_case()
        return c["n"], c["offs"], c["lits"]
    if key == "ragged":
        return (3000,) + generate_mixed(4, 3000, 9000, 1, 12)
    if key == "powerlaw1":   # hot variables under T = 1: vmix owner slots, the hot table
        return (5000,) + generate_ksat(1, 5000, 20000, 3, 1)
    if key == "small":       # far below ALLL_SMALL_U from the first iteration on
        return (500,) + generate_ksat(3, 500, 2000, 3)
    return structure(key)


# ---------------------------------------------------------------------------------------------
# Round robin under a small epoch budget.  B_MIN is the clamp (FP_EP_CAP_MIN = 2 (FP_G_MAX + 2)).
# Budgets per case: (at the clamp: fails > 0; between: both counters move; restarts only).  They
# were chosen from the counters of a run of every case over a sweep of budgets; DESIGN.md §6.1
# holds the table of the counters seen.
B_MIN = 16
RR_SEED, RR_K = 4242, 40
# case: (instance, T, from all-false, extra knobs, (budgets), counters expected per budget)
RR_CASES = {}


def rr_case(name, key, T, budgets, from_false=False, env=None):
    RR_CASES[name] = (key, T, from_false, env or {}, budgets)


def check_rr_counters(c, kind, what):
    """kind: 'fails' (at the clamp), 'both', 'restarts' (no iteration fails); 'clamp': the clamp minimum
    on a case where even that budget fails no iteration (RR_BUDGETS)."""
    if kind == "fails":
        assert c["rr_fails"] > 0, (what, c)
    elif kind == "both":
        assert c["rr_fails"] > 0 and c["rr_restarts"] > 0, (what, c)
    elif kind == "clamp":
        assert c["rr_restarts"] > 0 and c["rr_fails"] == 0, (what, c)
    else:
        assert c["rr_restarts"] > 0 and c["rr_fails"] == 0, (what, c)
    assert c["restarts"] == 0, (what, c)  # (the one-set loop's tail does not run)


def test_epoch_counters_write_four_words(gpu, monkeypatch):
    """alll_epoch_counters writes out[0 .. 3] and nothing after them; a fresh context counts nothing and
    starts at epoch 1, or at ALLL_EPOCH0."""
    import ctypes

    from alllsatisfiabilitysolver_amd import _native as N

    n, offs, lits = instance("small")
    for e0 in (None, 12345):
        with make(monkeypatch, {} if e0 is None else {"ALLL_EPOCH0": e0}, n, offs, lits, seed=1) as s:
            out = np.full(6, 0xABCD, np.uint64)
            assert N.lib().alll_epoch_counters(s._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 0
            assert list(out) == [0, 0, 0, e0 or 1, 0xABCD, 0xABCD]
            assert s.epoch_counters() == dict(rr_restarts=0, rr_fails=0, restarts=0, round_next=e0 or 1)


def run_rr_case(monkeypatch, name, budget, kind):
    key, T, from_false, env, _ = RR_CASES[name]
    n, offs, lits = instance(key)
    ref = reference(key, T, RR_SEED, RR_K, from_false)
    with make(monkeypatch, dict(env, ALLL_RR_EP_BUDGET=budget), n, offs, lits, seed=RR_SEED, n_threads=T) as s:
        if from_false:
            s.set_assignment_words(ref["A0"])
        follow(s, ref, f"{name}, budget {budget}")
        c = s.epoch_counters()
    check_rr_counters(c, kind, f"{name}, budget {budget}")
    return c


def _rr_params():
    return [(n, k) for n in RR_CASES for k in ("fails", "clamp", "both", "restarts") if k in RR_BUDGETS.get(n, {})]


FULL, REP4 = {"ALLL_RR_INC": 0}, {"ALLL_RR_REP_CAP": 4}
for _T in (2, 4, 16):
    rr_case(f"u3_T{_T}", "u3", _T, None)
rr_case("u3_T4_full_passes", "u3", 4, None, env=FULL)
rr_case("u3_T4_repair_gives_up", "u3", 4, None, env=REP4)
rr_case("k8_full_passes", "k8", 4, None, env=FULL)
rr_case("mixed", "mixed", 3, None)
rr_case("mixed_full_passes", "mixed", 3, None, env=FULL)
rr_case("powerlaw", "powerlaw", 4, None)
rr_case("chain513", "chain513", 3, None, from_false=True)
rr_case("combs64x300", "combs64x300", 3, None, from_false=True)
# The counters seen (restarts / fails over the case's iterations) are in DESIGN.md §6.1.  With the
# incremental passes only an iteration's first pass takes epochs (at most FP_G_MAX + 2 on these
# instances), so u3 and mixed fail no iteration even at the clamp: 'clamp' pins that, and their
# iterations fail under full passes only.  8-SAT solves in two iterations: the one counter that
# moves at all is a restart under full passes at the clamp (with incremental passes none does, so
# that is no case).
RR_BUDGETS = {
    "u3_T2": {"clamp": B_MIN, "restarts": 64}, "u3_T4": {"clamp": B_MIN, "restarts": 64},
    "u3_T16": {"clamp": B_MIN, "restarts": 64},
    "u3_T4_full_passes": {"fails": B_MIN, "both": 20, "restarts": 64},
    "u3_T4_repair_gives_up": {"fails": B_MIN, "both": 24, "restarts": 48},
    "k8_full_passes": {"restarts": B_MIN},
    "mixed": {"clamp": B_MIN, "restarts": 96}, "mixed_full_passes": {"clamp": B_MIN, "restarts": 64},
    "powerlaw": {"fails": B_MIN, "both": 64, "restarts": 256},
    "chain513": {"fails": B_MIN, "both": 40, "restarts": 128},
    "combs64x300": {"fails": B_MIN, "both": 48, "restarts": 96},
    "biased": {"restarts": 24},
    "long": {"every": B_MIN},
}


@pytest.mark.parametrize("name,kind", _rr_params(), ids=[f"{a}-{b}" for a, b in _rr_params()])
def test_rr_small_epoch_budget(gpu, monkeypatch, name, kind):
    """One round-robin case at one budget: 40 iterations (or to the solve) against the oracle, then
    the counter the budget was chosen for.  'fails': the clamp minimum, where k_rr_mw decides the
    iterations whose epochs ran out; 'restarts': restarts and no failed iteration; 'both'."""
    if name == "powerlaw":
        assert n_hot(instance("powerlaw")[0], instance("powerlaw")[2]) > 0
    run_rr_case(monkeypatch, name, RR_BUDGETS[name][kind], kind)


def test_rr_biased_tracked_run_across_restarts(gpu, monkeypatch):
    """The round-robin case of bias_cases (T = 4, thresholds and pins) with track_best, under a budget
    at which the epochs restart: the restart does not disturb the resample hooks, and best() is the
    record of the reference trajectory."""
    from best_cases import record

    c = bc.rr_case(4)
    budget = RR_BUDGETS["biased"]["restarts"]
    with make(monkeypatch, {"ALLL_RR_EP_BUDGET": budget}, c["n"], c["offs"], c["lits"], seed=c["seed"], n_threads=4,
              track_best=True) as s:
        s.set_thresholds(c["thr"])
        bc.follow(s, c["A0"], c["rows"], f"biased, budget {budget}")
        evaluated = [c["A0"]] + [r[4] for r in c["rows"][:-1]]
        want, got = record([(r[1], A) for r, A in zip(c["rows"], evaluated)]), s.best()
        assert (got["n_violated"], got["iteration"]) == (want["n_violated"], want["iteration"])
        np.testing.assert_array_equal(got["words"], want["words"], err_msg="best after the restarts")
        k = s.epoch_counters()
    assert k["rr_restarts"] > 0, k


def test_rr_long_run_epoch_and_serial_restarts_coincide(gpu, monkeypatch):
    """300 iterations of the ratio-4 instance, T = 4, at a budget under which every iteration after
    the first starts its epochs over (asserted: restarts == iterations - 1).  The 8-bit cover serials
    start over every few iterations, so both restarts fall in one iteration (restart == 3) every time
    they do, and the cover stamps cross their wrap at 255."""
    K, T = 300, 4
    n, offs, lits = instance("ratio4")
    ref = reference("ratio4", T, 31, K)
    assert ref["st"]["solved"] == 0 and len(ref["rows"]) == K - 1
    budget, seen = RR_BUDGETS["long"]["every"], []
    with make(monkeypatch, {"ALLL_RR_EP_BUDGET": budget, "ALLL_RR_INC": 0}, n, offs, lits, seed=31, n_threads=T) as s:
        follow(s, ref, f"300 iterations, budget {budget}", every=lambda s, it: seen.append(s.epoch_counters()["rr_restarts"]))
        c = s.epoch_counters()
    assert seen == list(range(len(seen))), "an iteration after the first did not restart its epochs"
    assert len(seen) == K - 1 and c["rr_restarts"] == K - 2, c


# ---------------------------------------------------------------------------------------------
# The one-set loop across the end of its 32-bit epochs.  The tail of an iteration starts the epochs
# over once the first unused epoch has reached restart_at = 2^32 - (64 + 2^20 + 2)
# (EP_RESTART_AT: at most GRID_ROUNDS_MAX = 64 grid rounds, MAX_TAIL_ROUNDS = 2^20); alll_create applies the same rule to
# ALLL_EPOCH0.  So a start at or past restart_at restarts at create, on fresh keys, and the starts
# that make k_tail clear keys in use lie just below it.
W_SEED, W_K = 77, 60
TWO32 = 1 << 32


def restart_at(grid_rounds=None):
    return TWO32 - (64 + (1 << 20) + 2)


def wrap_starts(grid_rounds, first_step):
    """{label: (ALLL_EPOCH0, restarts expected)}.  first_step: epochs iteration 1 uses, from the
    control run's counters."""
    at = restart_at(grid_rounds)
    return {
        "grid_round_of_iteration_1": (TWO32 - 3, 1),      # past restart_at: the rule at create
        "at_the_reduce": (TWO32 - 1, 1),
        "a_few_iterations_in_2^32": (TWO32 - 40, 1),
        "first_start_past_the_rule": (at, 1),
        "end_of_iteration_1": (at - 1, 1),                # k_tail of iteration 1 clears
        # round_next == restart_at - 1 when iteration 2's pre-reduce scatter reads it
        "scatter_of_iteration_2": (at - 1 - first_step, 1),
        "a_few_iterations_in": (at - 40, 1),
    }


def run_wrap(monkeypatch, key, env, what, grid_rounds=4, from_false=False, **kw):
    """The control (ALLL_EPOCH0 = 2^31: the knob alone changes nothing), then every start of
    wrap_starts: the same 60 iterations, one restart, small epochs after it."""
    n, offs, lits = instance(key)
    ref = reference(key, 1, W_SEED, W_K, from_false)
    steps = []

    def start(s):
        if from_false:
            s.set_assignment_words(ref["A0"])

    with make(monkeypatch, dict(env, ALLL_EPOCH0=1 << 31), n, offs, lits, seed=W_SEED, **kw) as s:
        start(s)
        assert s.epoch_counters()["round_next"] == 1 << 31
        follow(s, ref, f"{what}, control", every=lambda s, it: steps.append(s.epoch_counters()["round_next"]))
        c = s.epoch_counters()
        assert c["restarts"] == 0 and c["round_next"] > 1 << 31, c
    first_step = steps[0] - (1 << 31)
    assert 1 <= first_step <= grid_rounds + (1 << 20) + 1
    for label, (e0, want) in wrap_starts(grid_rounds, first_step).items():
        with make(monkeypatch, dict(env, ALLL_EPOCH0=e0), n, offs, lits, seed=W_SEED, **kw) as s:
            start(s)
            follow(s, ref, f"{what}, {label} (ALLL_EPOCH0 = {e0})")
            c = s.epoch_counters()
        assert c["restarts"] == want and c["round_next"] < 1 << 22, (what, label, c)
    return steps


WRAP_LAYOUTS = {
    # name: (instance, knobs, Solver flag names, grid rounds)
    "buckets": ("wrap", {"ALLL_BUCKET_MIN_U": 0}, (), 4),            # bucketed round 0 in every iteration
    "atomic_claims": ("wrap", {"ALLL_SMALL_U": 0}, ("FLAG_ATOMIC_CLAIMS",), 4),
    "generic_csr": ("wrap", {"ALLL_SMALL_U": 0}, ("FLAG_GENERIC_CSR",), 4),
    "small_u": ("wrap", {}, (), 4),                                  # round 0 on the grid, the rest in the tail
    "ragged": ("ragged", {"ALLL_SMALL_U": 0}, (), 4),                # k_eval_ragged
    "hot": ("powerlaw1", {"ALLL_SMALL_U": 0}, (), 7),                # vmix owner slots, the hot table's flush
    "tiny": ("small", {}, (), 4),
    "no_graph": ("wrap", {"ALLL_SMALL_U": 0}, ("FLAG_NO_GRAPH",), 4),
}


@pytest.mark.parametrize("layout", list(WRAP_LAYOUTS))
def test_one_set_loop_across_the_epoch_restart(gpu, native, monkeypatch, layout):
    key, env, flag_names, G = WRAP_LAYOUTS[layout]
    flags = 0
    for f in flag_names:
        flags |= getattr(native, f)
    n, offs, lits = instance(key)
    if layout == "hot":
        assert n_hot(n, lits) > 0
    with make(monkeypatch, env, n, offs, lits, seed=W_SEED, flags=flags) as s:
        assert s.uses_graphs()[0] is (layout != "no_graph")
        assert (s.layout() == 3) is (layout not in ("generic_csr", "ragged"))
    run_wrap(monkeypatch, key, env, layout, grid_rounds=G, flags=flags)


def test_deep_tail_at_the_margin(gpu, monkeypatch):
    """chain4097 from all-false: the tail of iteration 1 makes thousands of rounds.  The rule's margin
    (an iteration that starts below restart_at may use 64 + 2^20 epochs more) is what keeps
    that iteration below 2^32 when it starts at restart_at - 1, the last start at which the restart
    does not come before the iteration; wrap_starts holds that start and the first one past it."""
    n, offs, lits = instance("chain4097")
    steps = run_wrap(monkeypatch, "chain4097", {}, "chain4097", from_false=True)
    assert steps[0] - (1 << 31) > 2000  # (the tail's rounds of iteration 1)
    # a start from which iteration 1 runs across restart_at in the middle of its tail
    ref = reference("chain4097", 1, W_SEED, W_K, True)
    e0 = restart_at(4) - 1000
    with make(monkeypatch, {"ALLL_EPOCH0": e0}, n, offs, lits, seed=W_SEED) as s:
        s.set_assignment_words(ref["A0"])
        follow(s, ref, "chain4097, across restart_at inside the tail")
        c = s.epoch_counters()
    assert c["restarts"] == 1 and c["round_next"] < 1 << 22, c


def test_run_of_many_iterations_across_the_restart(gpu, monkeypatch):
    """run(60) as one call: the replayed graphs carry no decision about the restart."""
    n, offs, lits = instance("wrap")
    ref = reference("wrap", 1, W_SEED, W_K)
    for env in ({"ALLL_BUCKET_MIN_U": 0}, {"ALLL_SMALL_U": 0}):
        with make(monkeypatch, dict(env, ALLL_EPOCH0=restart_at(4) - 100), n, offs, lits, seed=W_SEED) as s:
            assert not ref["st"]["solved"]
            st = s.run(len(ref["rows"]))
            assert st["n_iterations"] == len(ref["rows"])
            for k in ("n_resamples", "sum_mis_size", "solved"):
                assert st[k] == ref["st"][k], k
            np.testing.assert_array_equal(s.assignment_words(), ref["A"])
            c = s.epoch_counters()
        assert c["restarts"] == 1 and c["round_next"] < 1 << 22, c


def test_streaming_solve_across_the_restart(gpu, oracle_mod, monkeypatch):
    """The streaming solve with one thread (stream_batch = 777): its LFMIS runs in the same tail."""
    o = oracle_mod
    n, offs, lits = instance("ratio4")
    st_o, A_o, rows = o.solve_stream(n, offs, lits, W_SEED, 777, max_iters=W_K, trace=True)
    for e0, want in ((1 << 31, 0), (restart_at(4) - 1, 1), (restart_at(4) - 40, 1), (TWO32 - 3, 1)):
        with make(monkeypatch, {"ALLL_EPOCH0": e0}, n, offs, lits, seed=W_SEED, stream_batch=777) as s:
            for it, nu, nm, dres, A_after in rows:
                before = s.stats()
                s.run(1)
                after = s.stats()
                assert after["n_violated"] == nu, (e0, it)
                assert s.mis().size == nm, (e0, it)
                assert after["n_resamples"] - before["n_resamples"] == dres, (e0, it)
                np.testing.assert_array_equal(s.assignment_words(), A_after, err_msg=f"{e0}: A after iteration {it}")
            c = s.epoch_counters()
        assert c["restarts"] == want and (c["round_next"] < 1 << 22) is bool(want), (e0, c)


def test_group_across_the_restart(gpu, oracle_mod, monkeypatch):
    """A GroupSolver of 8 items of 300 clauses: every item against the oracle's run of a Solver of its
    own, across the union's restart."""
    from alllsatisfiabilitysolver_amd import GroupSolver, generate_ksat

    o = oracle_mod
    items = [(70 + 5 * i,) + generate_ksat(20 + i, 70 + 5 * i, 300, 3) for i in range(8)]  # ratios 4.3 .. 2.9
    seeds = [900 + i for i in range(8)]
    refs = [o.solve(n, offs, lits, seed, max_iters=W_K, trace=True) for (n, offs, lits), seed in zip(items, seeds)]
    for e0, want in ((1 << 31, 0), (restart_at(4) - 1, 1), (restart_at(4) - 40, 1), (TWO32 - 1, 1)):
        for k, v in {"ALLL_EPOCH0": e0}.items():
            monkeypatch.setenv(k, str(v))
        with GroupSolver(items, seeds) as g:
            monkeypatch.delenv("ALLL_EPOCH0")
            for it in range(W_K - 1):
                sts = g.run(1)
                for i, (st_o, A_o, rows) in enumerate(refs):
                    # (a trace row per resampling pass; after them the item is solved and stays as it is)
                    nu, A = (rows[it][1], rows[it][4]) if it < len(rows) else (0, A_o)
                    assert sts[i]["n_violated"] == nu, (e0, it, i)
                    np.testing.assert_array_equal(g.assignment_words(i), A, err_msg=f"{e0}: item {i}, iteration {it}")
            for i, (st_o, A_o, rows) in enumerate(refs):
                for k in ("n_resamples", "sum_mis_size"):
                    assert sts[i][k] == st_o[k], (e0, i, k)
                done = st_o["solved"] and len(rows) < W_K - 1  # (its solved pass is among the W_K - 1 run)
                assert (sts[i]["solved"], sts[i]["n_iterations"]) == ((1, st_o["n_iterations"]) if done else (0, W_K - 1)), (e0, i)
            assert any(not st_o["solved"] for st_o, _, _ in refs)  # (the union runs all W_K - 1 iterations)
            c = g.epoch_counters()
        assert c["restarts"] == want and (c["round_next"] < 1 << 22) is bool(want), (e0, c)
