"""Best-assignment tracking (test-side only): the loop on the CPU as a trajectory of
(violated clauses, assignment evaluated) per eval pass, composed from the oracle's own primitives
(init_assignment, eval_mask, mask_to_list, lfmis / rr_mis, clause_vars, resample_words) and, under
thresholds, the biased stream of tests/bias_cases.py -- nothing of the code under test, and not
oracle.solve(trace=True), whose rows hold the assignment after the resample and omit the last pass.

Pass p (1-based, the n_iterations value after it) evaluates the assignment and, unless it is solved or
capped, resamples it at round p - 1.  The capped pass of a solve(max_iters) does not resample, so a
continuation evaluates the same assignment again at pass p + 1 (and resamples it at round p).  The
record is the first pass with the fewest violated clauses.

A case is computed once per process and shared, read-only, by the CPU module that pins its facts
(tests/test_best_cases.py) and the GPU tests (tests/test_gpu_best.py)."""
import functools

import numpy as np

import bias_cases as bc
from bias_cases import PIN1, _frozen, _ksat

EMPTY = dict(n_violated=2**64 - 1, iteration=0)


def trajectory(o, n, offs, lits, seed, passes, thr=None, T=1, capped=(), inject=None, A0=None, stop=None):
    """[(violated clauses, assignment evaluated)] of passes 1 .. `passes`, ending early at a solved pass.
    thr: per-variable thresholds (A0 defaults to the biased fill); T > 1: the round-robin MIS; capped:
    passes that do not resample; inject: {pass: words} set before that pass evaluates; stop(counts so
    far) -> True ends the trajectory after that pass."""
    m = len(offs) - 1
    if A0 is None:
        A0 = o.init_assignment(seed, n) if thr is None else bc.biased_init(o, seed, n, thr)
    A = np.array(A0, np.uint32)
    out = []
    for p in range(1, passes + 1):
        if inject and p in inject:
            A = np.array(inject[p], np.uint32)
        nu, vm = o.eval_mask(offs, lits, A)
        out.append((int(nu), A.copy()))
        if nu == 0 or (stop and stop([u for u, _ in out])):
            break
        if p in capped:
            continue
        if thr is not None:
            A = bc.biased_step(o, n, offs, lits, A, seed, p - 1, thr, T)[3]
        else:
            U = o.mask_to_list(m, vm)
            M = o.lfmis(n, offs, lits, U) if T == 1 else o.rr_mis(n, offs, lits, U, T)
            A = o.resample_words(A.copy(), seed, p - 1, o.clause_vars(offs, lits, M))
    return out


def record(traj):
    """The record after the passes of traj: the first pass with the fewest violated clauses."""
    if not traj:
        return dict(EMPTY, words=None)
    us = [u for u, _ in traj]
    i = us.index(min(us))
    return dict(n_violated=us[i], iteration=i + 1, words=traj[i][1])


def improving(traj):
    """The passes (1-based) that set a new record."""
    out, best = [], None
    for p, (u, _) in enumerate(traj, 1):
        if best is None or u < best:
            out.append(p)
            best = u
    return out


def counts(traj):
    return [u for u, _ in traj]


def unit_instance(o, seed):
    """n = 1 and one unit clause that the initial bit violates."""
    bit = int(o.init_assignment(seed, 1)[0]) & 1
    return 1, np.array([0, 1], np.uint64), np.array([bit], np.uint32)  # (literal 1 = not x0, 0 = x0)


# ---------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_best.py

MAIN = dict(n=203, m=812, gen=7, seed=1, passes=60)
CAP_RUN = 5  # passes the continuation of the capped case runs


@functools.lru_cache(maxsize=None)
def main_case():
    """1. n = 203, m = 812 (gen seed 7, seed 1): 60 passes; the 60th is the capped pass of solve(60)."""
    import oracle as o

    c = MAIN
    offs, lits = _ksat(c["gen"], c["n"], c["m"], 3)
    traj = trajectory(o, c["n"], offs, lits, c["seed"], c["passes"], capped=(c["passes"],))
    return _frozen(dict(n=c["n"], offs=offs, lits=lits, seed=c["seed"], passes=c["passes"], traj=traj))


@functools.lru_cache(maxsize=None)
def tie_case():
    """2. n = 33, m = 132 (gen seed 3, seed 1), 40 passes: the minimum is reached twice."""
    import oracle as o

    n, seed, passes = 33, 1, 40
    offs, lits = _ksat(3, n, 132, 3)
    traj = trajectory(o, n, offs, lits, seed, passes, capped=(passes,))
    return _frozen(dict(n=n, offs=offs, lits=lits, seed=seed, passes=passes, traj=traj))


@functools.lru_cache(maxsize=None)
def unit_case():
    """2b. n = 1, one unit clause against the initial bit: solved within a few passes."""
    import oracle as o

    seed = 1
    n, offs, lits = unit_instance(o, seed)
    traj = trajectory(o, n, offs, lits, seed, 64)
    return _frozen(dict(n=n, offs=offs, lits=lits, seed=seed, passes=64, traj=traj))


@functools.lru_cache(maxsize=None)
def capped_case():
    """3. main_case capped at the pass of its record (the capped pass is the record), then CAP_RUN
    passes of a continuation: the pass after the cap evaluates the same assignment again."""
    import oracle as o

    c = main_case()
    cap = record(c["traj"])["iteration"]
    traj = trajectory(o, c["n"], c["offs"], c["lits"], c["seed"], cap + CAP_RUN, capped=(cap,))
    return _frozen(dict(c, cap=cap, passes=cap + CAP_RUN, traj=traj))


@functools.lru_cache(maxsize=None)
def blocks_case():
    """4. Past one resample workgroup (4096 variables): n = 5003, m = 20000 (gen seed 11, seed 5), 40 passes."""
    import oracle as o

    n, seed, passes = 5003, 5, 40
    offs, lits = _ksat(11, n, 20000, 3)
    traj = trajectory(o, n, offs, lits, seed, passes, capped=(passes,))
    return _frozen(dict(n=n, offs=offs, lits=lits, seed=seed, passes=passes, traj=traj))


BIG_MUST = ((4095, 0), (4096, PIN1), (16383, 0x40000000), (16384, PIN1))
BIG_MAX_PASSES = 60


@functools.lru_cache(maxsize=None)
def big_case():
    """4b. n = 20003, m = 80000 (five resample workgroups) with pins and a bias on the variables at the
    workgroups' edges: as many passes as it takes until the record is not the last pass (at most 60)."""
    import oracle as o

    n, seed = 20003, 17
    offs, lits = _ksat(11, n, 80000, 3)
    thr = bc.mixed_thresholds(n, 7, must=BIG_MUST)
    traj = trajectory(o, n, offs, lits, seed, BIG_MAX_PASSES, thr=thr,
                      stop=lambda us: len(us) > 1 and us[-1] >= min(us[:-1]))
    return _frozen(dict(n=n, offs=offs, lits=lits, seed=seed, thr=thr, passes=len(traj), traj=traj))


@functools.lru_cache(maxsize=None)
def rr_case():
    """5. main_case's instance under the round robin of T = 4 sets, 30 passes."""
    import oracle as o

    c = main_case()
    traj = trajectory(o, c["n"], c["offs"], c["lits"], c["seed"], 30, T=4)
    return _frozen(dict(n=c["n"], offs=c["offs"], lits=c["lits"], seed=c["seed"], passes=30, T=4, traj=traj))


@functools.lru_cache(maxsize=None)
def biased_case():
    """5b. main_case's instance with thresholds and pins (the biased resample), 40 passes."""
    import oracle as o

    c = main_case()
    thr = bc.mixed_thresholds(c["n"], 9)
    traj = trajectory(o, c["n"], c["offs"], c["lits"], c["seed"], 40, thr=thr)
    return _frozen(dict(n=c["n"], offs=c["offs"], lits=c["lits"], seed=c["seed"], thr=thr, passes=40, traj=traj))


INJECT_WORSE_AT, INJECT_BETTER_AT, INJECT_PASSES = 21, 31, 40


@functools.lru_cache(maxsize=None)
def inject_case():
    """6. main_case with the assignment set from outside before pass 21 (all variables false: worse than
    the record) and before pass 31 (the record words of main_case's 60 passes: better than the record)."""
    import oracle as o

    c = main_case()
    worse = np.zeros((c["n"] + 31) // 32, np.uint32)
    better = record(c["traj"])["words"].copy()
    inject = {INJECT_WORSE_AT: worse, INJECT_BETTER_AT: better}
    traj = trajectory(o, c["n"], c["offs"], c["lits"], c["seed"], INJECT_PASSES, inject=inject)
    return _frozen(dict(n=c["n"], offs=c["offs"], lits=c["lits"], seed=c["seed"], passes=INJECT_PASSES, worse=worse,
                        better=better, traj=traj))


# (n_vars, clauses, generator seed, seed, seed of mixed_thresholds or None); the last one is at ratio 2.5
GROUP_ITEMS = ((1500, 6000, 40, 70, None), (5003, 20000, 41, 71, 31), (33, 132, 42, 72, 32), (4097, 16400, 43, 73, None),
               (200, 500, 4, 1, None))
GROUP_EXTRA, GROUP_MORE = 4, 10  # passes of the cap after the last item has solved; passes of a later run


@functools.lru_cache(maxsize=None)
def small_item():
    """The 200-variable item at ratio 2.5 (gen seed 4, seed 1): it solves."""
    import oracle as o

    n, m, gen, seed, _ = GROUP_ITEMS[4]
    offs, lits = _ksat(gen, n, m, 3)
    traj = trajectory(o, n, offs, lits, seed, 200)
    return _frozen(dict(n=n, offs=offs, lits=lits, seed=seed, traj=traj))


@functools.lru_cache(maxsize=None)
def group_case():
    """7. Five items; items 1 and 2 have thresholds; the last one solves at pass `solved_at`, the cap is
    GROUP_EXTRA passes later, then GROUP_MORE passes of a run.  Per item: the trajectory of a context of
    its own through the cap (`cap` passes, or to its solved pass) and through the later run."""
    import oracle as o

    small = small_item()
    solved_at = len(small["traj"])
    cap = solved_at + GROUP_EXTRA
    items, seeds, thrs, trajs = [], [], [], []
    for n, m, gen, seed, tseed in GROUP_ITEMS:
        offs, lits = _ksat(gen, n, m, 3)
        thr = None if tseed is None else bc.mixed_thresholds(n, tseed)
        items.append((n, offs, lits))
        seeds.append(seed)
        thrs.append(thr)
        trajs.append(trajectory(o, n, offs, lits, seed, cap + GROUP_MORE, thr=thr, capped=(cap,)))
    return _frozen(dict(items=items, seeds=seeds, thrs=thrs, trajs=trajs, cap=cap, solved_at=solved_at))


BATCH_SEEDS = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def batch_case():
    """8. main_case's instance under four seeds and the 200-variable item, capped at 60 passes."""
    import oracle as o

    c, small = main_case(), small_item()
    cap = c["passes"]
    items = [(c["n"], c["offs"], c["lits"])] * len(BATCH_SEEDS) + [(small["n"], small["offs"], small["lits"])]
    seeds = list(BATCH_SEEDS) + [small["seed"]]
    trajs = [trajectory(o, n, offs, lits, s, cap, capped=(cap,)) for (n, offs, lits), s in zip(items, seeds)]
    return _frozen(dict(items=items, seeds=seeds, trajs=trajs, cap=cap))
