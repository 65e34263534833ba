"""Groups past one workgroup of items (test-side only): a thousand tiny items in one
group, so that the per-item device loops (group_finish's stride, k_group_best's second workgroup and
ragged last one, group_merge's 64 distinct items per wave, runs of clauseless items in the clause
bases, one-word items under the per-word bits) leave their first trip, and seeds whose high word
differs between items that share the low one.

The references are the oracle's, per item in the item's own numbering at the item's seed: the Trace
scheme of tests/test_gpu_group.py, bias_cases.reference for items with thresholds, and
best_cases.trajectory / record for the records.  A case is computed once per process and shared,
read-only, by the CPU module that pins its facts (tests/test_swarm_cases.py) and the GPU tests
(tests/test_gpu_group_swarm.py)."""
import functools

import numpy as np

import best_cases
import bias_cases
from bias_cases import PIN1, _frozen
from group_cases import compose
from lfmis_structures import all_false, chain, copies, dense, star

N_SWARM = 1000
NS_RAGGED = (1, 2, 31, 32, 33, 65, 7)
NS_FIXED = (3, 4, 31, 32, 33, 65, 7)
MS = (0, 1, 2, 5, 9, 30, 63, 64, 65, 3, 13)
HARD_N, HARD_M = 120, 516  # ratio 4.3: not solved within the runs here, so the group keeps advancing
CAP = 12                   # max_iters of the swarms' full solves
TILE, MASK_WORD = 4096, 64
NO_CLAUSE = (np.zeros(1, np.uint64), np.zeros(0, np.uint32))


def swarm_seed(i):
    """The high word differs from item to item; two hundred items share each low word."""
    return (((i * 0x9E3779B1) % 2**32) << 32) | (i % 5)


def clauseless(i, N):
    """Runs of items without a clause: at the front, in the middle, at the end (longer than a wave)."""
    return i < 3 or 300 <= i < 380 or i >= N - 70


def emptied(i):
    """Ragged swarm: items whose clause m // 2 is emptied (where they have clauses)."""
    return i % 211 == 7


def swarm(N=N_SWARM, fixed=False):
    """-> (items, seeds).  Item i has NS[i % 7] variables and MS[i % 11] clauses; every i % 97 == 50
    is a hard item of 120 variables and 516 clauses; the items of clauseless() have none.  Ragged:
    widths 1-4, literals drawn over 2n (tautologies and repeated variables allowed), and the items
    of emptied() get an empty clause -- they are never solvable, and the empty clause sits in their
    MIS with zero literals.  Fixed: generate_ksat(1000 + i, n, m, 3), so the union takes the
    width-3 layouts."""
    from alllsatisfiabilitysolver_amd import generate_ksat

    rng = np.random.default_rng(11)
    NS = NS_FIXED if fixed else NS_RAGGED
    items = []
    for i in range(N):
        n, m = NS[i % 7], MS[i % 11]
        if clauseless(i, N):
            m = 0
        if i % 97 == 50:  # (item 341 among them: it splits the middle run into 41 and 38 clauseless items)
            n, m = HARD_N, HARD_M
        if m == 0:
            items.append((n, *NO_CLAUSE))
        elif fixed:
            items.append((n, *generate_ksat(1000 + i, n, m, 3)))
        else:
            widths = rng.integers(1, 5, m)
            if emptied(i):
                widths[m // 2] = 0
            offs = np.zeros(m + 1, np.uint64)
            offs[1:] = np.cumsum(widths)
            items.append((n, offs, rng.integers(0, 2 * n, int(offs[-1])).astype(np.uint32)))
    return items, [swarm_seed(i) for i in range(N)]


def lockstep(n_items=130):
    """n_items copies of copies(64) -- 64 times (x0 or x1 or x2) -- with distinct seeds that have a
    high word, every item from the all-false assignment.  In clause order mask word j of the violated
    bitmask is exactly item j: wave 0 of a full tile merges 64 distinct items, and each tile's MIS
    list holds one clause from each of 64 items.  -> (items, seeds, initial words per item)."""
    item = copies(64)
    return [item] * n_items, [swarm_seed(1000 + i) for i in range(n_items)], [all_false(item[0])] * n_items


def structures_bag():
    """Three random 3-SAT items of 2000 variables, then star(2000, 1) (a hub of degree >= HOT_THR_MIN
    whose union variable index is far from 0), copies(300), dense(500, 8, 3) and chain(513), all from
    all-false.  -> (items, seeds, initial words per item)."""
    from alllsatisfiabilitysolver_amd import generate_ksat

    items = [(2000, *generate_ksat(60 + i, 2000, 8000, 3)) for i in range(3)]
    items += [star(2000, 1), copies(300), dense(500, 8, 3), chain(513)]
    return items, [swarm_seed(2000 + i) for i in range(len(items))], [all_false(n) for n, _, _ in items]


def swarm_thresholds(i, n):
    """Thresholds of item i (every i % 3 == 1): random with pins, the first variable pinned 0 and,
    where n > 1, the last one pinned 1.  None: the item stays unbiased."""
    if i % 3 != 1:
        return None
    return bias_cases.mixed_thresholds(n, 500 + i, must=((0, 0), (n - 1, PIN1)) if n > 1 else ((0, 0),))


# ---------------------------------------------------------------------------------------------
# References


def rows_after(A0, rows, steps):
    """Trace.after() for the rows of bias_cases.reference / unbiased_reference (which end with the
    row of the pass that found nothing violated): the statistics and the assignment after `steps`
    iterations."""
    done = [r for r in rows[:steps] if r[1] > 0]
    ended = len(done) < min(steps, len(rows))
    assert ended or len(rows) >= steps, "the reference stops before these steps"
    return dict(n_iterations=len(done) + 1 if ended else steps, n_violated=0 if ended else done[-1][1],
                sum_mis_size=sum(int(r[2].size) for r in done), n_resamples=sum(r[3] for r in done),
                solved=int(ended)), (done[-1][4] if done else A0)


def _traces(items, seeds, cap, A0s=None):
    import oracle as o
    from test_gpu_group import Trace

    return [Trace(o, it, s, cap, A0=None if A0s is None else A0s[i]) for i, (it, s) in enumerate(zip(items, seeds))]


@functools.lru_cache(maxsize=None)
def swarm_case(fixed=False):
    """The swarm with every item's oracle trace capped at CAP passes."""
    items, seeds = swarm(N_SWARM, fixed)
    return _frozen(dict(items=items, seeds=seeds, traces=_traces(items, seeds, CAP)))


@functools.lru_cache(maxsize=None)
def swarm_traces_capped(cap):
    """The ragged swarm's traces under another cap (test_item_count_boundary)."""
    c = swarm_case()
    return _traces(c["items"], c["seeds"], cap)


@functools.lru_cache(maxsize=None)
def lockstep_case():
    items, seeds, A0s = lockstep()
    return _frozen(dict(items=items, seeds=seeds, A0s=A0s, traces=_traces(items, seeds, 8, A0s)))


@functools.lru_cache(maxsize=None)
def lockstep_trajectories():
    import oracle as o

    c = lockstep_case()
    return [best_cases.trajectory(o, *it, s, 6, A0=A0) for it, s, A0 in zip(c["items"], c["seeds"], c["A0s"])]


@functools.lru_cache(maxsize=None)
def bag_case():
    items, seeds, A0s = structures_bag()
    return _frozen(dict(items=items, seeds=seeds, A0s=A0s, traces=_traces(items, seeds, 12, A0s)))


@functools.lru_cache(maxsize=None)
def swarm_trajectories():
    """best_cases.trajectory of every item of the ragged swarm through the capped pass CAP."""
    import oracle as o

    c = swarm_case()
    return [best_cases.trajectory(o, *it, s, CAP, capped=(CAP,)) for it, s in zip(c["items"], c["seeds"])]


THR_STEPS = 6


@functools.lru_cache(maxsize=None)
def thresholds_case():
    """The ragged swarm with swarm_thresholds: per item the thresholds (or None), (A0, rows) of
    bias_cases.reference (None where unbiased: the item follows its trace) and the trajectory of its
    THR_STEPS passes."""
    import oracle as o

    c = swarm_case()
    thrs = [swarm_thresholds(i, it[0]) for i, it in enumerate(c["items"])]
    refs = [None if t is None else bias_cases.reference(o, *it, s, t, THR_STEPS)
            for it, s, t in zip(c["items"], c["seeds"], thrs)]
    trajs = [best_cases.trajectory(o, *it, s, THR_STEPS, thr=t) for it, s, t in zip(c["items"], c["seeds"], thrs)]
    return _frozen(dict(thrs=thrs, refs=refs, trajs=trajs))


def wants_after(case, steps, refs=None):
    """Per item (statistics, assignment) after `steps` iterations: from the biased reference where the
    item has one, else from its trace."""
    return [t.after(steps) if refs is None or refs[i] is None else rows_after(*refs[i], steps)
            for i, t in enumerate(case["traces"])]


# ---------------------------------------------------------------------------------------------
# The facts the GPU cases rely on, from the oracle alone (pinned in tests/test_swarm_cases.py)


def pass_sets(o, item, A):
    """(violated clauses, MIS) of assignment A, item-local ascending clause ids."""
    n, offs, lits = item
    _, vm = o.eval_mask(offs, lits, A)
    U = o.mask_to_list(len(offs) - 1, vm)
    return U, o.lfmis(n, offs, lits, U)


def first_pass_spread(o, items, A0s):
    """Pass 1 of the union in clause order: per full 4096-clause tile the distinct items among its
    violated clauses and among its MIS clauses, and the most items any 64-clause mask word holds
    violated clauses of."""
    places = compose(items)[3]
    m = places[-1]["clause_base"] + places[-1]["n_clauses"]
    item_of_U, item_of_M = np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    for i, (it, A0, p) in enumerate(zip(items, A0s, places)):
        U, M = pass_sets(o, it, A0)
        item_of_U[p["clause_base"] + U.astype(np.int64)] = i
        item_of_M[p["clause_base"] + M.astype(np.int64)] = i

    def distinct(a, size, full_only):
        out = []
        for c0 in range(0, m - size + 1 if full_only else m, size):
            x = a[c0:c0 + size]
            out.append(int(np.unique(x[x >= 0]).size))
        return out

    return distinct(item_of_U, TILE, True), distinct(item_of_M, TILE, True), max(distinct(item_of_U, MASK_WORD, False))
