"""Unit propagation of the pinned variables (test-side only): a numpy restatement of
the rounds of include/alll.h -- nothing of the code under test -- and the cases of the propagation
tests.  A case is computed once per process and shared, read-only, by the CPU module that pins its
facts (tests/test_prop_cases.py), the host tests and the GPU tests.

Why these sizes: the pack and apply kernels hold 32 variables per lane, 8192 per 256-lane workgroup,
so the 20003 variables of cases A and C make three workgroups with a ragged last word; 80000 clauses
are 313 scan workgroups; the chain of case C puts consecutive links in different workgroups and
needs every round's hand-over to work 299 times; cases D, E and F are the corners of the semantics."""
import functools

import numpy as np

from bias_cases import _frozen, _ksat

PIN1 = 0xFFFFFFFF
FAIR = 1 << 31
FIXPOINT, CONFLICT, ROUND_CAP, NONE = 0, 1, 2, 3


def propagate(n, offs, lits, thr, max_rounds=0):
    """The rounds of alll.h on the CPU -> (propagated thresholds, {status, rounds, n_forced, conflict_clause})."""
    thr = np.array(thr, np.uint32)
    lits = np.asarray(lits, np.int64)
    m = len(offs) - 1
    cl = np.repeat(np.arange(m), np.diff(np.asarray(offs, np.int64)))  # the clause of every literal
    v, neg = lits >> 1, (lits & 1).astype(bool)
    rounds = n_forced = 0

    def result(status, clause=m):
        return thr, dict(status=status, rounds=rounds, n_forced=n_forced, conflict_clause=int(clause))

    while True:
        t = thr[v]
        true = t == np.where(neg, 0, PIN1)
        free = ~true & (t != np.where(neg, PIN1, 0))
        open_ = np.bincount(cl, true, m) == 0  # no true literal (an empty clause too)
        n_free = np.bincount(cl, free, m)
        falsified = np.flatnonzero(open_ & (n_free == 0))
        if falsified.size:
            return result(CONFLICT, falsified[0])
        lo, hi = np.full(m, 2 * n, np.int64), np.full(m, -1, np.int64)  # the free literals' range per clause
        np.minimum.at(lo, cl[free], lits[free])
        np.maximum.at(hi, cl[free], lits[free])
        units = lo[open_ & (n_free > 0) & (lo == hi)]
        if units.size == 0:
            return result(FIXPOINT)
        if max_rounds and rounds >= max_rounds:
            return result(ROUND_CAP)
        thr[units[units & 1 == 1] >> 1] = 0
        thr[units[units & 1 == 0] >> 1] = PIN1  # (forced both ways: pinned to 1)
        n_forced += int(np.unique(units >> 1).size)
        rounds += 1


def cube(n, d, cs):
    """d random pins, every other variable a fair coin."""
    rng = np.random.default_rng(1000 * d + cs)
    vs = rng.choice(n, d, replace=False)
    val = rng.integers(0, 2, d)
    thr = np.full(n, FAIR, np.uint32)
    thr[vs] = np.where(val == 1, PIN1, 0).astype(np.uint32)
    return thr


def csr(clauses):
    offs = np.zeros(len(clauses) + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in clauses])
    return offs, np.array([l for c in clauses for l in c], np.uint32)


def pos(v):
    return 2 * v


def neg(v):
    return 2 * v + 1


def _case(name, n, offs, lits, thr, max_rounds=0):
    out, res = propagate(n, offs, lits, thr, max_rounds)
    return dict(name=name, n=n, offs=np.asarray(offs, np.uint64), lits=np.asarray(lits, np.uint32), thr=thr, out=out,
                res=res, max_rounds=max_rounds)


@functools.lru_cache(maxsize=None)
def a_instance():
    return _frozen((20003, *_ksat(11, 20003, 80000, 3)))


@functools.lru_cache(maxsize=None)
def b_instance():
    return _frozen((2003, *_ksat(5, 2003, 8000, 3)))


A_CUBES = {"A1": (1100, 14), "A2": (1000, 18), "A3": (1000, 1), "A4": (1000, 0)}
B_CUBES = {"B1": (120, 2), "B2": (120, 14), "B3": (100, 5)}
# cubes of B's instance that propagate to a fixpoint: the live cubes of the portfolio test
B_LIVE_CUBES = {"B4": (100, 0), "B5": (100, 1)}


def chain(n, mul, links):
    """(!x_p(i) | x_p(i+1)) for i < links, p(i) = mul * i mod n, stored in reverse order; x_p(0) pinned 1."""
    p = (mul * np.arange(links + 1, dtype=np.int64)) % n
    assert np.unique(p).size == p.size
    offs, lits = csr([[neg(int(p[i])), pos(int(p[i + 1]))] for i in reversed(range(links))])
    thr = np.full(n, FAIR, np.uint32)
    thr[p[0]] = PIN1
    return offs, lits, thr, p


# Cases G (800 pins on the power-law instance) and H (the mixed instance of widths 1-9) were meant to
# run three and two rounds; on these instances no cube does, and the reference shows why: every one of 1500 cubes of 800 pins on the power-law instance (seeds 0 .. 1499)
# ends in a conflict at round 0 or after one round (its hubs are forced at once, both ways), and the
# mixed instance of widths 1-9 has contradicting one-literal clauses, so that even without a pin it is
# in conflict after its first round.  G and H keep those instances, with the cube seed that forces the
# most; G2 (the same instance under 400 pins: three rounds, nine hot variables forced, then a
# conflict) and H2 (widths 2-9: six rounds to a fixpoint) are the cases with several rounds on the
# hot and the ragged layout.
G_CUBE, G2_CUBE, H_CUBE, H2_CUBE = (800, 7), (400, 18), (5, 1), (300, 9)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in A_CUBES:
        n, offs, lits = a_instance()
        return _frozen(_case(name, n, offs, lits, cube(n, *A_CUBES[name])))
    if name in B_CUBES or name in B_LIVE_CUBES:
        n, offs, lits = b_instance()
        return _frozen(_case(name, n, offs, lits, cube(n, *{**B_CUBES, **B_LIVE_CUBES}[name])))
    if name in ("C", "C_cap"):
        offs, lits, thr, _ = chain(20003, 4099, 299)
        return _frozen(_case(name, 20003, offs, lits, thr, 100 if name == "C_cap" else 0))
    if name == "C'":
        offs, lits, thr, _ = chain(2003, 409, 99)  # (100 variables in a chain: 99 clauses)
        return _frozen(_case(name, 2003, offs, lits, thr))
    if name == "D":
        offs, lits = csr([[neg(0), pos(1)], [neg(0), neg(1)], [pos(2), pos(3)]])
        thr = np.full(4, FAIR, np.uint32)
        thr[0] = PIN1
        return _frozen(_case(name, 4, offs, lits, thr))
    if name == "E":
        offs, lits = csr([[pos(0), pos(0), neg(1)], [pos(2), neg(2)], [pos(3)],
                          [neg(3), pos(4), pos(4), pos(4)] + [neg(1)] * 5 + [pos(5)]])
        thr = np.full(6, FAIR, np.uint32)
        thr[1], thr[5], thr[2] = PIN1, 0, 0x40000000
        return _frozen(_case(name, 6, offs, lits, thr))
    if name == "F":
        offs, lits = csr([[pos(0)], []])
        return _frozen(_case(name, 1, offs, lits, np.full(1, FAIR, np.uint32)))
    if name in ("G", "G2"):  # the powerlaw_hot instance of test_gpu_parity.py: hub variables, flagged hot on the device
        from alllsatisfiabilitysolver_amd import generate_ksat

        n = 20000
        offs, lits = generate_ksat(1, n, 80000, 3, 1)
        return _frozen(_case(name, n, offs, lits, cube(n, *(G_CUBE if name == "G" else G2_CUBE))))
    if name in ("H", "H2"):  # mixed widths with repeated variables, as bias_cases.mixed_case: the ragged layout
        from alllsatisfiabilitysolver_amd import generate_mixed

        n = 9001
        offs, lits = generate_mixed(5, n, 20000, 1 if name == "H" else 2, 9)
        return _frozen(_case(name, n, offs, lits, cube(n, *(H_CUBE if name == "H" else H2_CUBE))))
    raise KeyError(name)


ALL_CASES = [*A_CUBES, *B_CUBES, "C", "C_cap", "C'", "D", "E", "F", "G", "G2", "H", "H2"]
BATCH_CASES = [*B_CUBES, "C'", "D", "E", "F"]  # (every one fits a batch item)

# ---------------------------------------------------------------------------------------------
# Many items (tests/test_gpu_prop_swarm.py): the group and the batch form past their first trip.
# A many-item case is dict(items, seeds, thrs, outs, ress): per item (n, offs, lits), its 64-bit seed,
# its thresholds (None: the item has none), the reference's propagated thresholds (None) and result.

RUN_STEPS = 3  # iterations the GPU tests make after the propagation


def none_result(m):
    """What an item without thresholds gets: nothing is looked at."""
    return dict(status=NONE, rounds=0, n_forced=0, conflict_clause=int(m))


def many(items, seeds, thrs, max_rounds=0):
    outs, ress = [], []
    for (n, offs, lits), thr in zip(items, thrs):
        out, res = (None, none_result(len(offs) - 1)) if thr is None else propagate(n, offs, lits, thr, max_rounds)
        outs.append(out)
        ress.append(res)
    return dict(items=items, seeds=seeds, thrs=thrs, outs=outs, ress=ress, max_rounds=max_rounds)


def continued(full, capped):
    """The results of a call without a cap after one that was capped: what the capped call left over."""
    return [dict(f, rounds=f["rounds"] - c["rounds"], n_forced=f["n_forced"] - c["n_forced"])
            for f, c in zip(full["ress"], capped["ress"])]


def many_references(c):
    """Per item (A0, rows) of RUN_STEPS iterations on the oracle: under the propagated thresholds, or
    the unbiased run of an item that has none.  swarm_cases.rows_after reads them."""
    import oracle as o

    import bias_cases

    return _frozen([bias_cases.unbiased_reference(o, *it, s, RUN_STEPS) if out is None
                    else bias_cases.reference(o, *it, s, out, RUN_STEPS)
                    for it, s, out in zip(c["items"], c["seeds"], c["outs"])])


N_LADDER = 130
LADDER_CAPS = (1, 10, 129)
BIAS = 0x40000000


def ladder_kind(j):
    """The variants of the ladder by residue; where two apply the first of this order holds.
    Item 10 and item 11 are plain (the boundary of max_rounds = 10), item 129 is (the longest chain),
    and the conflict items 40 and 117 directly follow the clauseless items 39 and 116."""
    if j % 11 == 6:
        return "clauseless"
    if j % 7 == 5:
        return "conflict"
    if j % 5 == 3:
        return "none"
    return "plain"


def ladder_item(j):
    """n = j + 2 variables: x_0 pinned 1, a chain (!x_i | x_i+1), i < j, stored in reverse, and a
    spare variable x_j+1 under a bias.  plain: j rounds to a fixpoint, j forced.  conflict: one more
    clause (!x_j-1 | !x_j) at index j -- in the round that forces x_j it is a unit the other way, x_j
    is forced both ways and pinned 1, and the next scan finds the clause falsified: a conflict after j
    rounds, j forced.  (A one-literal clause (!x_j) would be a unit from round 0 on and meet the
    chain halfway.)  none: no thresholds, and a one-literal clause (x_0) and an empty clause behind
    the chain: every scan of the union finds a unit and a falsified clause in the item, and nothing
    may change.  clauseless: thresholds and no clause.  -> (n, offs, lits), thr or None."""
    kind, n = ladder_kind(j), j + 2
    clauses = [] if kind == "clauseless" else [[neg(i), pos(i + 1)] for i in reversed(range(j))]
    if kind == "conflict":
        clauses.append([neg(j - 1), neg(j)])
    if kind == "none":
        clauses += [[pos(0)], []]
    thr = np.full(n, FAIR, np.uint32)
    thr[0], thr[j + 1] = PIN1, BIAS
    return (n, *csr(clauses)), None if kind == "none" else thr


def ladder_closed_form(j):
    """What the reference has to find in item j (asserted in tests/test_prop_cases.py)."""
    return {"plain": dict(status=FIXPOINT, rounds=j, n_forced=j, conflict_clause=j),
            "conflict": dict(status=CONFLICT, rounds=j, n_forced=j, conflict_clause=j),
            "none": none_result(j + 2),
            "clauseless": dict(status=FIXPOINT, rounds=0, n_forced=0, conflict_clause=0)}[ladder_kind(j)]


@functools.lru_cache(maxsize=None)
def ladder(N=N_LADDER, max_rounds=0):
    """N items of 1 to 5 words that end in N different rounds, the variants of ladder_kind among them."""
    from swarm_cases import swarm_seed

    pairs = [ladder_item(j) for j in range(N)]
    return _frozen(many([it for it, _ in pairs], [swarm_seed(4000 + j) for j in range(N)], [t for _, t in pairs],
                        max_rounds))


@functools.lru_cache(maxsize=None)
def ladder_references():
    return many_references(ladder())


@functools.lru_cache(maxsize=None)
def mixed_group():
    """Both counting branches of k_prop_apply in one call.  64 one-word rungs of the ladder (chains
    of 1 to 30 links in a scrambled order: the first wave of words is 64 distinct items), the ladder,
    then cases B1 (a fixpoint after 6 rounds), B2 (a conflict after 1) and C' (99 rounds) -- items of
    63 words, which never fill an aligned wave of 64 -- a chain of 40 links over 4099 variables (129
    words: it holds a whole wave, the shuffle sum, and its links fall into that wave and into the two
    that span items), and lfmis_structures.star(2000, 1) with its hub pinned 0: the hub is hot in the
    union (bit 31 of its literals) at a variable index far from 0, and forces its 2000 neighbours in
    one round."""
    from lfmis_structures import star
    from swarm_cases import swarm_seed

    lad = ladder()
    pairs = [ladder_item(1 + (7 * k) % 30) for k in range(64)]
    items, thrs = [it for it, _ in pairs] + list(lad["items"]), [t for _, t in pairs] + list(lad["thrs"])
    for name in ("B1", "B2", "C'"):
        c = case(name)
        items.append((c["n"], c["offs"], c["lits"]))
        thrs.append(c["thr"])
    offs, lits, thr, _ = chain(4099, 1021, 40)
    items.append((4099, offs, lits))
    thrs.append(thr)
    n, offs, lits = star(2000, 1)
    hub = np.full(n, FAIR, np.uint32)
    hub[0] = 0
    items.append((n, offs, lits))
    thrs.append(hub)
    return _frozen(many(items, [swarm_seed(5000 + i) for i in range(len(items))], thrs))


@functools.lru_cache(maxsize=None)
def mixed_group_references():
    return many_references(mixed_group())


PROP_SWARM_AFTER_RUNS = (3, 341, 380)  # the first item with clauses after each run of clauseless items


def prop_swarm_thresholds(i, n, falsify=()):
    """Thresholds of item i of the ragged swarm: two items of three get random ones with pins
    (bias_cases.mixed_thresholds), clauseless items among them, and so do the three items of
    PROP_SWARM_AFTER_RUNS; `falsify`: literals pinned false afterwards.  None: no thresholds."""
    from bias_cases import mixed_thresholds

    if i % 3 == 2 and i not in PROP_SWARM_AFTER_RUNS:
        return None
    return mixed_thresholds(n, 700 + i, must=tuple((l >> 1, PIN1 if l & 1 else 0) for l in falsify))


def first_clause_if_falsifiable(offs, lits):
    """The literals of clause 0, or () where it is empty or holds a variable both ways."""
    c = [int(l) for l in lits[int(offs[0]):int(offs[1])]]
    return tuple(c) if c and len({l >> 1 for l in c}) == len(set(c)) else ()


@functools.lru_cache(maxsize=None)
def prop_swarm(max_rounds=0):
    """The thousand items and 64-bit seeds of swarm_cases.swarm() under prop_swarm_thresholds.  The
    items of PROP_SWARM_AFTER_RUNS have their clause 0 pinned all false where it can be: a conflict
    at round 0 whose clause index in the union is the clause base that a run of clauseless items
    before them shares."""
    from swarm_cases import swarm_case

    c = swarm_case()
    thrs = [prop_swarm_thresholds(i, n, first_clause_if_falsifiable(offs, lits) if i in PROP_SWARM_AFTER_RUNS else ())
            for i, (n, offs, lits) in enumerate(c["items"])]
    return _frozen(many(c["items"], c["seeds"], thrs, max_rounds))


@functools.lru_cache(maxsize=None)
def prop_swarm_references():
    return many_references(prop_swarm())


LIMIT_CHAIN = (8164, 8175, 8186, 8191)      # word 255; the last link forces variable 8191 (literal 16382)
LIMIT_TAIL = 8160                            # forced by (!x_8191 | x_8160): literal 16383 is read, and false
# (pins, cube seed): four rounds and 15 forced; five and 13; a conflict at round 0; four and 32
LIMIT_CUBES = ((300, 0), (300, 7), (400, 1), (500, 1))


@functools.lru_cache(maxsize=None)
def limit_instance():
    """A batch item at every limit: n = 8192 (256 words), 8192 clauses, 24576 literals.
    generate_ksat(21, 8192, 8192, 3) whose last four clauses are replaced by the three links of
    LIMIT_CHAIN and the tail link, stored in reverse, each with its second literal repeated (a
    repeated literal is one literal to the rules, and the literal count stays at the limit)."""
    n = 8192
    offs, lits = _ksat(21, n, n, 3)
    lits = np.array(lits, np.uint32)
    v = LIMIT_CHAIN + (LIMIT_TAIL,)
    links = [[neg(v[i]), pos(v[i + 1]), pos(v[i + 1])] for i in reversed(range(4))]
    lits[-12:] = np.array(links, np.uint32).ravel()
    return _frozen((n, np.asarray(offs, np.uint64), lits))


@functools.lru_cache(maxsize=None)
def limit_item(cs=0):
    """limit_instance under cube LIMIT_CUBES[cs]; whatever the cube says of the chain's variables,
    its start is pinned 1 and the others are free."""
    n, offs, lits = limit_instance()
    thr = cube(n, *LIMIT_CUBES[cs])
    thr[list(LIMIT_CHAIN[1:]) + [LIMIT_TAIL]] = FAIR
    thr[LIMIT_CHAIN[0]] = PIN1
    return _frozen(_case(f"limit{cs}", n, offs, lits, thr))


# the planner's criterion for hot variables (alll_internal.h: HOT_THR_MIN, HOT_MEAN_X)
HOT_THR_MIN, HOT_MEAN_X = 1024, 32


def hot_variables(n, lits):
    """Variables the device flags hot: degree >= max(HOT_THR_MIN, HOT_MEAN_X * (literals / n + 1))."""
    deg = np.bincount(np.asarray(lits, np.int64) >> 1, minlength=n)
    return np.flatnonzero(deg >= max(HOT_THR_MIN, HOT_MEAN_X * (len(lits) // n + 1)))
