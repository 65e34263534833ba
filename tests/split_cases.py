"""Split scores and the cube splitter (test-side only): a numpy restatement of the
scores of include/alll.h and of split_cubes -- nothing of the code under test; the propagation is
prop_cases.propagate -- and the cases of the split tests.  A case is computed once per process and
shared, read-only, by the CPU module that pins its facts (tests/test_split_cases.py), the host tests
and the GPU tests.

Why these sizes: k_score_pick_* hold 32 variables per lane, 8192 per 256-lane workgroup, so the 20003
variables of case A make three workgroups with a ragged last word, and its 80000 clauses 313 scan
workgroups; B is the instance of the portfolio tests; the power-law instance has hub literals that
thousands of clauses add to (flagged hot on the device), the mixed one is the ragged layout; the
crafted cases are the corners of the semantics."""
import functools

import numpy as np

import prop_cases as P
from bias_cases import _frozen

PIN1, FAIR = P.PIN1, P.FAIR


def scores(n, offs, lits, thr=None):
    """The scores of alll.h on the CPU -> (S uint64[2 n], {var, score_pos, score_neg, n_open})."""
    lits = np.asarray(lits, np.int64)
    m = len(offs) - 1
    cl = np.repeat(np.arange(m), np.diff(np.asarray(offs, np.int64)))  # the clause of every literal
    v, neg = lits >> 1, (lits & 1).astype(bool)
    if thr is None:
        true, free = np.zeros(lits.size, bool), np.ones(lits.size, bool)
    else:
        t = np.asarray(thr, np.uint32)[v]
        true = t == np.where(neg, 0, PIN1)
        free = ~true & (t != np.where(neg, PIN1, 0))
    open_ = np.bincount(cl, true, m) == 0  # no true literal (an empty and a falsified clause too)
    f = np.bincount(cl, free, m).astype(np.int64)  # free occurrences, with multiplicity
    w = np.int64(1) << (16 - np.minimum(f, 16))
    add = free & open_[cl]
    S = np.zeros(2 * n, np.int64)
    np.add.at(S, lits[add], w[cl[add]])
    T = S[0::2] + S[1::2]
    var = int(np.argmax(T)) if n and T.max() > 0 else n  # (argmax: the lowest index on a tie)
    rec = dict(var=var, score_pos=int(S[2 * var]) if var < n else 0, score_neg=int(S[2 * var + 1]) if var < n else 0,
               n_open=int(open_.sum()))
    return S.astype(np.uint64), rec


def n_ties(S):
    """How many variables hold the largest T."""
    T = S[0::2].astype(np.int64) + S[1::2].astype(np.int64)
    return int((T == T.max()).sum())


def cube_thr(n, cube):
    thr = np.full(n, FAIR, np.uint32)
    for l in cube:
        thr[l >> 1] = 0 if l & 1 else PIN1
    return thr


def split(n, offs, lits, depth, base=()):
    """split_cubes on the CPU, as the tree it is: a node propagates its pins (a conflict: a dead leaf),
    scores (nothing left: a satisfied leaf), and above `depth` has the children preferred literal,
    then its complement -- the first child holds the lower items, so depth-first order is the order of
    the leaves' smallest items.  -> the list of leaves {cube, status, thr}."""
    leaves = []

    def node(cube, thr, level):
        thr, res = P.propagate(n, offs, lits, thr)
        if res["status"] == P.CONFLICT:
            leaves.append(dict(cube=cube, status="conflict", thr=None))
            return
        _, s = scores(n, offs, lits, thr)
        if s["var"] == n:
            leaves.append(dict(cube=cube, status="satisfied", thr=thr))
        elif level == depth:
            leaves.append(dict(cube=cube, status="open", thr=thr))
        else:
            p = 2 * s["var"] + (0 if s["score_pos"] >= s["score_neg"] else 1)
            for b in (0, 1):
                t = thr.copy()
                t[s["var"]] = 0 if (p ^ b) & 1 else PIN1
                node(cube + [p ^ b], t, level + 1)

    node([int(l) for l in base], cube_thr(n, base), 0)
    return leaves


def csr_case(name, n, clauses, pins=()):
    """A crafted case: pins = ((variable, threshold), ...), every other variable a fair coin."""
    offs, lits = P.csr(clauses)
    thr = np.full(n, FAIR, np.uint32)
    for v, t in pins:
        thr[v] = t
    return dict(name=name, n=n, offs=offs, lits=lits, thr=thr)


TIE_LOW, TIE_HIGH = 7, 300 * 32 + 10  # words 0 and 300: two pick workgroups


@functools.lru_cache(maxsize=None)
def instance(name):
    from alllsatisfiabilitysolver_amd import generate_ksat, generate_mixed

    if name == "A":
        return P.a_instance()
    if name == "B":
        return P.b_instance()
    if name == "PL":  # the power-law instance of prop_cases G: hub variables, flagged hot on the device
        return _frozen((20000, *generate_ksat(1, 20000, 80000, 3, 1)))
    if name == "R":   # mixed widths 2-9 with repeated variables: the ragged layout
        return _frozen((9001, *generate_mixed(5, 9001, 20000, 2, 9)))
    if name == "S40":
        return _frozen((40, *generate_ksat(3, 40, 120, 3)))
    if name == "S33":
        return _frozen((33, *generate_ksat(4, 33, 140, 3)))
    raise KeyError(name)


# name -> (instance, the prop_cases case whose propagated thresholds it runs under, or None)
INSTANCE_CASES = {"B": ("B", None), "B1p": ("B", "B1"), "B4p": ("B", "B4"), "B5p": ("B", "B5"),
                  "A": ("A", None), "A1p": ("A", "A1"), "A4p": ("A", "A4"), "PL": ("PL", None), "R": ("R", None)}
CRAFTED = ["wide20", "repeat", "taut", "dead", "sat_bias", "all_sat", "tie_far"]
ALL_CASES = [*INSTANCE_CASES, *CRAFTED]
FLAG_CASES = ["A", "A4p", "PL", "R"]  # also under GENERIC_CSR, NO_GRAPH and ATOMIC_CLAIMS


def _crafted(name):
    pos, neg = P.pos, P.neg
    if name == "wide20":    # 1. sixteen free literals and more weigh 1 each
        return csr_case(name, 20, [[pos(v) for v in range(20)]])
    if name == "repeat":    # 2. x x !y with y pinned 1: f = 2, both occurrences add
        return csr_case(name, 2, [[pos(0), pos(0), neg(1)]], [(1, PIN1)])
    if name == "taut":      # 3. x !x: f = 2
        return csr_case(name, 1, [[pos(0), neg(0)]])
    if name == "dead":      # 4. an empty clause and a falsified one are open and add nothing
        return csr_case(name, 3, [[], [pos(0)], [pos(1), pos(2)]], [(0, 0)])
    if name == "sat_bias":  # 5. a satisfied clause adds nothing; a bias is free
        return csr_case(name, 3, [[pos(0), pos(1)], [pos(1), neg(2)]], [(0, PIN1), (1, 0x40000000)])
    if name == "all_sat":   # the pins satisfy every clause
        return csr_case(name, 4, [[pos(0), pos(1)], [neg(2), pos(3)], [pos(0), neg(2), pos(3)]], [(0, PIN1), (2, 0)])
    if name == "tie_far":   # equal T in words 0 and 300: the lowest variable wins across workgroups
        return csr_case(name, TIE_HIGH + 1, [[pos(TIE_HIGH), pos(TIE_LOW)]])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, n, offs, lits, thr or None, S, rec)."""
    if name in INSTANCE_CASES:
        inst, under = INSTANCE_CASES[name]
        n, offs, lits = instance(inst)
        c = dict(name=name, n=n, offs=np.asarray(offs, np.uint64), lits=np.asarray(lits, np.uint32),
                 thr=None if under is None else P.case(under)["out"])
    else:
        c = _crafted(name)
    c["S"], c["rec"] = scores(c["n"], c["offs"], c["lits"], c["thr"])
    return _frozen(c)


def b4_base():
    """The pins of prop_cases B4's cube as a cube."""
    thr = P.case("B4")["thr"]
    v = np.flatnonzero(thr != FAIR)
    return (2 * v + (thr[v] == 0)).tolist()


# name -> (instance, depth, base)
SPLIT_CASES = {"S40": ("S40", 6, ()), "S33": ("S33", 6, ()), "B_base": ("B", 5, None), "PL": ("PL", 4, ())}


@functools.lru_cache(maxsize=None)
def split_case(name):
    inst, depth, base = SPLIT_CASES[name]
    base = tuple(b4_base()) if base is None else base
    n, offs, lits = instance(inst)
    return _frozen(dict(name=name, n=n, offs=np.asarray(offs, np.uint64), lits=np.asarray(lits, np.uint32), depth=depth,
                        base=base, leaves=split(n, offs, lits, depth, base)))


def many_scores(c, thrs):
    """Per item of a many-item case of prop_cases (S, rec) under thrs[i] (None: every variable free)."""
    return [scores(n, offs, lits, t) for (n, offs, lits), t in zip(c["items"], thrs)]
