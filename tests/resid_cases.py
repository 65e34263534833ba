"""The residual formula under the pins (test-side only): a numpy restatement of the
semantics of include/alll.h and of the lift -- nothing of the code under test; the propagation is
prop_cases.propagate -- and the cases of the residual tests.  A case is computed once per process and
shared, read-only, by the CPU module that pins its facts (tests/test_resid_cases.py), the host tests
and the GPU tests.

Why these sizes.  Every pass of the device works in tiles of TILE = 256 clauses or assignment words,
and one workgroup of TILE lanes scans the tile sums, TILE of them per trip.  Case A (20003 variables,
80000 clauses) has 313 clause tiles -- two trips of the clause and literal scans -- but only 626
words, three word tiles.  The scan-size case Z makes every one of the three scans take a second trip:
  clause tiles  = ceil(70001 / 256)                 = 274 > 256
  word tiles    = ceil(ceil(2100003 / 32) / 256)    = ceil(65626 / 256) = 257 > 256
(the smallest such sizes are 65537 clauses and 32 * 65536 + 1 = 2097153 variables; Z stays a little
above them so that the second trip holds more than one tile and the last word is ragged).  B is the
instance of the portfolio tests, PL has hub literals (flagged hot on the device), R is the ragged
layout, W is the instance whose residuals fit a batch item while it does not; the crafted cases are
the corners of the semantics."""
import functools

import numpy as np

import prop_cases as P
from bias_cases import _frozen

PIN1, FAIR = P.PIN1, P.FAIR
TILE = 256
Z_VARS, Z_CLAUSES, Z_PINS = 2100003, 70001, 700000


def _ceil(a, b):
    return -(-a // b)


assert _ceil(Z_CLAUSES, TILE) == 274 > TILE and _ceil(_ceil(Z_VARS, 32), TILE) == 257 > TILE


def residual(n, offs, lits, thr=None):
    """The residual of alll.h on the CPU -> the dict of residual_instance."""
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
    kept = np.bincount(cl, true, m) == 0       # no true literal (an empty and a falsified clause too)
    occ = free & kept[cl]                      # the free occurrences of kept clauses, in their order
    f = np.bincount(cl, occ, m).astype(np.int64)
    var_kept = np.zeros(n, bool)
    var_kept[v[occ]] = True
    var_map = np.flatnonzero(var_kept)
    new = np.cumsum(var_kept) - 1
    offsets = np.zeros(int(kept.sum()) + 1, np.uint64)
    offsets[1:] = np.cumsum(f[kept])
    dead = np.flatnonzero(kept & (f == 0))
    return dict(n_vars=int(var_map.size), n_clauses=int(kept.sum()), n_literals=int(occ.sum()), offsets=offsets,
                literals=(2 * new[v[occ]] + (lits[occ] & 1)).astype(np.uint32), var_map=var_map.astype(np.uint32),
                clause_map=np.flatnonzero(kept).astype(np.uint64),
                thr=np.full(var_map.size, FAIR, np.uint32) if thr is None else np.asarray(thr, np.uint32)[var_map],
                n_falsified=int(dead.size), first_falsified=int(dead[0]) if dead.size else m)


def lift(n, thr, var_map, words_res):
    """The lift of alll.h: pins kept, kept variables copied, the rest 0 -> ceil(n / 32) words."""
    bits = np.zeros(32 * ((n + 31) // 32), np.uint8)
    if thr is not None:
        bits[:n][np.asarray(thr, np.uint32) == PIN1] = 1
    res = np.unpackbits(np.ascontiguousarray(words_res, np.uint32).view(np.uint8), bitorder="little")
    bits[np.asarray(var_map, np.int64)] = res[:len(var_map)]
    return np.packbits(bits, bitorder="little").view(np.uint32)


def violated(offs, lits, words):
    """The clauses without a true literal under the bit-packed assignment, ascending (numpy evaluation)."""
    lits = np.asarray(lits, np.int64)
    m = len(offs) - 1
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")
    true = bits[lits >> 1] != (lits & 1)
    cl = np.repeat(np.arange(m), np.diff(np.asarray(offs, np.int64)))
    return np.flatnonzero(np.bincount(cl, true, m) == 0)


def satisfied(offs, lits, words):
    """Every clause has a true literal under the bit-packed assignment."""
    return violated(offs, lits, words).size == 0


def greedy_model(n, offs, lits):
    """A model found by decisions (the first free literal of the first unsatisfied clause) with unit
    propagation and no backtracking, bit-packed -- or None where that search fails.  It finds one on
    formulas far below the satisfiability threshold; it is no solver."""
    offs, lits = np.asarray(offs, np.int64).tolist(), np.asarray(lits, np.int64).tolist()
    clauses = [lits[offs[j]:offs[j + 1]] for j in range(len(offs) - 1)]
    occ = {}
    for j, c in enumerate(clauses):
        for l in c:
            occ.setdefault(l, []).append(j)
    val = [-1] * n

    def true(l):
        return val[l >> 1] == 1 - (l & 1)

    def assign(l):
        stack = [l]
        while stack:
            l = stack.pop()
            if val[l >> 1] != -1:
                if not true(l):
                    return False
                continue
            val[l >> 1] = 1 - (l & 1)
            for j in occ.get(l ^ 1, ()):
                c = clauses[j]
                if any(true(x) for x in c):
                    continue
                free = {x for x in c if val[x >> 1] == -1}
                if not free:
                    return False
                if len(free) == 1:
                    stack.append(free.pop())
        return True

    for c in clauses:
        if not c or (len(set(c)) == 1 and not assign(c[0])):
            return None
    for c in clauses:
        if not any(true(x) for x in c):
            free = [x for x in c if val[x >> 1] == -1]
            if not free or not assign(free[0]):
                return None
    bits = np.array([int(v == 1) for v in val] + [0] * (-n % 32), np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint32)


def widths(r, upto=3):
    """How many residual clauses have 0, 1, .. upto literals."""
    return np.bincount(np.diff(r["offsets"].astype(np.int64)), minlength=upto + 1)[:upto + 1].tolist()


def same(got, want):
    """The first difference between two residual dicts, or None."""
    for k in ("n_vars", "n_clauses", "n_literals", "n_falsified", "first_falsified"):
        if got[k] != want[k]:
            return f"{k}: {got[k]} != {want[k]}"
    for k in ("offsets", "literals", "var_map", "clause_map", "thr"):
        if k in got and (got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])):
            return f"{k} differs ({got[k].dtype}[{got[k].size}], {want[k].dtype}[{want[k].size}])"
    return None


def counts(r):
    return {k: r[k] for k in ("n_vars", "n_clauses", "n_literals", "n_falsified", "first_falsified")}


@functools.lru_cache(maxsize=None)
def instance(name):
    from alllsatisfiabilitysolver_amd import generate_ksat

    import split_cases

    if name == "W":
        return _frozen((30011, *generate_ksat(7, 30011, 2500, 3)))
    if name == "Z":
        return _frozen((Z_VARS, *generate_ksat(13, Z_VARS, Z_CLAUSES, 3)))
    return split_cases.instance(name)


def _propagated(n, offs, lits, thr):
    out, res = P.propagate(n, offs, lits, thr)
    assert res["status"] == P.FIXPOINT
    return out


# name -> (instance, thresholds): None, ("thr" | "out", a prop_cases case), or a function of the instance
INSTANCE_CASES = {
    "A": ("A", None), "A1p": ("A", ("out", "A1")), "A4": ("A", ("thr", "A4")), "A4p": ("A", ("out", "A4")),
    "A2c": ("A", ("out", "A2")),   # after its propagation's conflict: the thresholds of the failing round's start
    "A3": ("A", ("thr", "A3")),    # a raw cube with falsified clauses
    "B1p": ("B", ("out", "B1")), "B4p": ("B", ("out", "B4")), "B5p": ("B", ("out", "B5")),
    "PL": ("PL", None), "PLG2": ("PL", ("thr", "G2")),
    "W": ("W", None), "W64": ("W", lambda n, o, l: P.cube(n, 64, 1)),
    "W3000p": ("W", lambda n, o, l: _propagated(n, o, l, P.cube(n, 3000, 2))),
    "R": ("R", ("out", "H2")),     # mixed widths 2-9 under a cube that propagates to a fixpoint: the ragged layout
    "Z": ("Z", lambda n, o, l: P.cube(n, Z_PINS, 3)),
}
FAR_LOW, FAR_HIGH = 7, 300 * 32 + 10  # words 0 and 300: two word tiles
CRAFTED = ["repeat", "taut", "dead", "sat_bias", "all_sat", "far", "null_thr"]
ALL_CASES = [*INSTANCE_CASES, *CRAFTED]
FLAG_CASES = ["A4p", "PL", "R", "Z"]  # also under GENERIC_CSR, NO_GRAPH and ATOMIC_CLAIMS
FIXPOINT_CASES = ["A1p", "A4p", "B1p", "B4p", "B5p", "W3000p", "R"]  # n_falsified == 0 and no unit left


def _crafted(name):
    from split_cases import csr_case

    pos, neg = P.pos, P.neg
    if name == "repeat":    # x x !y with y pinned 1 becomes x x
        return csr_case(name, 2, [[pos(0), pos(0), neg(1)]], [(1, PIN1)])
    if name == "taut":      # x !x stays x !x
        return csr_case(name, 1, [[pos(0), neg(0)]])
    if name == "dead":      # an empty clause and a falsified one are kept as empty clauses
        return csr_case(name, 3, [[pos(1), pos(2)], [], [pos(0)], [neg(2)]], [(0, 0)])
    if name == "sat_bias":  # a satisfied clause is dropped; a bias is free and is carried
        return csr_case(name, 4, [[pos(0), pos(1)], [pos(3), neg(2), pos(0)], [neg(3), neg(0)]], [(0, PIN1), (3, 0x40000000)])
    if name == "all_sat":   # the pins satisfy every clause: 0 / 0 / 0
        return csr_case(name, 4, [[pos(0), pos(1)], [neg(2), pos(3)], [pos(0), neg(2), pos(3)]], [(0, PIN1), (2, 0)])
    if name == "far":       # kept variables only in words 0 and 300
        return csr_case(name, FAR_HIGH + 1, [[pos(FAR_HIGH), neg(FAR_LOW)], [pos(5), pos(FAR_HIGH)]], [(5, PIN1)])
    if name == "null_thr":  # no thresholds at all: every variable free, variable 2 never occurs
        c = csr_case(name, 4, [[pos(3), neg(0)], [pos(1)], []])
        c["thr"] = None
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, n, offs, lits, thr or None, res)."""
    if name in INSTANCE_CASES:
        inst, under = INSTANCE_CASES[name]
        n, offs, lits = instance(inst)
        thr = None if under is None else under(n, offs, lits) if callable(under) else P.case(under[1])[under[0]]
        c = dict(name=name, n=n, offs=np.asarray(offs, np.uint64), lits=np.asarray(lits, np.uint32), thr=thr)
    else:
        c = _crafted(name)
    c["res"] = residual(c["n"], c["offs"], c["lits"], c["thr"])
    return _frozen(c)


def many_residuals(c, thrs):
    """Per item of a many-item case of prop_cases its residual under thrs[i] (None: every variable free)."""
    return [residual(n, offs, lits, t) for (n, offs, lits), t in zip(c["items"], thrs)]


W_CUBES = 4


@functools.lru_cache(maxsize=None)
def w_cubes():
    """Four cubes of 8 random pins on W, as lists of literals."""
    n = instance("W")[0]
    out = []
    for cs in range(W_CUBES):
        thr = P.cube(n, 8, 40 + cs)
        v = np.flatnonzero(thr != FAIR)
        out.append((2 * v + (thr[v] == 0)).tolist())
    return out


def reference_portfolio(n, offs, lits, cubes):
    """What solve_cubes_residual has to build from `cubes` (none dead at depth 0): per cube that
    propagates to a fixpoint (cube index, propagated thresholds, residual)."""
    import split_cases

    out = []
    for i, cube in enumerate(cubes):
        thr, res = P.propagate(n, offs, lits, split_cases.cube_thr(n, cube))
        if res["status"] != P.CONFLICT:
            out.append((i, thr, residual(n, offs, lits, thr)))
    return out
