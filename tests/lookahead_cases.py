"""The look-ahead cube splitter and the probes of a whole group (test-side only): a
restatement of split_cubes_lookahead as the tree it is, built from probe_cases.reduce,
split_cases.scores and split_cases.cube_thr only -- nothing of the code under test -- and the cases of
the group-probe tests, whose reference is probe_cases.probe per item.  A case is computed once per
process and shared, read-only, by the CPU module that pins its facts (tests/test_lookahead_cases.py),
the host tests and the GPU tests.

Why these sizes: k_probe_apply and k_probe_rows hold a variable per lane, so a wave holds two
assignment words and, in a group whose items have one word each, two items: 130 such items are 65
waves that each span a border, in a second workgroup too.  A layer is 64 probes of every item: items
of 1, 63, 64, 65 and 130 probes side by side are one to three layers with ragged ends, next to an item
without probes and items of other layouts; the 2003 variables of B are eight workgroups of the apply
kernel.  The thousand items of the swarm go past one workgroup of slots in the 64-lane kernels."""
import functools

import numpy as np

import probe_cases as C
import prop_cases as P
import split_cases as S
from bias_cases import _frozen

PIN1, FAIR = P.PIN1, P.FAIR


def split(n, offs, lits, depth, base=(), n_candidates=32):
    """split_cubes_lookahead on the CPU: a node reduces its thresholds (probe_cases.reduce; a conflict: a
    dead leaf, satisfied: a leaf), at `depth` is an open leaf, else splits on the reduction's look-ahead
    variable (none: the arg-max of the scores under the reduced thresholds), preferred literal first.
    -> the list of leaves {cube, status, thr, n_failed, n_necessary, passes}."""
    leaves = []

    def node(cube, thr, level):
        r = C.reduce(n, offs, lits, thr, n_candidates)
        leaf = dict(cube=cube, status=r["status"], thr=None if r["status"] == "conflict" else r["thr"],
                    n_failed=r["n_failed"], n_necessary=r["n_necessary"], passes=r["passes"])
        if r["status"] != "open" or level == depth:
            leaves.append(leaf)
            return
        sc, rec = S.scores(n, offs, lits, r["thr"])
        v = r["lookahead_var"] if r["lookahead_var"] != n else rec["var"]
        p = 2 * v + (0 if int(sc[2 * v]) >= int(sc[2 * v + 1]) else 1)
        for b in (0, 1):
            t = r["thr"].copy()
            t[v] = 0 if (p ^ b) & 1 else PIN1
            node(cube + [p ^ b], t, level + 1)

    node([int(l) for l in base], S.cube_thr(n, base), 0)
    return leaves


# a: 0, b: 1, c: 2 and g: 3: probe_cases.FAIL_BOTH with every clause guarded by !g, joined with free clauses
# over g and 4 .. 6.  Under g = 1 both literals of a fail, which no unit propagation finds: the root (one
# candidate) splits on g, and the child g = 1 is a conflict leaf found by failed literals alone
G = 3
CRAFTED_CLAUSES = [[P.neg(G)] + c for c in C.FAIL_BOTH] + [[P.pos(G), P.pos(4), P.pos(5)], [P.neg(4), P.pos(5), P.pos(G)],
                                                           [P.pos(4), P.neg(5), P.neg(6)], [P.pos(6), P.pos(4), P.neg(G)]]


@functools.lru_cache(maxsize=None)
def crafted():
    """7 variables, 8 clauses of width 3."""
    return _frozen((7, *P.csr(CRAFTED_CLAUSES)))


def b_cube_base():
    """The pins of cube(2003, *B_FAIL_CUBE) as a cube."""
    thr = P.cube(2003, *C.B_FAIL_CUBE)
    v = np.flatnonzero(thr != FAIR)
    return tuple((2 * v + (thr[v] == 0)).tolist())


# name -> (instance, depth, base, n_candidates)
SPLIT_CASES = {"S40_8": ("S40", 6, (), 8), "S40_32": ("S40", 6, (), 32), "S33_8": ("S33", 6, (), 8),
               "random14": ("random14", 3, (), 4), "crafted": ("crafted", 2, (), 1), "B_16": ("B", 3, None, 16),
               "B_32": ("B", 3, None, 32)}


def split_input(name):
    """(n, offs, lits, depth, base, n_candidates)."""
    inst, depth, base, k = SPLIT_CASES[name]
    if inst == "random14":
        n, offs, lits = C.small_random()
    elif inst == "crafted":
        n, offs, lits = crafted()
    else:
        n, offs, lits = S.instance(inst)
    return n, np.asarray(offs, np.uint64), np.asarray(lits, np.uint32), depth, (b_cube_base() if base is None else base), k


@functools.lru_cache(maxsize=None)
def split_case(name):
    n, offs, lits, depth, base, k = split_input(name)
    return _frozen(split(n, offs, lits, depth, base, k))


def same_leaves(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for j, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b) == {"cube", "status", "thr", "n_failed", "n_necessary", "passes"}, j
        assert {k: v for k, v in a.items() if k != "thr"} == {k: v for k, v in b.items() if k != "thr"}, j
        assert (a["thr"] is None) == (b["thr"] is None), j
        if a["thr"] is not None:
            np.testing.assert_array_equal(a["thr"], b["thr"], err_msg=f"leaf {j}")


# ---- the probes of a group: dict(items, thrs, probes, max_rounds, want) with want[i] = (res, pm, pv)

def _item(c, probes=None, max_rounds=0):
    """An item from a case of probe_cases: its own probes and their reference, or others'."""
    if probes is None:
        return (c["n"], c["offs"], c["lits"]), c["thr"], c["probes"], (list(c["res"]), c["pm"], c["pv"])
    probes = np.asarray(probes, np.uint32)
    return (c["n"], c["offs"], c["lits"]), c["thr"], probes, C.probe(c["n"], c["offs"], c["lits"], c["thr"], probes, max_rounds)


def _group(parts, max_rounds=0):
    return _frozen(dict(items=[p[0] for p in parts], thrs=[p[1] for p in parts], probes=[p[2] for p in parts],
                        max_rounds=max_rounds, want=[p[3] for p in parts]))


ONE_WORD = ["fail_a", "fail_both", "necessary", "pinned", "duplicate", "none_free"]
N_ONE_WORD = 130


@functools.lru_cache(maxsize=None)
def one_word(reverse=False):
    """130 items of 2 to 3 variables, every one probing its case's literals: every wave of the apply and
    rows kernels holds two items."""
    names = [ONE_WORD[i % len(ONE_WORD)] for i in range(N_ONE_WORD)]
    return _group([_item(C.case(x)) for x in (reversed(names) if reverse else names)])


@functools.lru_cache(maxsize=None)
def ragged():
    """B_fail's slices of 1, 63, 64, 65 and 130 probes as five items, B_fail without probes, B_free
    (no thresholds), A4 (fixed width 3 alone; the union is ragged) and H2 (widths 2 to 9)."""
    parts = [_item(c) for c in C.b_slices()]
    parts.append(_item(C.case("B_fail"), probes=[]))
    parts += [_item(C.case(x)) for x in ("B_free", "A4", "H2")]
    return _group(parts)


@functools.lru_cache(maxsize=None)
def capped():
    """Chain C under the call's cap of 100 rounds (probes that end in ROUND_CAP, in FIXPOINT at the cap
    and before it) next to a crafted item the cap never reaches."""
    c = C.case("C_cap")
    return _group([_item(c), _item(C.case("fail_both"), probes=np.arange(6), max_rounds=c["max_rounds"])], c["max_rounds"])


def swarm_probes(n, thr):
    """Both literals of the first free variable and the positive one of the last; none: no probes."""
    free = np.arange(n) if thr is None else C.free_vars(thr)
    return np.array([2 * free[0], 2 * free[0] + 1, 2 * free[-1]] if free.size else [], np.uint32)


@functools.lru_cache(maxsize=None)
def swarm():
    """The thousand items of prop_cases.prop_swarm(), three probes each where the item has a free variable."""
    c = P.prop_swarm()
    parts = []
    for (n, offs, lits), thr in zip(c["items"], c["thrs"]):
        probes = swarm_probes(n, thr)
        parts.append(((n, offs, lits), thr, probes, C.probe(n, offs, lits, thr, probes)))
    return _group(parts)


def check_group(got, c, what=""):
    """What GroupSolver.probes(rows=True) returned against the case's reference, item by item."""
    assert len(got) == len(c["want"]), what
    for i, ((res, pm, pv), (wres, wpm, wpv)) in enumerate(zip(got, c["want"])):
        bad = [(j, r, w) for j, (r, w) in enumerate(zip(res, wres)) if r != w]
        assert len(res) == len(wres) and not bad, (what, i, len(bad), bad[:5])
        assert pm.shape == wpm.shape and pv.shape == wpv.shape, (what, i, pm.shape, wpm.shape)
        np.testing.assert_array_equal(pm, wpm, err_msg=f"{what}: item {i}: pm rows")
        np.testing.assert_array_equal(pv, wpv, err_msg=f"{what}: item {i}: pv rows")


# ---- the layout of plan_group_probes, restated

SLAB, REC_BYTES, MAX_LAYERS = 64, 24, 4096
SLOT_BYTES = SLAB * REC_BYTES + 3 * 8 + 4 + 8


def plan(n_vars, counts, rows, forced=0, budget=1 << 30):
    """The layout for items of n_vars[i] variables and counts[i] probes -> dict(n_layers, max_item_vars,
    nv_pad, n_row_words, row_base, chunks [(layer0, n_layers, n_slots, row_words, bytes)], slots per chunk
    [(slot_base, slot_item, slot_row)]).  The union gives every item whole words."""
    n_vars, counts = np.asarray(n_vars, np.int64), np.asarray(counts, np.int64)
    words = (n_vars + 31) // 32
    word_base = np.concatenate([[0], np.cumsum(words)])[:-1]
    union = int(word_base[-1] * 32 + n_vars[-1]) if n_vars.size else 0
    nv_pad = (union + 63) // 64 * 64
    layers = (counts + SLAB - 1) // SLAB
    n_layers = int(layers.max()) if layers.size else 0
    out = dict(n_layers=n_layers, max_item_vars=int(n_vars[counts > 0].max()) if (counts > 0).any() else 0, nv_pad=nv_pad,
               n_row_words=int((counts * words).sum()), row_base=np.concatenate([[0], np.cumsum(counts * words)]).tolist(),
               chunks=[], slots=[])
    if not counts.sum():
        out["n_layers"] = 0
        return out
    in_layer = lambda l: np.clip(counts - SLAB * l, 0, SLAB)  # noqa: E731
    cost = []
    for l in range(n_layers):
        k = in_layer(l)
        rw = int((k * words).sum()) if rows else 0
        cost.append((int((k > 0).sum()), rw, 32 * nv_pad + int((k > 0).sum()) * SLOT_BYTES + 8 * rw))
    cap = min(forced, MAX_LAYERS) if forced else MAX_LAYERS
    l = 0
    while l < n_layers:
        first, ns, rw, by = l, 0, 0, 0
        while l < n_layers and l - first < cap and (forced or l == first or by + cost[l][2] <= budget):
            ns, rw, by = ns + cost[l][0], rw + cost[l][1], by + cost[l][2]
            l += 1
        out["chunks"].append((first, l - first, ns, rw, by))
        own = np.clip(layers - first, 0, l - first)
        base = np.concatenate([[0], np.cumsum(own)])
        item, row = [], [0]
        for i in np.flatnonzero(own).tolist():
            for y in range(int(own[i])):
                item.append(i)
                row.append(row[-1] + (int(in_layer(first + y)[i] * words[i]) if rows else 0))
        out["slots"].append((base.tolist(), item, row))
    return out
