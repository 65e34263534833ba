"""Failed-literal probing (test-side only): the reference of a probe is
prop_cases.propagate -- the numpy restatement of the rounds of include/alll.h, pinned on its own in
tests/test_prop_cases.py -- applied to the thresholds with the probe's pin, nothing of the code under
test; a restatement of failed_literal_reduce built from it and from split_cases.scores; and the cases
of the probe tests.  A case is computed once per process and shared, read-only, by the CPU module that
pins its facts (tests/test_probe_cases.py), the host tests and the GPU tests.

Why these sizes: a slab is 64 probes, so slices of 1, 63, 64, 65 and 130 probes are its edges and
3422 probes are 54 slabs with a ragged last one; k_probe_apply and k_probe_rows hold a variable per
lane, 256 per workgroup, k_probe_scan a clause per lane: the 20003 variables and 80000 clauses of A4
are 79 and 313 workgroups with a ragged last assignment word; chain C keeps one slab's probes ending
in 43 different rounds over some 300; G2 is the hot-flagged layout, H2 the ragged one (widths 2 to 9:
both sides of the width the scan keeps in registers); the crafted cases are the corners of the
semantics."""
import functools

import numpy as np

import prop_cases as P
import split_cases as S
from bias_cases import _frozen

PIN1, FAIR = P.PIN1, P.FAIR
pos, neg = P.pos, P.neg


def pack_rows(thr):
    """(pm, pv) words of thresholds thr: the pinned variables and their values."""
    n = len(thr)
    bits = np.zeros((2, 32 * ((n + 31) // 32)), np.uint8)
    bits[0, :n] = (thr == 0) | (thr == PIN1)
    bits[1, :n] = thr == PIN1
    w = np.packbits(bits, axis=1, bitorder="little").view(np.uint32)
    return w[0], w[1]


def rows_thr(base, pm, pv):
    """The propagated thresholds of a probe from its rows and the base thresholds (a bias stays)."""
    n = len(base)
    m = np.unpackbits(np.ascontiguousarray(pm).view(np.uint8), bitorder="little")[:n].astype(bool)
    v = np.unpackbits(np.ascontiguousarray(pv).view(np.uint8), bitorder="little")[:n].astype(bool)
    return np.where(m, np.where(v, PIN1, 0), base).astype(np.uint32)


def probe(n, offs, lits, thr, probes, max_rounds=0):
    """One prop_cases.propagate per probe -> (list of results, pm uint32[n_probes, n_words], pv)."""
    base = np.full(n, FAIR, np.uint32) if thr is None else np.asarray(thr, np.uint32)
    m = len(offs) - 1
    res, pm, pv = [], [], []
    for l in np.asarray(probes, np.int64).tolist():
        v = l >> 1
        if base[v] in (0, PIN1):
            out, r = base, P.none_result(m)
        else:
            t = base.copy()
            t[v] = 0 if l & 1 else PIN1
            out, r = P.propagate(n, offs, lits, t, max_rounds)
        a, b = pack_rows(out)
        res.append(r)
        pm.append(a)
        pv.append(b)
    nw = (n + 31) // 32
    return res, np.array(pm, np.uint32).reshape(len(res), nw), np.array(pv, np.uint32).reshape(len(res), nw)


def free_vars(thr):
    return np.flatnonzero((thr != 0) & (thr != PIN1))


def both_literals(vs):
    vs = np.asarray(vs, np.int64)
    return np.stack([2 * vs, 2 * vs + 1], 1).ravel().astype(np.uint32)


def reduce(n, offs, lits, thr=None, n_candidates=64, max_passes=0):
    """failed_literal_reduce on the CPU from prop_cases.propagate, split_cases.scores and probe above."""
    thr = np.full(n, FAIR, np.uint32) if thr is None else np.array(thr, np.uint32)
    out = dict(status="open", passes=0, n_failed=0, n_necessary=0)
    while True:
        out["passes"] += 1
        out["candidates"], out["lookahead_var"] = [], n
        thr, r = P.propagate(n, offs, lits, thr)
        if r["status"] == P.CONFLICT:
            out["status"] = "conflict"
            break
        sc, rec = S.scores(n, offs, lits, thr)
        if rec["n_open"] == 0:
            out["status"] = "satisfied"
            break
        T = sc[0::2].astype(np.int64) + sc[1::2].astype(np.int64)
        cands = sorted((v for v in range(n) if T[v] > 0), key=lambda v: (-T[v], v))[:n_candidates]
        res, pm, pv = probe(n, offs, lits, thr, both_literals(cands))
        out["candidates"] = [(v, res[2 * i], res[2 * i + 1]) for i, v in enumerate(cands)]
        failed = [(v, [x["status"] == P.CONFLICT for x in (a, b)]) for v, a, b in out["candidates"]]
        if any(all(f) for _, f in failed):
            out["status"] = "conflict"
            break
        pins = {v: 0 if f[0] else 1 for v, f in failed if any(f)}  # the failed literal's negation
        out["n_failed"] += len(pins)
        looks = []
        for i, (v, a, b) in enumerate(out["candidates"]):
            if a["status"] != P.FIXPOINT or b["status"] != P.FIXPOINT:
                continue
            looks.append(((a["n_forced"] + 1) * (b["n_forced"] + 1), int(T[v]), -v))
            ta, tb = rows_thr(thr, pm[2 * i], pv[2 * i]), rows_thr(thr, pm[2 * i + 1], pv[2 * i + 1])
            for u in free_vars(thr).tolist():
                if ta[u] == tb[u] and ta[u] in (0, PIN1) and u not in pins:
                    pins[u] = int(ta[u] == PIN1)
                    out["n_necessary"] += 1
        if looks:
            out["lookahead_var"] = -max(looks)[2]
        if not pins:
            break
        for u, x in pins.items():
            thr[u] = PIN1 if x else 0
        if max_passes and out["passes"] >= max_passes:
            break
    out["thr"] = thr
    return out


def consistent_models(n, offs, lits, thr):
    """The satisfying assignments (as integers, bit v = x_v) that agree with the pins of thr; n <= 16."""
    x = np.arange(1 << n, dtype=np.int64)
    ok = np.ones(x.size, bool)
    for v in range(n):
        if thr[v] in (0, PIN1):
            ok &= ((x >> v) & 1) == (1 if thr[v] == PIN1 else 0)
    for c in range(len(offs) - 1):
        sat = np.zeros(x.size, bool)
        for l in np.asarray(lits[int(offs[c]):int(offs[c + 1])], np.int64).tolist():
            sat |= ((x >> (l >> 1)) & 1) != (l & 1)
        ok &= sat
    return set(x[ok].tolist())


def _case(name, n, offs, lits, thr, probes, max_rounds=0):
    probes = np.asarray(probes, np.uint32)
    res, pm, pv = probe(n, offs, lits, thr, probes, max_rounds)
    return dict(name=name, n=n, offs=np.asarray(offs, np.uint64), lits=np.asarray(lits, np.uint32), thr=thr,
                probes=probes, max_rounds=max_rounds, res=res, pm=pm, pv=pv)


def _fair(n, pins=()):
    thr = np.full(n, FAIR, np.uint32)
    for v, t in pins:
        thr[v] = t
    return thr


CRAFTED = ["fail_a", "fail_both", "necessary", "E_all", "F_all", "pinned", "duplicate", "none_free"]
# a: 0, b: 1, c: 2
FAIL_A = [[neg(0), pos(1)], [neg(0), neg(1)]]
FAIL_BOTH = FAIL_A + [[pos(0), pos(2)], [pos(0), neg(2)]]
NECESSARY = [[neg(0), pos(1)], [pos(0), pos(1)]]  # (a: 0, c: 1)


def crafted_instance(name):
    """(n, offs, lits, thr) of a crafted case."""
    if name == "fail_a":
        return (2, *P.csr(FAIL_A), _fair(2))
    if name in ("fail_both", "duplicate"):
        return (3, *P.csr(FAIL_BOTH), _fair(3))
    if name == "necessary":
        return (2, *P.csr(NECESSARY), _fair(2))
    if name == "E_all":   # repeated literals, x !x, a bias, width 10; the base is no fixpoint
        c = P.case("E")
        return c["n"], c["offs"], c["lits"], c["thr"]
    if name == "F_all":   # an empty clause: a conflict at round 0 whatever is probed
        c = P.case("F")
        return c["n"], c["offs"], c["lits"], None
    if name == "pinned":  # a pinned 0: the probes of a are NONE, those of c run under the base's pin
        return (3, *P.csr(FAIL_BOTH), _fair(3, [(0, 0)]))
    if name == "none_free":  # every variable pinned: a slab without a running probe
        return (3, *P.csr(FAIL_BOTH), _fair(3, [(0, PIN1), (1, PIN1), (2, 0)]))
    raise KeyError(name)


B_FAIL_CUBE = (170, 4)
B_SLICES = (1, 63, 64, 65, 130)
CHAIN_STEP, CHAIN_LINKS, CHAIN_CAP, CHAIN_EDGE = 7, 299, 100, 199


@functools.lru_cache(maxsize=None)
def b_fail_base():
    """b_instance() under cube(2003, 170, 4), propagated -> (thresholds, result)."""
    n, offs, lits = P.b_instance()
    out, res = P.propagate(n, offs, lits, P.cube(n, *B_FAIL_CUBE))
    return _frozen((out, res))


def fixpoint_prefix(n, offs, lits, thr):
    """thr propagated; where that conflicts, the pins of thr in variable order halved until it does not."""
    pins = np.flatnonzero(thr != FAIR)
    k = pins.size
    while True:
        t = np.full(n, FAIR, np.uint32)
        t[pins[:k]] = thr[pins[:k]]
        out, res = P.propagate(n, offs, lits, t)
        if res["status"] == P.FIXPOINT:
            return out, k
        k //= 2


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, n, offs, lits, thr or None, probes, max_rounds, res, pm, pv)."""
    if name in CRAFTED:
        n, offs, lits, thr = crafted_instance(name)
        probes = [0, 0, 1, 0, 5, 0] if name == "duplicate" else np.arange(2 * n)
        return _frozen(_case(name, n, offs, lits, thr, probes))
    if name in ("C", "C_cap"):  # no base pin, no thresholds at all: the probe starts the chain where it stands
        offs, lits, _, p = P.chain(20003, 4099, CHAIN_LINKS)
        starts = list(range(0, CHAIN_LINKS, CHAIN_STEP)) + ([CHAIN_EDGE] if name == "C_cap" else [])
        return _frozen(_case(name, 20003, offs, lits, None, [pos(int(p[i])) for i in starts],
                             CHAIN_CAP if name == "C_cap" else 0))
    if name == "B_fail":
        n, offs, lits = P.b_instance()
        thr = b_fail_base()[0]
        return _frozen(_case(name, n, offs, lits, thr, both_literals(free_vars(thr))))
    if name == "B_free":  # B's instance without thresholds: every variable free
        n, offs, lits = P.b_instance()
        return _frozen(_case(name, n, offs, lits, None, both_literals(np.arange(0, n, 29))))
    if name == "A4":
        c = P.case("A4")
        return _frozen(_case(name, c["n"], c["offs"], c["lits"], c["out"], both_literals(free_vars(c["out"])[:70])))
    if name in ("G2", "H2"):
        c = P.case(name)
        thr, _ = fixpoint_prefix(c["n"], c["offs"], c["lits"], c["thr"])
        return _frozen(_case(name, c["n"], c["offs"], c["lits"], thr, both_literals(free_vars(thr)[:65])))
    raise KeyError(name)


def sliced(c, first, count):
    """Probes [first, first + count) of case c: every probe is independent."""
    s = slice(first, first + count)
    return dict(c, probes=c["probes"][s], res=c["res"][s], pm=c["pm"][s], pv=c["pv"][s])


def b_slices():
    """The slab edges: slices of B_fail that start at its first failed literal."""
    c = case("B_fail")
    first = next(i for i, r in enumerate(c["res"]) if r["status"] == P.CONFLICT)
    return [sliced(c, first, k) for k in B_SLICES]


ALL_CASES = [*CRAFTED, "C", "C_cap", "B_fail", "B_free", "A4", "G2", "H2"]
# name -> (instance, the keywords of the call); necessary1: one candidate, a, whose two probes both force c
REDUCE_CASES = {"B_fail": ("B_fail", {}), "fail_a": ("fail_a", {}), "fail_both": ("fail_both", {}),
                "necessary": ("necessary", {}), "necessary1": ("necessary", dict(n_candidates=1)), "E_all": ("E_all", {}),
                "F_all": ("F_all", {}), "pinned": ("pinned", {}), "random14": ("random14", {}),
                "random14_one_pass": ("random14", dict(max_passes=1)), "random14_3": ("random14", dict(n_candidates=3))}
BRUTE_CASES = [k for k in REDUCE_CASES if k != "B_fail"]


@functools.lru_cache(maxsize=None)
def small_random():
    """A random instance of 14 variables and 28 clauses of widths 2 and 3 (17 models; the reduction
    finds three failed literals and three necessary assignments), for the brute-force soundness test."""
    from alllsatisfiabilitysolver_amd import generate_mixed

    return _frozen((14, *generate_mixed(4, 14, 28, 2, 3)))


def reduce_input(name):
    """(n, offs, lits, thr, keywords) a reduce case starts from: B_fail from its cube, unpropagated."""
    inst, kw = REDUCE_CASES[name]
    if inst == "B_fail":
        n, offs, lits = P.b_instance()
        return n, offs, lits, P.cube(n, *B_FAIL_CUBE), kw
    if inst == "random14":
        return (*small_random(), None, kw)
    return (*crafted_instance(inst), kw)


@functools.lru_cache(maxsize=None)
def reduce_case(name):
    n, offs, lits, thr, kw = reduce_input(name)
    return _frozen(reduce(n, offs, lits, thr, **kw))
