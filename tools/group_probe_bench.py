#!/usr/bin/env python3
"""Measures the probes of a whole group and the look-ahead splitter on the MI355X;
every leg prints one JSON line (profiles/group_probe/summary.txt keeps them):

  --leg g   --shape A64: 64 items of generate_ksat(11, 20003, 80000, 3) under 64 different cubes of
            1000 random pins; --shape B1024: 1024 items of generate_ksat(5, 2003, 8000, 3) under cubes
            of 100 pins.  The cubes are propagated; every item that did not conflict probes both
            literals of its 32 free variables of largest T.  Timed, alternated, host wall clock: one
            GroupSolver.probes call for all items against one Solver.probe call per item on contexts
            created, given the same thresholds and propagated outside the timed region.  The records
            of the two are asserted equal.  Under `rocprofv3 --kernel-trace --stats` the leg gives the
            device time of k_probe_scan in both forms (the group's kernel is the GroupProbeArgs
            instantiation).
  --leg s   split_cubes_lookahead, device against host=True, wall clock of the whole call: B under
            cube(2003, 170, 4) at depth 3 with 16 candidates, and A at depth 6 with 32 candidates.

Run one leg per process, each under a time limit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAIR, PIN1 = 1 << 31, 0xFFFFFFFF
SHAPES = {"A64": (11, 20003, 80000, 64, 1000), "B1024": (5, 2003, 8000, 1024, 100)}


def cube(n, d, cs):
    rng = np.random.default_rng(1000 * d + cs)
    vs = rng.choice(n, d, replace=False)
    val = rng.integers(0, 2, d)
    thr = np.full(n, FAIR, np.uint32)
    thr[vs] = np.where(val == 1, PIN1, 0).astype(np.uint32)
    return thr


def spread(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3),
            "max_ms": round(1e3 * max(xs), 3), "runs": len(xs)}


def leg_group(shape, reps, warmup, n_cands):
    from alllsatisfiabilitysolver_amd import GroupSolver, Solver, generate_ksat

    gen, n, m, n_items, pins = SHAPES[shape]
    offs, lits = generate_ksat(gen, n, m, 3)
    g = GroupSolver([(n, offs, lits)] * n_items, range(1, n_items + 1))
    for i in range(n_items):
        g.set_thresholds(i, cube(n, pins, i))
    res = g.propagate_pins()
    live = [i for i, r in enumerate(res) if r["status"] == 0]
    _, scores = g.var_scores(with_scores=True)
    probes = [np.zeros(0, np.uint32)] * n_items
    for i in live:
        S = scores[i]
        T = S[0::2].astype(np.int64) + S[1::2].astype(np.int64)
        order = np.argsort(-T, kind="stable")[:n_cands]
        c = order[T[order] > 0]
        probes[i] = np.stack([2 * c, 2 * c + 1], 1).astype(np.uint32).ravel()
    # the contexts of their own, 64 at a time (a context holds a stream and pinned memory): per block the
    # group call and the block's Solver.probe calls alternate; a repetition's one-after-another time is
    # the sum over the blocks
    t_group, t_single, rounds = [], [0.0] * reps, 0
    for first in range(0, len(live), 64):
        block = live[first:first + 64]
        solvers = {}
        for i in block:
            s = Solver(n, offs, lits, seed=i + 1)
            s.set_thresholds(g.thresholds(i))
            solvers[i] = s
        for rep in range(warmup + reps):
            t0 = time.perf_counter()
            got = g.probes(probes)
            t1 = time.perf_counter()
            own = {i: solvers[i].probe(probes[i]) for i in block}
            t2 = time.perf_counter()
            if rep == 0:
                assert all(got[i] == own[i] for i in block), "the group's records differ from the contexts'"
                rounds = max([rounds] + [r["rounds"] for i in block for r in got[i]])
            if rep >= warmup:
                t_group.append(t1 - t0)
                t_single[rep - warmup] += t2 - t1
        for s in solvers.values():
            s.close()
    out = {"leg": "g", "shape": shape, "n_items": n_items, "live_items": len(live), "probes": int(sum(p.size for p in probes)),
           "max_rounds_run": rounds, "group_call": spread(t_group), "one_after_another": spread(t_single),
           "ratio": round(statistics.median(t_single) / statistics.median(t_group), 2)}
    g.close()
    return out


def leg_split(reps, warmup):
    from alllsatisfiabilitysolver_amd import generate_ksat, split_cubes_lookahead

    out = {"leg": "s"}
    nb, na = 2003, 20003
    b = generate_ksat(5, nb, 8000, 3)
    a = generate_ksat(11, na, 80000, 3)
    thr = cube(nb, 170, 4)
    v = np.flatnonzero(thr != FAIR)
    base = (2 * v + (thr[v] == 0)).tolist()
    for name, args in (("B_depth3_16", (nb, *b, 3, base, 16)), ("A_depth6_32", (na, *a, 6, (), 32))):
        t_dev, t_host, leaves = [], [], None
        for rep in range(warmup + reps):
            t0 = time.perf_counter()
            dev = split_cubes_lookahead(*args)
            t1 = time.perf_counter()
            host = split_cubes_lookahead(*args, host=True)
            t2 = time.perf_counter()
            assert [(l["cube"], l["status"]) for l in dev] == [(l["cube"], l["status"]) for l in host]
            leaves = [l["status"] for l in dev]
            if rep >= warmup:
                t_dev.append(t1 - t0)
                t_host.append(t2 - t1)
        out[name] = {"leaves": len(leaves), "conflict": leaves.count("conflict"), "open": leaves.count("open"),
                     "device": spread(t_dev), "host": spread(t_host)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["g", "s"], required=True)
    ap.add_argument("--shape", choices=list(SHAPES), default="A64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--candidates", type=int, default=32)
    a = ap.parse_args()
    out = leg_group(a.shape, a.reps, a.warmup, a.candidates) if a.leg == "g" else leg_split(a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
