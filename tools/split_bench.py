#!/usr/bin/env python3
"""Measures the split scores and the cube splitter on the MI355X; every leg prints
one JSON line (profiles/split/summary.txt keeps them):

  --leg m   bench.py's config M (random 3-SAT, 2.5 M variables / 10 M clauses) under 25,000 random pins:
            propagate_pins(1) (the cube falsifies a clause as given: one k_prop_scan per call) and
            var_scores(with_scores=False), alternated, host wall clock around every call.  Under
            `rocprofv3 --kernel-trace --stats` the same leg gives the device times of k_score_scan and
            k_score_pick_* beside k_prop_scan of the same context in the same run.
  --leg p   the same calls on config C5 (power-law 3-SAT of the same size, no pins): what the hubs'
            contention costs.
            ALLL_SCORE_PLAIN=1 in the environment runs either leg on the scan without the wave's
            aggregation of hot literals.
  --leg s   one split_cubes(depth = 6) on generate_ksat(11, 20003, 80000, 3) as a whole call, with the
            time inside GroupSolver.thresholds / set_thresholds (the host's share) and inside
            propagate_pins / var_scores (the kernels and their round trips) apart.

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


def cube(n, d, cs):
    rng = np.random.default_rng(1000 * d + cs)
    vs = rng.choice(n, d, replace=False)
    val = rng.integers(0, 2, d)
    thr = np.full(n, FAIR, np.uint32)
    thr[vs] = np.where(val == 1, PIN1, 0).astype(np.uint32)
    return thr


def scores_leg(kind, pins):
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, k = 2_500_000, 10_000_000, 3
    offs, lits = generate_ksat(1, n, m, k, kind)
    out = {"leg": "p" if kind else "m", "n_vars": n, "n_clauses": m, "pins": pins,
           "plain_atomics": os.environ.get("ALLL_SCORE_PLAIN", "0")}
    with Solver(n, offs, lits, seed=1) as s:
        if pins:
            s.set_thresholds(cube(n, pins, 0))
        out["record"] = s.var_scores(with_scores=False)  # warm-up: code objects
        prop_ms, score_ms = [], []
        for _ in range(10):
            if pins:
                t0 = time.perf_counter()
                res = s.propagate_pins(1)
                prop_ms.append((time.perf_counter() - t0) * 1e3)
                out["propagate"] = res
            t0 = time.perf_counter()
            rec = s.var_scores(with_scores=False)
            score_ms.append((time.perf_counter() - t0) * 1e3)
            assert rec == out["record"]
        out["var_scores_ms"] = {"median": statistics.median(score_ms), "min": min(score_ms), "max": max(score_ms)}
        if prop_ms:
            out["propagate_pins_ms"] = {"median": statistics.median(prop_ms), "min": min(prop_ms), "max": max(prop_ms)}
    return out


def leg_s():
    from alllsatisfiabilitysolver_amd import GroupSolver, generate_ksat, split_cubes

    n = 20003
    offs, lits = generate_ksat(11, n, 80000, 3)
    spent = {}

    def timed(name):
        fn = getattr(GroupSolver, name)

        def wrapper(self, *a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(self, *a, **kw)
            finally:
                spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t0) * 1e3

        setattr(GroupSolver, name, wrapper)

    for name in ("thresholds", "set_thresholds", "propagate_pins", "var_scores"):
        timed(name)
    split_cubes(n, offs, lits, 1)  # warm-up: code objects
    spent.clear()
    t0 = time.perf_counter()
    leaves = split_cubes(n, offs, lits, 6)
    total = (time.perf_counter() - t0) * 1e3
    status = {}
    for l in leaves:
        status[l["status"]] = status.get(l["status"], 0) + 1
    return {"leg": "s", "n_vars": n, "n_clauses": 80000, "depth": 6, "total_ms": total, "inside_ms": spent,
            "leaves": len(leaves), "status": status,
            "pinned_per_open_leaf": [int(min((l["thr"] != FAIR).sum() for l in leaves if l["thr"] is not None)),
                                     int(max((l["thr"] != FAIR).sum() for l in leaves if l["thr"] is not None))]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["m", "p", "s"])
    leg = ap.parse_args().leg
    print(json.dumps(leg_s() if leg == "s" else scores_leg(1 if leg == "p" else 0, 0 if leg == "p" else 25000)))
