#!/usr/bin/env python3
"""Measures the unit propagation of pinned variables on the MI355X; every leg prints
one JSON line (profiles/propagate/summary.txt keeps them):

  --leg r   a round at bench.py's config M (random 3-SAT, 2.5 M variables / 10 M clauses) with 1 % of
            the variables pinned: the stand-alone evaluation pass of the same context (alll_bench_eval),
            then propagate_pins(max_rounds = 1, 2, 3) and propagate_pins() to the end, host wall clock
            around every call; a call that applies r rounds scans r + 1 times, and the per-round cost
            is the slope of the time over the scans (every call also packs once and refills the
            assignment).  Under `rocprofv3 --kernel-trace --stats`
            the same leg gives the device time of k_prop_scan beside the evaluation kernel's.
  --leg b   a portfolio of 256 cubes of 100 pins on generate_ksat(5, 2003, 8000, 3), max_iters 2000;
  --leg a   64 cubes of 1000 pins on generate_ksat(11, 20003, 80000, 3), max_iters 200:
            solve_cubes and solve_cubes_propagated, alternated, three runs each (wall time of the
            whole call), and from the host helpers the cubes dropped at depth 0 and after propagation
            and the variables forced per surviving cube.

Cubes are drawn as in tests/prop_cases.py.  Run one leg per process, each under a time limit.
"""
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


def leg_r():
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, k = 2_500_000, 10_000_000, 3
    offs, lits = generate_ksat(1, n, m, k)
    thr = cube(n, n // 100, 0)
    out = {"leg": "r", "n_vars": n, "n_clauses": m, "pins": n // 100}
    with Solver(n, offs, lits, seed=1) as s:
        s.set_thresholds(thr)
        out["eval_kernel"] = s.eval_kernel()
        out["eval_ms"] = [s.bench_eval(20)[0] for _ in range(3)]
        s.propagate_pins(1)  # warm-up: code objects
        calls = []  # (cap, rounds applied, scans = rounds + 1, ms)
        for cap in (1, 2, 3, 1, 2, 3, 1, 2, 3):
            s.set_thresholds(thr)
            t0 = time.perf_counter()
            res = s.propagate_pins(cap)
            calls.append((cap, res["rounds"], res["rounds"] + 1, (time.perf_counter() - t0) * 1e3))
        out["calls"] = calls
        scans = sorted({c[2] for c in calls})
        med = {k: statistics.median(c[3] for c in calls if c[2] == k) for k in scans}
        out["call_ms_by_scans"] = med
        if len(scans) > 1:  # scan + apply + the host's read of the record, per round
            out["round_ms"] = (med[scans[-1]] - med[scans[0]]) / (scans[-1] - scans[0])
        s.set_thresholds(thr)
        t0 = time.perf_counter()
        out["to_the_end"] = dict(s.propagate_pins(), ms=(time.perf_counter() - t0) * 1e3)
        out["eval_ms_after"] = s.bench_eval(20)[0]
    return out


def portfolio(n, offs, lits, n_cubes, d, max_iters):
    from alllsatisfiabilitysolver_amd import pinned_conflict, propagate_pins, solve_cubes, solve_cubes_propagated

    thrs = [cube(n, d, cs) for cs in range(n_cubes)]
    cubes = [(2 * np.flatnonzero(t != FAIR) + (t[t != FAIR] == 0)).tolist() for t in thrs]
    depth0 = sum(pinned_conflict(n, offs, lits, t) is not None for t in thrs)
    host = [propagate_pins(n, offs, lits, t)[1] for t in thrs]
    dead = sum(r["status"] == 1 for r in host)
    forced = [r["n_forced"] for r in host if r["status"] != 1]
    out = {"n_vars": n, "n_clauses": len(offs) - 1, "cubes": n_cubes, "pins": d, "max_iters": max_iters,
           "dropped_at_depth_0": depth0, "dropped_after_propagation": dead,
           "forced_per_surviving_cube": {"mean": statistics.mean(forced) if forced else 0, "min": min(forced, default=0),
                                         "max": max(forced, default=0)},
           "rounds_max": max(r["rounds"] for r in host)}
    solve_cubes_propagated(n, offs, lits, cubes[:4], max_iters=2)  # warm-up: code objects
    for prop in (False, True, True, False, False, True):
        t0 = time.perf_counter()
        win, st, _ = (solve_cubes_propagated if prop else solve_cubes)(n, offs, lits, cubes, max_iters=max_iters)
        ms = (time.perf_counter() - t0) * 1e3
        r = out.setdefault("propagate" if prop else "plain", {"ms": [], "winner": win,
                                                              "winner_iterations": st and st["n_iterations"]})
        r["ms"].append(ms)
    return out


def leg_b():
    from alllsatisfiabilitysolver_amd import generate_ksat

    return dict(portfolio(2003, *generate_ksat(5, 2003, 8000, 3), 256, 100, 2000), leg="b")


def leg_a():
    from alllsatisfiabilitysolver_amd import generate_ksat

    return dict(portfolio(20003, *generate_ksat(11, 20003, 80000, 3), 64, 1000, 200), leg="a")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["r", "b", "a"])
    print(json.dumps({"r": leg_r, "b": leg_b, "a": leg_a}[ap.parse_args().leg]()))
