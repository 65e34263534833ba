#!/usr/bin/env python3
"""Measures the residual formula and the portfolio on residuals on the MI355X; every
leg prints one JSON line (profiles/residual/summary.txt keeps them):

  --leg m   bench.py's config M (random 3-SAT, 2.5 M variables / 10 M clauses) under 25,000 random pins:
            propagate_pins(1) (the cube falsifies a clause as given: one k_prop_scan per call),
            residual(with_arrays=False) and residual() alternated, host wall clock around every call.
            Under `rocprofv3 --kernel-trace --stats` the same leg gives the device times of the
            k_resid_* kernels beside k_prop_scan of the same context in the same run.
  --leg a   the payoff on generate_ksat(11, 20003, 80000, 3): eight cubes of 1100 random pins that
            propagate to a fixpoint, solve_cubes_propagated against solve_cubes_residual over the same
            cubes and seeds under one iteration cap: wall clock of the whole call and of the final
            solve() in it, which solver class ran the cubes, iterations per second.
  --leg w   the same on generate_ksat(7, 30011, 2500, 3) with sixteen cubes of 8 random pins: the
            instance does not fit a batch item, every residual does.

Run one leg per process, each under a time limit.  Legs a and w must NOT be run under rocprofv3 until
the cause of the following is known: the one run of leg a under `rocprofv3 --kernel-trace --stats`
ended in a segmentation fault on the host, in a launch under alll_group_solve, within a second of the
runtime's start; the same leg without the profiler runs cleanly."""
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


def ms(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def leg_m():
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, k, pins = 2_500_000, 10_000_000, 3, 25000
    offs, lits = generate_ksat(1, n, m, k)
    out = {"leg": "m", "n_vars": n, "n_clauses": m, "pins": pins}
    with Solver(n, offs, lits, seed=1) as s:
        s.set_thresholds(cube(n, pins, 0))
        out["record"] = s.residual(with_arrays=False)  # warm-up: code objects
        prop_ms, rec_ms, full_ms = [], [], []
        for i in range(10):
            t0 = time.perf_counter()
            out["propagate"] = s.propagate_pins(1)
            prop_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            rec = s.residual(with_arrays=False)
            rec_ms.append((time.perf_counter() - t0) * 1e3)
            assert rec == out["record"]
            if i < 3:
                t0 = time.perf_counter()
                r = s.residual()
                full_ms.append((time.perf_counter() - t0) * 1e3)
                assert {k_: r[k_] for k_ in rec} == rec and int(r["offsets"][-1]) == rec["n_literals"]
        out["propagate_pins_ms"], out["residual_record_ms"], out["residual_arrays_ms"] = ms(prop_ms), ms(rec_ms), ms(full_ms)
    return out


def payoff(leg, n, offs, lits, cubes, max_iters):
    from alllsatisfiabilitysolver_amd import solve_cubes_propagated, solve_cubes_residual, solver

    ran = {}

    def timed(cls):
        fn = cls.solve

        def wrapper(self, *a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(self, *a, **kw)
            finally:
                ran["class"], ran["solve_ms"] = cls.__name__, (time.perf_counter() - t0) * 1e3
                ran["items"] = self.n_items

        cls.solve = wrapper

    timed(solver.BatchSolver)
    timed(solver.GroupSolver)
    seeds = list(range(1, len(cubes) + 1))
    out = {"leg": leg, "n_vars": n, "n_clauses": int(offs.size - 1), "cubes": len(cubes), "max_iters": max_iters}
    for name, fn in (("propagated", solve_cubes_propagated), ("residual", solve_cubes_residual)):
        fn(n, offs, lits, cubes, seeds, max_iters)  # warm-up: code objects
        walls, solves, res = [], [], None
        for _ in range(3):
            ran.clear()
            t0 = time.perf_counter()
            res = fn(n, offs, lits, cubes, seeds, max_iters)
            walls.append((time.perf_counter() - t0) * 1e3)
            solves.append(ran["solve_ms"])
        iters = max_iters if res[0] is None else res[1]["n_iterations"]
        out[name] = {"class": ran["class"], "items": ran["items"], "winner": res[0], "iterations": iters,
                     "wall_ms": ms(walls), "solve_ms": ms(solves),
                     "iterations_per_s_of_solve": iters / (statistics.median(solves) * 1e-3),
                     "iterations_per_s_of_call": iters / (statistics.median(walls) * 1e-3)}
    return out


def literals_of(thr):
    v = np.flatnonzero(thr != FAIR)
    return (2 * v + (thr[v] == 0)).tolist()


def leg_a():
    from alllsatisfiabilitysolver_amd import PROP_FIXPOINT, generate_ksat, propagate_pins

    n = 20003
    offs, lits = generate_ksat(11, n, 80000, 3)
    cubes, cs = [], 0
    while len(cubes) < 8:  # (cubes of 1100 pins that the propagation does not refute)
        thr = cube(n, 1100, cs)
        if propagate_pins(n, offs, lits, thr)[1]["status"] == PROP_FIXPOINT:
            cubes.append(literals_of(thr))
        cs += 1
    return payoff("a", n, offs, lits, cubes, 200)


def leg_w():
    from alllsatisfiabilitysolver_amd import generate_ksat

    n = 30011
    offs, lits = generate_ksat(7, n, 2500, 3)
    return payoff("w", n, offs, lits, [literals_of(cube(n, 8, 40 + cs)) for cs in range(16)], 2000)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["m", "a", "w"])
    print(json.dumps({"m": leg_m, "a": leg_a, "w": leg_w}[ap.parse_args().leg]()))
