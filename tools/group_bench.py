#!/usr/bin/env python3
"""Measures the group path (GroupSolver) on the MI355X and writes
profiles/group/summary.txt:

  (a) 64 seeds of random 3-SAT with 5,000 variables / 20,000 clauses, max_iters 500: one
      GroupSolver against one Solver(...).solve() after another;
  (b) 16 items of 25,000 variables / 100,000 clauses, measured the same way;
  (c) 64 items at the batch limits (8,192 variables / 8,192 clauses), GroupSolver against
      BatchSolver.

Every leg runs in a child process of its own under a time limit; after a leg that fails, is killed
or times out, nothing more is started.  Times are host wall clock around calls that end in a device
synchronise, after a warm-up of the same shapes; the contenders alternate, RUNS times each, and the
median is reported with every run beside it.  Every result of the group (statistics and
assignments) is checked against the other contender's.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 5
LEG_TIMEOUT = {"a": 300, "b": 300, "c": 120}
KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
SHAPES = {"a": (5000, 20000, 64, 500, True), "b": (25000, 100000, 16, 500, False), "c": (8192, 8192, 64, 500, False)}


def problems_of(leg):
    from alllsatisfiabilitysolver_amd import generate_ksat

    n, m, items, cap, one_instance = SHAPES[leg]
    if one_instance:
        p = (n, *generate_ksat(1, n, m, 3))
        return [p] * items, list(range(1, items + 1)), cap
    return [(n, *generate_ksat(1 + i, n, m, 3)) for i in range(items)], list(range(1, items + 1)), cap


def run_many(cls, problems, seeds, cap):
    """-> (create s, solve s, results, assignments) of one GroupSolver / BatchSolver."""
    t0 = time.perf_counter()
    with cls(problems, seeds, max_iters=cap) as g:
        t1 = time.perf_counter()
        res = g.solve()
        t2 = time.perf_counter()
        A = [g.assignment_words(i) for i in range(len(problems))]
    return t1 - t0, t2 - t1, [{k: r[k] for k in KEYS} for r in res], A


def run_sequence(problems, seeds, cap):
    from alllsatisfiabilitysolver_amd import Solver

    create = solve = 0.0
    res, A = [], []
    for (n, offs, lits), sd in zip(problems, seeds):
        t0 = time.perf_counter()
        with Solver(n, offs, lits, seed=sd, max_iters=cap) as s:
            t1 = time.perf_counter()
            st = s.solve()
            t2 = time.perf_counter()
            A.append(s.assignment_words())
        create += t1 - t0
        solve += t2 - t1
        res.append({k: st[k] for k in KEYS})
    return create, solve, res, A


def leg(name):
    import numpy as np
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver

    problems, seeds, cap = problems_of(name)
    other = (lambda: run_many(BatchSolver, problems, seeds, cap)) if name == "c" else (lambda: run_sequence(problems, seeds, cap))
    group = lambda: run_many(GroupSolver, problems, seeds, cap)
    group(), other()  # warm-up: code objects, allocator, the same shapes
    g_runs, o_runs, equal = [], [], True
    for _ in range(RUNS):  # alternate the contenders
        gc, gs, gres, gA = group()
        oc, os_, ores, oA = other()
        g_runs.append((gc, gs))
        o_runs.append((oc, os_))
        equal = equal and gres == ores and all(np.array_equal(x, y) for x, y in zip(gA, oA))
    iters = sum(r["n_iterations"] for r in gres)
    print(json.dumps({"leg": name, "items": len(problems), "n_vars": SHAPES[name][0], "n_clauses": SHAPES[name][1],
                      "max_iters": cap, "iterations_all_items": iters, "solved": sum(r["solved"] for r in gres),
                      "max_item_iterations": max(r["n_iterations"] for r in gres),
                      "group_solve_ms": [1e3 * s for _, s in g_runs], "group_create_ms": [1e3 * c for c, _ in g_runs],
                      "other_solve_ms": [1e3 * s for _, s in o_runs], "other_create_ms": [1e3 * c for c, _ in o_runs],
                      "other": "BatchSolver" if name == "c" else "Solver sequence", "equal": equal}))


def fmt(r):
    med = statistics.median
    gs, os_ = med(r["group_solve_ms"]), med(r["other_solve_ms"])
    gt = med([a + b for a, b in zip(r["group_solve_ms"], r["group_create_ms"])])
    ot = med([a + b for a, b in zip(r["other_solve_ms"], r["other_create_ms"])])
    runs = lambda v: " ".join(f"{x:.2f}" for x in v)
    per_it = 1e3 * gs / max(1, r["max_item_iterations"])
    return "\n".join([
        f"({r['leg']}) {r['items']} items, {r['n_vars']} variables / {r['n_clauses']} clauses, max_iters {r['max_iters']}: "
        f"{r['iterations_all_items']} iterations in all, {r['solved']} items solved, longest item {r['max_item_iterations']}",
        f"    group            solve {gs:10.2f} ms   with create {gt:10.2f} ms   ({per_it:.1f} us per union iteration)   runs: {runs(r['group_solve_ms'])}",
        f"    {r['other']:<16} solve {os_:10.2f} ms   with create {ot:10.2f} ms   runs: {runs(r['other_solve_ms'])}",
        f"    time of the {r['other']} / time of the group: {os_ / gs:.2f} (solve), {ot / gt:.2f} (with create)",
        f"    results equal (statistics and assignments, every run): {'yes' if r['equal'] else 'NO'}", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group", "summary.txt"))
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg)
    out = [f"Group path on one MI355X (tools/group_bench.py); host wall clock around synchronising calls, median of {RUNS} "
           "alternated runs after a warm-up.", ""]
    for name in sorted(SHAPES):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True,
                           timeout=LEG_TIMEOUT[name])
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"leg {name} failed with status {p.returncode}: nothing more is started")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(r), flush=True)
        out.append(fmt(r))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
