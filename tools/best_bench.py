#!/usr/bin/env python3
"""Measures the cost of best-assignment tracking on the MI355X and writes its summary
to --out (section 1 of profiles/best/summary.txt is a copy):

  (m) bench.py's config M (random 3-SAT, 2.5 M variables / 10 M clauses, seed 1): 5 warm-up iterations,
      then 60 timed ones, one context with tracking off and one with it on, in one process, three pairs
      off / on and three on / off; ms per iteration of every run;
  (g) leg (a) of tools/group_bench.py (64 seeds of 5,000 variables / 20,000 clauses, max_iters 500) as
      one GroupSolver.solve(), tracking off against on, alternated, three runs each;
  (b) 256 items of 200 variables / 800 clauses, max_iters 2000, as one BatchSolver.solve(), tracking off
      against on, alternated, three runs each;
  (p) config M with tracking on, 5 + 60 iterations and nothing else: the run to put under
      rocprofv3 --kernel-trace --stats for the average of k_resample_vars_best (never part of --legs).

Every leg runs in a child process of its own under a time limit; after a leg that fails, is killed or
times out, nothing more is started.  Times are host wall clock around calls that end in a device
synchronise, after a warm-up of the same shapes.  With tracking on every leg also checks the records
against the statistics (the record is never above the last pass's count) and that the final
assignments and statistics equal those of the run without tracking.
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

LEG_TIMEOUT = {"m": 400, "g": 300, "b": 120, "p": 200}
KEYS = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
M_SHAPE = (2_500_000, 10_000_000, 3)
WARMUP, STEPS = 5, 60


def m_run(Solver, n, offs, lits, track):
    """-> (ms per iteration, statistics, final words, record or None) of WARMUP + STEPS iterations."""
    with Solver(n, offs, lits, seed=1, track_best=track) as s:
        s.run(WARMUP, sync=False)
        s.synchronize()
        t0 = time.perf_counter()
        s.run(STEPS, sync=False)
        s.synchronize()
        dt = time.perf_counter() - t0
        st = s.stats()
        best = s.best() if track else None
        return dt * 1e3 / STEPS, {k: st[k] for k in KEYS}, s.assignment_words(), best


def leg_m():
    import numpy as np
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, k = M_SHAPE
    offs, lits = generate_ksat(1, n, m, k)
    m_run(Solver, n, offs, lits, False), m_run(Solver, n, offs, lits, True)  # warm-up: code objects, allocator
    off, on, equal, rec = [], [], True, None
    for order in [(False, True)] * 3 + [(True, False)] * 3:
        got = {t: m_run(Solver, n, offs, lits, t) for t in order}
        off.append(got[False][0])
        on.append(got[True][0])
        equal = equal and got[False][1] == got[True][1] and np.array_equal(got[False][2], got[True][2])
        rec = got[True][3]
        equal = equal and rec["n_violated"] <= got[True][1]["n_violated"] and 1 <= rec["iteration"] <= WARMUP + STEPS
    return {"leg": "m", "n_vars": n, "n_clauses": m, "warmup": WARMUP, "steps": STEPS, "off_ms_per_step": off,
            "on_ms_per_step": on, "order": "3 x (off, on), 3 x (on, off)", "equal": equal,
            "record": [rec["n_violated"], rec["iteration"]]}


def leg_p():
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    n, m, k = M_SHAPE
    offs, lits = generate_ksat(1, n, m, k)
    ms, st, _, rec = m_run(Solver, n, offs, lits, True)
    return {"leg": "p", "ms_per_step": ms, "n_violated": st["n_violated"], "record": [rec["n_violated"], rec["iteration"]]}


def many_run(cls, problems, seeds, cap, track):
    with cls(problems, seeds, max_iters=cap) as g:
        if track:
            g.track_best()
        t0 = time.perf_counter()
        res = g.solve()
        dt = time.perf_counter() - t0
        A = [g.assignment_words(i) for i in range(len(seeds))]
        recs = [g.best(i) for i in range(len(seeds))] if track else None
    return dt * 1e3, [{k: r[k] for k in KEYS} for r in res], A, recs


def leg_many(name):
    import numpy as np
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver, generate_ksat

    cls, n, m, items, cap = (GroupSolver, 5000, 20000, 64, 500) if name == "g" else (BatchSolver, 200, 800, 256, 2000)
    p = (n, *generate_ksat(1, n, m, 3))
    problems, seeds = [p] * items, list(range(1, items + 1))
    many_run(cls, problems, seeds, cap, False), many_run(cls, problems, seeds, cap, True)  # warm-up
    off, on, equal = [], [], True
    for order in [(False, True), (True, False), (False, True)]:
        got = {t: many_run(cls, problems, seeds, cap, t) for t in order}
        off.append(got[False][0])
        on.append(got[True][0])
        equal = equal and got[False][1] == got[True][1] and all(np.array_equal(x, y) for x, y in zip(got[False][2], got[True][2]))
        equal = equal and all(r["n_violated"] <= st["n_violated"] and 1 <= r["iteration"] <= st["n_iterations"]
                              for r, st in zip(got[True][3], got[True][1]))
    res = got[True][1]
    return {"leg": name, "solver": cls.__name__, "items": items, "n_vars": n, "n_clauses": m, "max_iters": cap,
            "iterations_all_items": sum(r["n_iterations"] for r in res), "solved": sum(r["solved"] for r in res),
            "off_solve_ms": off, "on_solve_ms": on, "order": "(off, on), (on, off), (off, on)", "equal": equal,
            "best_of_portfolio": min(r["n_violated"] for r in got[True][3]),
            "last_of_portfolio": min(r["n_violated"] for r in res)}


def fmt(r):
    med = statistics.median
    runs = lambda v: " ".join(f"{x:.4f}" for x in v)
    if r["leg"] == "m":
        a, b = r["off_ms_per_step"], r["on_ms_per_step"]
        return "\n".join([
            f"(m) config M ({r['n_vars']} variables / {r['n_clauses']} clauses), {r['warmup']} warm-up + {r['steps']} timed "
            f"iterations, ms per iteration; order {r['order']}",
            f"    tracking off   median {med(a):.4f}   min {min(a):.4f}   max {max(a):.4f}   runs: {runs(a)}",
            f"    tracking on    median {med(b):.4f}   min {min(b):.4f}   max {max(b):.4f}   runs: {runs(b)}",
            f"    on / off (medians): {med(b) / med(a):.4f}; record {r['record'][0]} violated at pass {r['record'][1]}",
            f"    statistics and final assignment equal with and without tracking, every pair: {'yes' if r['equal'] else 'NO'}", ""])
    a, b = r["off_solve_ms"], r["on_solve_ms"]
    return "\n".join([
        f"({r['leg']}) {r['solver']}, {r['items']} items of {r['n_vars']} variables / {r['n_clauses']} clauses, max_iters "
        f"{r['max_iters']}: {r['iterations_all_items']} iterations in all, {r['solved']} solved; solve ms; order {r['order']}",
        f"    tracking off   median {med(a):.3f}   runs: {runs(a)}",
        f"    tracking on    median {med(b):.3f}   runs: {runs(b)}",
        f"    on / off (medians): {med(b) / med(a):.4f}",
        f"    fewest violated clauses over the items: {r['best_of_portfolio']} in the records, {r['last_of_portfolio']} in the last assignments",
        f"    statistics and final assignments equal with and without tracking, every pair: {'yes' if r['equal'] else 'NO'}", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEG_TIMEOUT), help="run one leg in this process, print its JSON line")
    ap.add_argument("--legs", default="mgb")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "best_bench.txt"))
    args = ap.parse_args()
    if args.leg:
        from alllsatisfiabilitysolver_amd import device_count

        if device_count() < 1:
            raise SystemExit("best_bench: no HIP device visible (no fallback)")
        r = leg_m() if args.leg == "m" else leg_p() if args.leg == "p" else leg_many(args.leg)
        print(json.dumps(r), flush=True)
        return 0
    out = ["Best-assignment tracking on one MI355X (tools/best_bench.py); host wall clock around synchronising calls.", ""]
    for name in args.legs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True,
                               timeout=LEG_TIMEOUT[name])
        except subprocess.TimeoutExpired:
            print(f"leg {name}: time limit {LEG_TIMEOUT[name]} s; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"leg {name}: exit {p.returncode}; nothing more is started\n{p.stdout}\n{p.stderr}", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        out.append(fmt(json.loads(line)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
