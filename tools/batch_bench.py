#!/usr/bin/env python3
"""Measures the batch path (BatchSolver) on the MI355X and writes
profiles/batch/summary.txt:

  (a) 256 items of the 200-variable / 800-clause instance (gen seed 1), seeds 1..256, max_iters
      2000: through one BatchSolver, and one after another through Solver(...).solve(); every
      batch result (statistics and assignment) is checked against the sequential leg;
  (b) the portfolio of the 200 / 520 instance over seeds 1..256 (solve_portfolio);
  (c) 64 items at the limits (8192 variables, 8192 clauses, 3-SAT), solved;
  (s) the slice rule's input: per-iteration time of one launch of items at the limits that never
      solve (2048 variables, 8192 clauses: ratio 4), 64 and 256 items, several slice lengths;
  (g) the LFMIS choice: the workloads of (b) and (a) with the one-wave serial greedy taking the
      violated sets of at most 0 (never), 4, 16 and 64 clauses (ALLL_BATCH_SERIAL_MAX);
  (u) the batch leg of (a) alone, best of 5, with a digest of every item's result; with --ab-lib
      OTHER.so it runs alternately on this build and on OTHER (ALLL_LIB_AB), three pairs in both
      orders: the unbiased batch of two builds side by side;
  (t) the cost of per-variable thresholds: the workload of (a), and 64 items of
      2048 / 8192 for 256 iterations, unbiased, with every threshold at 2^31 LDS-resident, and
      with the thresholds read from global memory (ALLL_BATCH_THR_GLOBAL=1), in one process;
  (q) a cube portfolio: the 256 cubes of variables 0..7 of the 200 / 520 instance of (b), time
      from create to the first answer in a BatchSolver and in a GroupSolver.

Every leg runs in a child process of its own under a time limit; after a leg that fails, is
killed or times out, nothing more is started.  Times are host wall clock around calls that end
in a device synchronise, after a warm-up of the same shapes.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEG_TIMEOUT = {"a": 240, "b": 60, "c": 60, "s": 120, "g": 60, "u": 60, "t": 120, "q": 120}
SERIAL_MAX = (0, 4, 16, 64)


def leg_a():
    import numpy as np
    from alllsatisfiabilitysolver_amd import BatchSolver, Solver, generate_ksat

    n, m, cap, items = 200, 800, 2000, 256
    offs, lits = generate_ksat(1, n, m, 3)
    seeds = list(range(1, items + 1))
    keys = ("n_iterations", "n_resamples", "sum_mis_size", "avg_mis_size", "n_violated", "solved")
    with BatchSolver([(n, offs, lits)] * 4, seeds[:4], max_iters=50) as b:  # warm-up: code objects
        b.solve()
    with Solver(n, offs, lits, seed=1, max_iters=50) as s:
        s.solve()
    t0 = time.perf_counter()
    with BatchSolver([(n, offs, lits)] * items, seeds, max_iters=cap) as b:
        t1 = time.perf_counter()
        res = b.solve()
        t2 = time.perf_counter()
        A = [b.assignment_words(i) for i in range(items)]
    batch_total, batch_solve = time.perf_counter() - t0, t2 - t1
    seq_solve = 0.0
    t0 = time.perf_counter()
    mismatches = 0
    iters = 0
    for i, sd in enumerate(seeds):
        with Solver(n, offs, lits, seed=sd, max_iters=cap) as s:
            t1 = time.perf_counter()
            st = s.solve()
            seq_solve += time.perf_counter() - t1
            ok = all(st[k] == res[i][k] for k in keys) and np.array_equal(s.assignment_words(), A[i])
            mismatches += not ok
            iters += st["n_iterations"]
    seq_total = time.perf_counter() - t0
    return {"leg": "a", "items": items, "n_vars": n, "n_clauses": m, "max_iters": cap, "iterations": iters,
            "solved": sum(r["solved"] for r in res), "mismatches": mismatches,
            "batch_solve_s": batch_solve, "batch_total_s": batch_total,
            "seq_solve_s": seq_solve, "seq_total_s": seq_total}


def leg_b():
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat, solve_portfolio

    n, m, items = 200, 520, 256
    offs, lits = generate_ksat(1, n, m, 3)
    seeds = list(range(1, items + 1))
    solve_portfolio(n, offs, lits, seeds[:4], max_iters=50)  # warm-up
    t0 = time.perf_counter()
    seed, st, _ = solve_portfolio(n, offs, lits, seeds, max_iters=100000)
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    with BatchSolver([(n, offs, lits)] * items, seeds, max_iters=100000) as b:
        res = b.solve()
    every = time.perf_counter() - t0
    its = sorted(r["n_iterations"] for r in res)
    return {"leg": "b", "items": items, "n_vars": n, "n_clauses": m, "winning_seed": seed,
            "winning_iterations": st["n_iterations"] if st else None, "portfolio_s": first,
            "all_seeds_s": every, "all_solved": sum(r["solved"] for r in res), "iterations_total": sum(its),
            "iterations_min": its[0], "iterations_median": its[len(its) // 2], "iterations_max": its[-1]}


def leg_c():
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat

    n, m, items = 8192, 8192, 64
    offs, lits = generate_ksat(1, n, m, 3)
    seeds = list(range(1, items + 1))
    with BatchSolver([(n, offs, lits)] * 2, seeds[:2], max_iters=3) as b:  # warm-up
        b.solve()
    t0 = time.perf_counter()
    with BatchSolver([(n, offs, lits)] * items, seeds) as b:
        t1 = time.perf_counter()
        res = b.solve()
        t2 = time.perf_counter()
    iters = sum(r["n_iterations"] for r in res)
    return {"leg": "c", "items": items, "n_vars": n, "n_clauses": m, "solved": sum(r["solved"] for r in res),
            "iterations": iters, "iterations_max": max(r["n_iterations"] for r in res),
            "solve_s": t2 - t1, "total_s": time.perf_counter() - t0}


def leg_s():
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat

    n, m = 2048, 8192
    offs, lits = generate_ksat(1, n, m, 3)
    rows = []
    for items in (64, 256):
        with BatchSolver([(n, offs, lits)] * items, list(range(1, items + 1))) as b:
            b.set_slice(8)
            b.run(8)  # warm-up; also past the first iterations' large violated sets
            for sl in (16, 64, 256, 1024):
                b.set_slice(sl)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    st = b.run(sl)  # one launch of sl iterations + the state read-back
                    t.append(time.perf_counter() - t0)
                assert all(r["solved"] == 0 for r in st)
                rows.append({"items": items, "slice": sl, "launch_ms": [x * 1e3 for x in t],
                             "us_per_iteration": min(t) / sl * 1e6, "n_violated_item0": st[0]["n_violated"]})
    return {"leg": "s", "n_vars": n, "n_clauses": m, "rows": rows}


def leg_g():
    """One setting of ALLL_BATCH_SERIAL_MAX (the environment's): best of 5 solves of each workload."""
    from alllsatisfiabilitysolver_amd import BatchSolver, generate_ksat

    out = {"leg": "g", "serial_max": int(os.environ.get("ALLL_BATCH_SERIAL_MAX", "0"))}
    for name, (n, m, cap) in {"portfolio": (200, 520, 100000), "dense": (200, 800, 2000)}.items():
        offs, lits = generate_ksat(1, n, m, 3)
        seeds = list(range(1, 257))
        t, iters = [], 0
        for _ in range(6):  # (the first one warms up)
            with BatchSolver([(n, offs, lits)] * len(seeds), seeds, max_iters=cap) as b:
                t0 = time.perf_counter()
                res = b.solve()
                t.append(time.perf_counter() - t0)
            iters = sum(r["n_iterations"] for r in res)
        out[name] = {"iterations": iters, "solve_ms": [x * 1e3 for x in t[1:]]}
    return out


def _digest(res, words):
    import hashlib

    h = hashlib.sha256()
    keys = ("n_iterations", "n_resamples", "sum_mis_size", "n_violated", "solved")
    for r, w in zip(res, words):
        h.update(repr([r[k] for k in keys]).encode() + w.tobytes())
    return h.hexdigest()[:16]


def _timed_batch(problems, seeds, thr, reps, cap=0, run=0):
    """Best-of-reps input: solve (or run(run)) of one batch, every item under thresholds thr (None: unbiased)."""
    from alllsatisfiabilitysolver_amd import BatchSolver

    t, iters, dig = [], 0, None
    for _ in range(reps + 1):  # (the first one warms up)
        with BatchSolver(problems, seeds, max_iters=cap) as b:
            if thr is not None:
                for i in range(len(seeds)):
                    b.set_thresholds(i, thr)
            t0 = time.perf_counter()
            res = b.run(run) if run else b.solve()
            t.append(time.perf_counter() - t0)
            iters = sum(r["n_iterations"] for r in res)
            dig = _digest(res, [b.assignment_words(i) for i in range(len(seeds))])
    return {"iterations": iters, "digest": dig, "ms": [x * 1e3 for x in t[1:]]}


def leg_u():
    from alllsatisfiabilitysolver_amd import generate_ksat

    n, m, cap, items = 200, 800, 2000, 256
    offs, lits = generate_ksat(1, n, m, 3)
    out = _timed_batch([(n, offs, lits)] * items, list(range(1, items + 1)), None, 5, cap=cap)
    return dict(out, leg="u", lib=os.environ.get("ALLL_LIB_AB", "this build"))


def leg_t():
    import numpy as np
    from alllsatisfiabilitysolver_amd import generate_ksat

    out = {"leg": "t", "rows": []}
    for name, n, m, items, cap, run in (("200/800", 200, 800, 256, 2000, 0), ("2048/8192", 2048, 8192, 64, 0, 256)):
        offs, lits = generate_ksat(1, n, m, 3)
        problems, seeds = [(n, offs, lits)] * items, list(range(1, items + 1))
        half = np.full(n, 1 << 31, np.uint32)
        for mode, thr, env in (("unbiased", None, None), ("thresholds in LDS", half, None),
                               ("thresholds in global memory", half, "1"), ("unbiased again", None, None)):
            os.environ.pop("ALLL_BATCH_THR_GLOBAL", None)
            if env:
                os.environ["ALLL_BATCH_THR_GLOBAL"] = env  # (read at create)
            out["rows"].append(dict(_timed_batch(problems, seeds, thr, 5, cap=cap, run=run), size=name, items=items,
                                    mode=mode))
    os.environ.pop("ALLL_BATCH_THR_GLOBAL", None)
    return out


def leg_q():
    from alllsatisfiabilitysolver_amd import (BatchSolver, GroupSolver, cube_thresholds, generate_ksat,
                                              pinned_conflict)

    n, m, cap = 200, 520, 100000
    offs, lits = generate_ksat(1, n, m, 3)
    cubes = [[2 * v + 1 - ((i >> v) & 1) for v in range(8)] for i in range(256)]
    out = {"leg": "q", "n_vars": n, "n_clauses": m, "cubes": len(cubes)}
    for name, cls in (("batch", BatchSolver), ("group", GroupSolver)):
        t = []
        for rep in range(4):  # (the first one warms up)
            t0 = time.perf_counter()
            thrs = [cube_thresholds(n, c) for c in cubes]
            live = [i for i, x in enumerate(thrs) if pinned_conflict(n, offs, lits, x) is None]
            with cls([(n, offs, lits)] * len(live), [i + 1 for i in live], max_iters=cap) as b:
                for k, i in enumerate(live):
                    b.set_thresholds(k, thrs[i])
                res = b.solve(first_solved=True)
                solved = [k for k, r in enumerate(res) if r["solved"]]
                best = min(solved, key=lambda k: (res[k]["n_iterations"], k))
                b.assignment_words(best)
            t.append(time.perf_counter() - t0)
        out[name] = {"live": len(live), "winner": live[best], "winner_iterations": res[best]["n_iterations"],
                     "ms": [x * 1e3 for x in t[1:]]}
    return out


def summary(r):
    out = ["Batch path on one MI355X (tools/batch_bench.py); host wall clock around synchronising calls.", ""]
    a, b, c, s = (r.get(k) for k in "abcs")
    g = [r[k] for k in sorted(r) if k.startswith("g")]
    if a:
        it = a["iterations"]
        out += [f"(a) {a['items']} items, {a['n_vars']} variables / {a['n_clauses']} clauses, seeds 1..{a['items']}, "
                f"max_iters {a['max_iters']}: {it} iterations in all, {a['solved']} items solved",
                f"    batch      solve {a['batch_solve_s'] * 1e3:10.2f} ms   with create and read-back "
                f"{a['batch_total_s'] * 1e3:10.2f} ms   {it / a['batch_solve_s']:12.0f} it/s aggregate   "
                f"{it / a['batch_solve_s'] / a['items']:10.0f} it/s per item",
                f"    sequential solve {a['seq_solve_s'] * 1e3:10.2f} ms   with create and read-back "
                f"{a['seq_total_s'] * 1e3:10.2f} ms   {it / a['seq_solve_s']:12.0f} it/s (one item at a time)",
                f"    batch over sequential: {a['seq_solve_s'] / a['batch_solve_s']:.1f}x (solve), "
                f"{a['seq_total_s'] / a['batch_total_s']:.1f}x (with create and read-back)",
                f"    results equal to the sequential leg (statistics and assignments): "
                f"{'yes, all ' + str(a['items']) if a['mismatches'] == 0 else 'NO, ' + str(a['mismatches']) + ' differ'}",
                ""]
    if b:
        out += [f"(b) portfolio, {b['n_vars']} variables / {b['n_clauses']} clauses, seeds 1..{b['items']}:",
                f"    first solved: seed {b['winning_seed']} after {b['winning_iterations']} iterations, "
                f"{b['portfolio_s'] * 1e3:.2f} ms (create to answer)",
                f"    every seed to the end: {b['all_solved']} solved, iterations min / median / max "
                f"{b['iterations_min']} / {b['iterations_median']} / {b['iterations_max']}, "
                f"{b['all_seeds_s'] * 1e3:.2f} ms, {b['iterations_total'] / b['all_seeds_s']:.0f} it/s aggregate", ""]
    if c:
        out += [f"(c) {c['items']} items at the limits ({c['n_vars']} variables / {c['n_clauses']} clauses, 3-SAT): "
                f"{c['solved']} solved, {c['iterations']} iterations in all (most {c['iterations_max']})",
                f"    solve {c['solve_s'] * 1e3:.2f} ms, with create {c['total_s'] * 1e3:.2f} ms, "
                f"{c['iterations'] / c['solve_s']:.0f} it/s aggregate, "
                f"{c['iterations'] / c['solve_s'] / c['items']:.0f} it/s per item", ""]
    if s:
        out += [f"(s) one launch of items that never solve ({s['n_vars']} variables / {s['n_clauses']} clauses, 3-SAT):",
                "    items  slice   launch ms (3 runs)            us per iteration (best)"]
        for row in s["rows"]:
            ms = "  ".join(f"{x:8.3f}" for x in row["launch_ms"])
            out.append(f"    {row['items']:5d}  {row['slice']:5d}   {ms}   {row['us_per_iteration']:8.2f}")
        out.append("")
    if g:
        out += ["(g) LFMIS choice: violated sets of at most `serial` clauses take the one-wave serial greedy, larger ones",
                "    the claim rounds; 256 seeds each, solve ms (best of 5; all 5):",
                "    serial   200/520 to the end (small sets)              200/800, 2000 iterations (sets of ~100)"]
        for x in g:
            cells = []
            for name in ("portfolio", "dense"):
                ms = x[name]["solve_ms"]
                cells.append(f"{min(ms):7.2f}  ({' '.join(f'{v:.2f}' for v in ms)})")
            out.append(f"    {x['serial_max']:6d}   {cells[0]:48s} {cells[1]}")
        out.append("")
    u = [r[k] for k in sorted(r) if k.startswith("u")]
    if u:
        out += ["(u) the batch of (a) alone on two builds, alternately (solve ms, best of 5; all 5; digest of the results):"]
        for x in u:
            out.append(f"    {os.path.basename(x['lib']):24s} {min(x['ms']):8.3f}  ({' '.join(f'{v:.3f}' for v in x['ms'])})  "
                       f"{x['iterations']} iterations  {x['digest']}")
        out.append("")
    t = r.get("t")
    if t:
        out += ["(t) per-variable thresholds, every item at thr = 2^31 (ms, best of 5; all 5):"]
        for x in t["rows"]:
            out.append(f"    {x['size']:10s} {x['items']:4d} items  {x['mode']:28s} {min(x['ms']):9.3f}  "
                       f"({' '.join(f'{v:.3f}' for v in x['ms'])})  {x['iterations']} iterations  {x['digest']}")
        out.append("")
    q = r.get("q")
    if q:
        out += [f"(q) cube portfolio: {q['cubes']} cubes of variables 0..7, {q['n_vars']} variables / {q['n_clauses']} clauses, "
                "create to first answer (ms, best of 3; all 3):"]
        for name in ("batch", "group"):
            x = q[name]
            out.append(f"    {name:6s} {min(x['ms']):9.2f}  ({' '.join(f'{v:.2f}' for v in x['ms'])})  {x['live']} live cubes, "
                       f"winner cube {x['winner']} after {x['winner_iterations']} iterations")
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["a", "b", "c", "s", "g", "u", "t", "q"],
                    help="run one leg in this process, print its JSON line")
    ap.add_argument("--ab-lib", help="leg u: another build's liballl.so to alternate with (three pairs, both orders)")
    ap.add_argument("--legs", default="abcsg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "summary.txt"))
    args = ap.parse_args()
    if args.leg:
        from alllsatisfiabilitysolver_amd import device_count

        if device_count() < 1:
            raise SystemExit("batch_bench: no HIP device visible (no fallback)")
        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "s": leg_s, "g": leg_g, "u": leg_u, "t": leg_t, "q": leg_q}
        print(json.dumps(legs[args.leg]()), flush=True)
        return 0
    results = {}
    env = {k: v for k, v in os.environ.items() if k != "ALLL_BATCH_SERIAL_MAX"}  # (the library's default)
    env.pop("ALLL_LIB_AB", None)
    runs = [(leg, leg, env) for leg in args.legs if leg not in "gu"]
    if "u" in args.legs:
        other = dict(env, ALLL_LIB_AB=os.path.abspath(args.ab_lib)) if args.ab_lib else None
        order = [other, env, env, other, other, env] if other else [env]
        runs += [("u", f"u{i}", e) for i, e in enumerate(order)]
    if "g" in args.legs:
        runs += [("g", f"g{i}", dict(env, ALLL_BATCH_SERIAL_MAX=str(sm))) for i, sm in enumerate(SERIAL_MAX)]
    for leg, key, e in runs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True,
                               text=True, timeout=LEG_TIMEOUT[leg], env=e)
        except subprocess.TimeoutExpired:
            print(f"leg {leg}: time limit {LEG_TIMEOUT[leg]} s; nothing more is started", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"leg {leg}: exit {p.returncode}; nothing more is started\n{p.stdout}\n{p.stderr}", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        results[key] = json.loads(p.stdout.strip().splitlines()[-1])
        print(p.stdout.strip().splitlines()[-1], flush=True)
    text = summary(results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    a = results.get("a")
    return 1 if a and a["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
