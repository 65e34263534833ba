#!/usr/bin/env python3
"""Measures failed-literal probing on the MI355X; every leg prints one JSON line
(profiles/probe/summary.txt keeps them):

  --leg m   bench.py's config M (random 3-SAT, 2.5 M variables / 10 M clauses) under a cube of random
            pins, propagated (the largest of 20,000 / 10,000 / 5,000 / 2,000 pins that reaches a
            fixpoint): both literals of the --probes / 2 free variables with the largest T, through
            Solver.probe without rows, host wall clock around every call, and the rounds the probes
            make.  Under `rocprofv3 --kernel-trace --stats` the leg gives the device times of
            k_probe_scan / judge / apply / settle per round.
  --leg s   the same probes, the first --singles of them, one at a time the way a caller had to before:
            set_thresholds(base with the probe's pin) and propagate_pins on the same context; records
            equal to the probe call's are asserted.  Under rocprofv3 it gives k_prop_scan and
            k_prop_apply per round beside the probe kernels of leg m.
  --leg r   failed_literal_reduce, device against host path, wall clock: on B-fail (2003 variables /
            8000 clauses under 170 pins) and on generate_ksat(11, 20003, 80000, 3) under 1000 pins,
            an instance above the batch size.

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


def config_m(s_cls, generate_ksat):
    """The context of config M under a propagated cube -> (solver, base thresholds, facts)."""
    n, m = 2_500_000, 10_000_000
    offs, lits = generate_ksat(1, n, m, 3, 0)
    s = s_cls(n, offs, lits, seed=1)
    for pins in (20000, 10000, 5000, 2000):
        s.set_thresholds(cube(n, pins, 0))
        res = s.propagate_pins()
        if res["status"] == 0:
            break
    else:
        raise SystemExit("no cube propagates to a fixpoint")
    return s, s.thresholds(), {"n_vars": n, "n_clauses": m, "pins": pins, "base": res}


def candidates(s, n_probes):
    S, _ = s.var_scores()
    T = S[0::2].astype(np.int64) + S[1::2].astype(np.int64)
    vs = np.argsort(-T, kind="stable")[:n_probes // 2]
    return np.stack([2 * vs, 2 * vs + 1], 1).astype(np.uint32).ravel()


def summary(res):
    status = {}
    for r in res:
        status[r["status"]] = status.get(r["status"], 0) + 1
    return {"status": status, "max_rounds": max(r["rounds"] for r in res), "sum_rounds": sum(r["rounds"] for r in res),
            "max_forced": max(r["n_forced"] for r in res)}


def leg_m(n_probes, reps):
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    s, _, out = config_m(Solver, generate_ksat)
    with s:
        probes = candidates(s, n_probes)
        first = s.probe(probes)  # warm-up: code objects
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = s.probe(probes)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert res == first
        out.update(leg="m", probes=int(probes.size),
                   slabs_env=os.environ.get("ALLL_PROBE_SLABS", ""), calls=reps + 1, **summary(first),
                   probe_ms={"median": statistics.median(ms), "min": min(ms), "max": max(ms)})
    return out


def leg_s(n_probes, singles):
    from alllsatisfiabilitysolver_amd import Solver, generate_ksat

    s, base, out = config_m(Solver, generate_ksat)
    with s:
        probes = candidates(s, n_probes)[:singles]
        want = s.probe(probes)
        ms, got = [], []
        for l in probes.tolist():
            thr = base.copy()
            thr[l >> 1] = 0 if l & 1 else PIN1
            s.set_thresholds(thr)
            t0 = time.perf_counter()
            got.append(s.propagate_pins())
            ms.append((time.perf_counter() - t0) * 1e3)
        assert got == want, (got, want)
        out.update(leg="s", singles=int(probes.size), **summary(want), scans=sum(r["rounds"] + 1 for r in want),
                   propagate_pins_ms={"median": statistics.median(ms), "min": min(ms), "max": max(ms), "sum": sum(ms)})
    return out


def leg_r():
    from alllsatisfiabilitysolver_amd import failed_literal_reduce, generate_ksat

    out = {"leg": "r"}
    for name, (n, m, seed, pins, cs) in {"B_fail": (2003, 8000, 5, 170, 4), "A4": (20003, 80000, 11, 1000, 0)}.items():
        offs, lits = generate_ksat(seed, n, m, 3)
        thr = cube(n, pins, cs)
        failed_literal_reduce(n, offs, lits, thr, device=True, max_passes=1)  # warm-up: code objects
        t = {}
        for device in (True, False):
            t0 = time.perf_counter()
            r = failed_literal_reduce(n, offs, lits, thr, device=device)
            t["device_ms" if device else "host_ms"] = (time.perf_counter() - t0) * 1e3
            t["device" if device else "host"] = {k: r[k] for k in ("status", "passes", "n_failed", "n_necessary",
                                                                    "lookahead_var")}
        assert t["device"] == t["host"]
        out[name] = t
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["m", "s", "r"])
    ap.add_argument("--probes", type=int, default=64)
    ap.add_argument("--singles", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(leg_r() if a.leg == "r" else leg_m(a.probes, a.reps) if a.leg == "m" else leg_s(a.probes, a.singles)))
