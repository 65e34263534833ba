"""Host-side Python front-end of the MI355X solver (over the C-ABI, liballl.so).

Two layers:
  * `Solver` -- a thin owner of one `alll_ctx` with numpy in/out (tests, bench, CLI).
  * `SATInstance` / `VariablesArray` / `Clause` / `Statistics` -- the reference's API shape
    (library/include/SATInstance.h:25-66, :156-173; VariablesArray.h:17-35; Clause.h:17-28)
    for Python callers.  C++ callers use include/alll_compat/SATInstance.h instead.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N

_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


def _p(a, t):
    return a.ctypes.data_as(t)


# ------------------------------------------------------------------ instance helpers
def generate_ksat(gen_seed: int, n_vars: int, n_clauses: int, k: int, kind: int = 0,
                  c_begin: int = 0, c_end: Optional[int] = None):
    """Random k-SAT, k distinct variables per clause (kind 0 uniform, 1 power-law).
    Returns (offsets uint64[m+1], literals uint32[m*k]) for clauses [c_begin, c_end)."""
    c_end = n_clauses if c_end is None else c_end
    lits = np.empty((c_end - c_begin) * k, np.uint32)
    N.check(N.lib().alll_generate_ksat(gen_seed, n_vars, n_clauses, k, kind, c_begin, c_end,
                                       _p(lits, _u32p)), "generate_ksat")
    offs = np.arange(c_end - c_begin + 1, dtype=np.uint64) * np.uint64(k)
    return offs, lits


def generate_mixed(gen_seed: int, n_vars: int, n_clauses: int, w_min: int, w_max: int):
    """Random clauses of mixed widths (uniform in [w_min, w_max]), variables and signs uniform
    (a variable may repeat inside a clause, as DIMACS allows).  Returns (offsets uint64[m+1],
    literals uint32[L]); deterministic for a seed (numpy PCG64)."""
    rng = np.random.default_rng(gen_seed)
    w = rng.integers(w_min, w_max + 1, n_clauses, dtype=np.int64)
    offs = np.zeros(n_clauses + 1, np.uint64)
    np.cumsum(w, out=offs[1:])
    L = int(offs[-1])
    v = rng.integers(0, n_vars, L, dtype=np.uint32)
    sgn = rng.integers(0, 2, L, dtype=np.uint32)
    return offs, (v << np.uint32(1)) | sgn


def assignment_digest(words) -> str:
    """64-bit FNV-1a over the bit-packed assignment's uint32 words (one xor-multiply step per
    word), as 16 hex digits: the trajectory digest of tests/golden/bench_trajectory.json."""
    h = 0xCBF29CE484222325
    for w in np.ascontiguousarray(words, np.uint32).tolist():
        h = ((h ^ w) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def parse_dimacs(text: bytes):
    """DIMACS text -> (n_vars, offsets, literals) with the reference loader semantics."""
    L = N.lib()
    v, c, ln = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.alll_dimacs_parse(text, len(text), ctypes.byref(v), ctypes.byref(c), None, None,
                             ctypes.byref(ln))
    if rc == N.ALLL_ERR_BAD_INPUT:
        N.check(rc, "dimacs")
    offs = np.zeros(c.value + 1, np.uint64)
    lits = np.zeros(max(1, ln.value), np.uint32)
    N.check(L.alll_dimacs_parse(text, len(text), ctypes.byref(v), ctypes.byref(c), _p(offs, _u64p),
                                _p(lits, _u32p), ctypes.byref(ln)), "dimacs")
    return int(v.value), offs, lits[: ln.value]


def read_dimacs(path: str):
    L = N.lib()
    v, c, ln = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    bp = os.fsencode(path)
    rc = L.alll_dimacs_read(bp, ctypes.byref(v), ctypes.byref(c), None, None, ctypes.byref(ln))
    if rc in (N.ALLL_ERR_BAD_INPUT, N.ALLL_ERR_IO):
        N.check(rc, f"dimacs {path}")
    offs = np.zeros(c.value + 1, np.uint64)
    lits = np.zeros(max(1, ln.value), np.uint32)
    N.check(L.alll_dimacs_read(bp, ctypes.byref(v), ctypes.byref(c), _p(offs, _u64p),
                               _p(lits, _u32p), ctypes.byref(ln)), f"dimacs {path}")
    return int(v.value), offs, lits[: ln.value]


# ------------------------------------------------ per-variable probabilities (alll.h)
def var_thresholds(p) -> np.ndarray:
    """Probabilities P(x_v = 1) -> the uint32 thresholds of Solver.set_thresholds
    (alll_var_threshold per entry: 0 -> 0 and 1 -> 0xFFFFFFFF pin the variable)."""
    p = np.atleast_1d(np.asarray(p, np.float64))
    vals, inv = np.unique(p, return_inverse=True)  # (one call per distinct probability)
    thr = np.zeros(vals.size, np.uint32)
    L, t = N.lib(), ctypes.c_uint32()
    for i, x in enumerate(vals.tolist()):
        N.check(L.alll_var_threshold(x, ctypes.byref(t)), f"var_thresholds({x})")
        thr[i] = t.value
    return thr[inv].reshape(p.shape)


def biased_initial_assignment(seed: int, n_vars: int, thr) -> np.ndarray:
    """The biased initial fill for `seed` under thresholds thr, as n_vars bytes of 0/1 (host-only)."""
    thr = np.ascontiguousarray(thr, np.uint32)
    if thr.size != n_vars:
        raise ValueError(f"{thr.size} thresholds for {n_vars} variables")
    out = np.zeros(max(1, n_vars), np.uint8)
    N.check(N.lib().alll_biased_initial_assignment(seed, n_vars, _p(thr, _u32p), _p(out, _u8p)),
            "biased_initial_assignment")
    return out[:n_vars]


def pinned_conflict(n_vars: int, offsets, literals, thr) -> Optional[int]:
    """alll_pinned_conflict: the first clause whose literals are all pinned false by thresholds thr
    (an empty clause counts), or None when every clause can still be met (host-only)."""
    offs = np.ascontiguousarray(offsets, np.uint64)
    lits = np.ascontiguousarray(literals, np.uint32)
    thr = np.ascontiguousarray(thr, np.uint32)
    m = max(0, offs.size - 1)
    prob = N.Problem(int(n_vars), 0, m, _p(offs, _u64p), _p(lits, _u32p))
    c = ctypes.c_uint64()
    N.check(N.lib().alll_pinned_conflict(ctypes.byref(prob), _p(thr, _u32p), thr.size, ctypes.byref(c)),
            "pinned_conflict")
    return None if c.value == m else int(c.value)


def propagate_pins(n_vars: int, offsets, literals, thr, max_rounds: int = 0):
    """alll_pinned_propagate: unit propagation of the pins of thresholds thr (host-only; the rounds of
    include/alll.h).  Returns (propagated thresholds, {"status", "rounds", "n_forced",
    "conflict_clause"}); status is one of PROP_FIXPOINT / PROP_CONFLICT / PROP_ROUND_CAP, conflict_clause
    the number of clauses when there is none.  thr itself is left alone."""
    offs = np.ascontiguousarray(offsets, np.uint64)
    lits = np.ascontiguousarray(literals, np.uint32)
    out = np.array(thr, np.uint32)  # (a copy: the library propagates in place)
    m = max(0, offs.size - 1)
    prob = N.Problem(int(n_vars), 0, m, _p(offs, _u64p), _p(lits, _u32p))
    res = N.PropagateResult()
    N.check(N.lib().alll_pinned_propagate(ctypes.byref(prob), _p(out, _u32p), out.size, max_rounds, ctypes.byref(res)),
            "pinned_propagate")
    return out, res.as_dict()


def var_scores(n_vars: int, offsets, literals, thr=None):
    """alll_pinned_scores: the split scores under thresholds thr (host-only; None: every variable
    free).  Returns (scores uint64[2 * n_vars], {"var", "score_pos", "score_neg", "n_open"}): scores[l]
    is S[l] of include/alll.h, var the free variable with the largest S[2v] + S[2v+1] (the lowest on a
    tie), n_vars when no open clause holds a free literal."""
    offs = np.ascontiguousarray(offsets, np.uint64)
    lits = np.ascontiguousarray(literals, np.uint32)
    m = max(0, offs.size - 1)
    prob = N.Problem(int(n_vars), 0, m, _p(offs, _u64p), _p(lits, _u32p))
    scores = np.zeros(2 * int(n_vars), np.uint64)
    res = N.SplitResult()
    if thr is None:
        t, n = None, 0
    else:
        thr = np.ascontiguousarray(thr, np.uint32)
        t, n = _p(thr, _u32p), thr.size
    N.check(N.lib().alll_pinned_scores(ctypes.byref(prob), t, n, _p(scores, _u64p), ctypes.byref(res)), "pinned_scores")
    return scores, res.as_dict()


def _probe_out(n_probes: int, n_vars: int, rows: bool):
    """The result records of a probe call and, with rows, its two arrays of n_probes x n_words words."""
    res = (N.PropagateResult * max(1, n_probes))()
    nw = (int(n_vars) + 31) // 32
    pm = np.zeros((n_probes, nw), np.uint32) if rows else None
    pv = np.zeros((n_probes, nw), np.uint32) if rows else None
    return res, nw, pm, pv


def _probe_ret(res, n_probes: int, rows: bool, pm, pv):
    out = [res[i].as_dict() for i in range(n_probes)]
    return (out, pm, pv) if rows else out


def probe_literals(n_vars: int, offsets, literals, thr, probes, max_rounds: int = 0, rows: bool = False):
    """alll_pinned_probe: failed-literal probing (host-only; include/alll.h).  Every probe is a literal
    l = 2v + sign; its result is what propagate_pins returns under thr (None: every variable a fair
    coin) with l pinned true -- a probe on a variable thr already pins: PROP_NONE.  Returns the list of
    {"status", "rounds", "n_forced", "conflict_clause"}; rows=True: (list, pm, pv), uint32[n_probes,
    n_words] each: the pinned variables when the probe ends and their values, bit-packed."""
    offs = np.ascontiguousarray(offsets, np.uint64)
    lits = np.ascontiguousarray(literals, np.uint32)
    probes = np.ascontiguousarray(probes, np.uint32).ravel()
    m = max(0, offs.size - 1)
    prob = N.Problem(int(n_vars), 0, m, _p(offs, _u64p), _p(lits, _u32p))
    if thr is None:
        t, n = None, 0
    else:
        thr = np.ascontiguousarray(thr, np.uint32)
        t, n = _p(thr, _u32p), thr.size
    res, _, pm, pv = _probe_out(probes.size, n_vars, rows)
    N.check(N.lib().alll_pinned_probe(ctypes.byref(prob), t, n, _p(probes, _u32p), probes.size, max_rounds, res,
                                      _p(pm, _u32p) if rows else None, _p(pv, _u32p) if rows else None), "pinned_probe")
    return _probe_ret(res, probes.size, rows, pm, pv)


class _ResidualArrays:
    """The output arrays of a residual call at their capacities (sums of the items' original sizes),
    and their cut into one dict per item."""

    def __init__(self, sizes, with_arrays: bool):
        # sizes: per item (n_vars, n_clauses, n_literals)
        self.on = with_arrays
        if not with_arrays:  # (the counts alone: nothing to hold)
            return
        nv, m, nl = (sum(s[k] for s in sizes) for k in range(3))
        self.offsets = np.zeros(m + len(sizes), np.uint64)
        self.literals = np.zeros(max(1, nl), np.uint32)
        self.var_map = np.zeros(max(1, nv), np.uint32)
        self.clause_map = np.zeros(max(1, m), np.uint64)
        self.thr = np.zeros(max(1, nv), np.uint32)

    def args(self):
        if not self.on:
            return (None,) * 5
        return (_p(self.offsets, _u64p), _p(self.literals, _u32p), _p(self.var_map, _u32p), _p(self.clause_map, _u64p),
                _p(self.thr, _u32p))

    def items(self, records) -> List[dict]:
        out, c0, l0, v0 = [], 0, 0, 0
        for i, r in enumerate(records):
            d = {"n_vars": r["n_vars"], "n_clauses": r["n_clauses"], "n_literals": r["n_literals"],
                 "n_falsified": r["n_falsified"], "first_falsified": r["first_falsified"]}
            if self.on:
                c1, l1, v1 = c0 + r["n_clauses"], l0 + r["n_literals"], v0 + r["n_vars"]
                d.update(offsets=self.offsets[c0 + i:c1 + i + 1].copy(), literals=self.literals[l0:l1].copy(),
                         var_map=self.var_map[v0:v1].copy(), clause_map=self.clause_map[c0:c1].copy(),
                         thr=self.thr[v0:v1].copy())
                c0, l0, v0 = c1, l1, v1
            out.append(d)
        return out


def residual_instance(n_vars: int, offsets, literals, thr=None) -> dict:
    """alll_pinned_residual: the residual formula under thresholds thr (host-only; None: every
    variable free): the clauses without a true literal, reduced to their free literals, over the
    variables that still occur, renumbered in ascending order (include/alll.h).  Returns {"n_vars",
    "n_clauses", "n_literals", "offsets", "literals", "var_map", "clause_map", "thr", "n_falsified",
    "first_falsified"}: (n_vars, offsets, literals) is the residual problem, thr its thresholds,
    var_map / clause_map the original variable / clause of every residual one."""
    offs = np.ascontiguousarray(offsets, np.uint64)
    lits = np.ascontiguousarray(literals, np.uint32)
    m = max(0, offs.size - 1)
    prob = N.Problem(int(n_vars), 0, m, _p(offs, _u64p), _p(lits, _u32p))
    if thr is None:
        t, n = None, 0
    else:
        thr = np.ascontiguousarray(thr, np.uint32)
        t, n = _p(thr, _u32p), thr.size
    # (the capacities: the literal count is offsets[m] once the call has validated the instance)
    out = _ResidualArrays([(int(n_vars), m, lits.size)], True)
    res = N.ResidualResult()
    N.check(N.lib().alll_pinned_residual(ctypes.byref(prob), t, n, ctypes.byref(res), *out.args()), "pinned_residual")
    return out.items([res.as_dict()])[0]


def lift_assignment(n_vars: int, thr, var_map, words_res) -> np.ndarray:
    """The full assignment of a residual one (bit-packed, ceil(n_vars / 32) words): the pinned
    variables of thr (None: none) at their pins, the kept variables var_map[u] at bit u of words_res,
    every other variable 0."""
    bits = np.zeros(32 * ((int(n_vars) + 31) // 32), np.uint8)
    if thr is not None:
        bits[:n_vars][np.asarray(thr, np.uint32) == 0xFFFFFFFF] = 1
    var_map = np.asarray(var_map, np.int64)
    res = np.unpackbits(np.ascontiguousarray(words_res, np.uint32).view(np.uint8), bitorder="little")
    if res.size < var_map.size:
        raise ValueError(f"{res.size} residual bits for {var_map.size} kept variables")
    bits[var_map] = res[:var_map.size]
    return np.packbits(bits, bitorder="little").view(np.uint32)


# ----------------------------------------------------------------------------- Solver
class Solver:
    """Owns one device solver context (alll_ctx).  probabilities: P(x_v = 1) per variable (0 and 1
    pin the variable; set_probabilities), None = fair coins, the unbiased stream.  track_best: keep
    the best assignment the loop evaluates (track_best, best)."""

    def __init__(self, n_vars: int, offsets, literals, seed: int = 1, max_iters: int = 0,
                 device: int = -1, n_threads: int = 1, rank: int = 0, world: int = 1,
                 comm_id: Optional[bytes] = None, flags: int = 0, grid_rounds: int = 0,
                 exchange=None, stream_batch: int = 0, set_starts=None, probabilities=None,
                 track_best: bool = False):
        self._L = N.lib()
        self.n_vars = int(n_vars)
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        self.literals = np.ascontiguousarray(literals, np.uint32)
        self.m = self.offsets.size - 1
        prob = N.Problem(self.n_vars, 0, self.m, _p(self.offsets, _u64p), _p(self.literals, _u32p))
        opt = N.Options()
        self._L.alll_default_options(ctypes.byref(opt))
        opt.seed, opt.max_iters, opt.device = seed, max_iters, device
        opt.n_threads, opt.rank, opt.world = n_threads, rank, world
        opt.flags, opt.grid_rounds = flags, grid_rounds
        opt.stream_batch = stream_batch  # > 0: streaming solve semantics (alll.h)
        # n_threads > 1: round-robin MIS over n_threads chunks (alll.h); set_starts = the
        # n_threads + 1 chunk boundaries, None = the example/main.cpp chunking
        if set_starts is not None:
            self._set_starts = np.ascontiguousarray(set_starts, np.uint64)
            opt.set_starts = _p(self._set_starts, _u64p)
        if comm_id is not None:
            ctypes.memmove(opt.comm_id, comm_id, 128)
        self._ctx = ctypes.c_void_p()
        N.check(self._L.alll_create(ctypes.byref(prob), ctypes.byref(opt), ctypes.byref(self._ctx)),
                "alll_create")
        self.world = world
        self.rank = rank
        self._xfn = None
        if exchange is not None:
            self.set_host_exchange(exchange)
        try:
            if probabilities is not None:
                self.set_probabilities(probabilities)
            if track_best:
                self.track_best()
        except Exception:
            self.close()
            raise

    def track_best(self, on: bool = True):
        """alll_track_best: keep (or stop keeping) the best assignment the loop's eval passes see.
        Before the first iteration only (alll.h)."""
        N.check(self._L.alll_track_best(self._ctx, 1 if on else 0), "alll_track_best")

    def best(self) -> dict:
        """alll_get_best: {"n_violated", "iteration", "words"} of the first eval pass with the fewest
        violated clauses: the assignment it evaluated, bit-packed.  Before any pass: n_violated
        2^64 - 1, iteration 0, words all zero."""
        nv, it = ctypes.c_uint64(), ctypes.c_uint64()
        w = np.zeros((self.n_vars + 31) // 32, np.uint32)
        N.check(self._L.alll_get_best(self._ctx, ctypes.byref(nv), ctypes.byref(it), _p(w, _u32p), w.size),
                "alll_get_best")
        return {"n_violated": int(nv.value), "iteration": int(it.value), "words": w}

    def set_probabilities(self, p):
        """P(x_v = 1) per variable (n_vars entries; 0 and 1 pin the variable), or None for the
        unbiased stream.  Before the first iteration only; rewrites the assignment (alll.h)."""
        self.set_thresholds(None if p is None else var_thresholds(p))

    def set_thresholds(self, thr):
        """alll_set_var_thresholds: n_vars uint32 thresholds (var_thresholds), or None."""
        if thr is None:
            N.check(self._L.alll_set_var_thresholds(self._ctx, None, 0), "set_var_thresholds")
            return
        thr = np.ascontiguousarray(thr, np.uint32)
        N.check(self._L.alll_set_var_thresholds(self._ctx, _p(thr, _u32p), thr.size), "set_var_thresholds")

    def propagate_pins(self, max_rounds: int = 0) -> dict:
        """alll_propagate_pins: unit propagation of the pinned variables on the device (max_rounds 0:
        to the fixpoint or the conflict).  Before the first iteration, on a solver that has
        thresholds; afterwards the solver is one given thresholds() from the start.  Returns
        {"status", "rounds", "n_forced", "conflict_clause"} (propagate_pins, the host form)."""
        res = N.PropagateResult()
        N.check(self._L.alll_propagate_pins(self._ctx, max_rounds, ctypes.byref(res)), "alll_propagate_pins")
        return res.as_dict()

    def thresholds(self) -> np.ndarray:
        """alll_get_var_thresholds: the solver's n_vars thresholds (the propagated ones after
        propagate_pins)."""
        thr = np.zeros(self.n_vars, np.uint32)
        N.check(self._L.alll_get_var_thresholds(self._ctx, _p(thr, _u32p), thr.size), "alll_get_var_thresholds")
        return thr

    def var_scores(self, with_scores: bool = True):
        """alll_var_scores: the split scores under the solver's current thresholds (none: every
        variable free), computed on the device.  At any time; nothing of the solver changes.  Returns
        (scores, split) as var_scores, the host form; with_scores=False: the split record alone."""
        res = N.SplitResult()
        if not with_scores:
            N.check(self._L.alll_var_scores(self._ctx, None, 0, ctypes.byref(res)), "alll_var_scores")
            return res.as_dict()
        scores = np.zeros(2 * self.n_vars, np.uint64)
        N.check(self._L.alll_var_scores(self._ctx, _p(scores, _u64p), scores.size, ctypes.byref(res)), "alll_var_scores")
        return scores, res.as_dict()

    def probe(self, probes, max_rounds: int = 0, rows: bool = False):
        """alll_probe_literals: failed-literal probing under the solver's current thresholds (none:
        every variable free) on the device, 64 probes per pass over the clauses.  At any time; nothing
        of the solver changes.  Returns what probe_literals, the host form, returns."""
        probes = np.ascontiguousarray(probes, np.uint32).ravel()
        res, nw, pm, pv = _probe_out(probes.size, self.n_vars, rows)
        N.check(self._L.alll_probe_literals(self._ctx, _p(probes, _u32p), probes.size, max_rounds, res,
                                            _p(pm, _u32p) if rows else None, _p(pv, _u32p) if rows else None, nw),
                "alll_probe_literals")
        return _probe_ret(res, probes.size, rows, pm, pv)

    def residual(self, with_arrays: bool = True) -> dict:
        """alll_residual: the residual formula under the solver's current thresholds (none: every
        variable free), compacted on the device.  At any time; nothing of the solver changes.  Returns
        the dict of residual_instance, the host form; with_arrays=False: the counts alone."""
        out = _ResidualArrays([(self.n_vars, self.m, self.literals.size)], with_arrays)
        res = N.ResidualResult()
        N.check(self._L.alll_residual(self._ctx, ctypes.byref(res), *out.args()), "alll_residual")
        return out.items([res.as_dict()])[0]

    def set_host_exchange(self, exchange):
        """exchange(op, buf: numpy uint8 view, bytes_per_rank_or_total) -> None; see
        include/alll.h (ALLL_XCHG_*).  Used instead of RCCL (e.g. several ranks on one GPU)."""
        world = self.world

        def fn(user, op, buf, nbytes):
            try:
                total = nbytes * world if op == N.XCHG_ALLGATHER else nbytes
                arr = np.ctypeslib.as_array((ctypes.c_uint8 * total).from_address(buf))
                exchange(op, arr, nbytes)
                return 0
            except Exception:  # reported as ALLL_ERR_RCCL by the library
                import traceback

                traceback.print_exc()
                return 1

        self._xfn = N.EXCHANGE_FN(fn)
        N.check(self._L.alll_set_host_exchange(self._ctx, self._xfn, None), "set_host_exchange")

    # lifecycle
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.alll_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # loop
    def solve(self) -> dict:
        st = N.Stats()
        rc = self._L.alll_solve(self._ctx, ctypes.byref(st))
        if rc not in (N.ALLL_OK, N.ALLL_ERR_MAX_ITERS):
            N.check(rc, "alll_solve")
        return st.as_dict()

    def run(self, n_iters: int, sync: bool = True) -> Optional[dict]:
        if sync:
            st = N.Stats()
            N.check(self._L.alll_run(self._ctx, n_iters, ctypes.byref(st)), "alll_run")
            return st.as_dict()
        N.check(self._L.alll_run(self._ctx, n_iters, None), "alll_run")
        return None

    def synchronize(self):
        N.check(self._L.alll_synchronize(self._ctx), "alll_synchronize")

    def stats(self) -> dict:
        st = N.Stats()
        N.check(self._L.alll_get_stats(self._ctx, ctypes.byref(st)), "alll_get_stats")
        return st.as_dict()

    def verify(self):
        ok = ctypes.c_int()
        nv = ctypes.c_uint64()
        N.check(self._L.alll_verify(self._ctx, ctypes.byref(ok), ctypes.byref(nv)), "alll_verify")
        return bool(ok.value), int(nv.value)

    # state access
    def assignment_words(self) -> np.ndarray:
        w = np.zeros((self.n_vars + 31) // 32, np.uint32)
        N.check(self._L.alll_get_assignment_words(self._ctx, _p(w, _u32p), w.size), "get_assignment")
        return w

    def set_assignment_words(self, w):
        w = np.ascontiguousarray(w, np.uint32)
        N.check(self._L.alll_set_assignment_words(self._ctx, _p(w, _u32p), w.size), "set_assignment")

    def assignment(self) -> np.ndarray:
        a = np.zeros(max(1, self.n_vars), np.uint8)
        N.check(self._L.alll_get_assignment(self._ctx, _p(a, _u8p), a.size), "get_assignment")
        return a[: self.n_vars]

    def set_assignment(self, a):
        a = np.ascontiguousarray(a, np.uint8)
        N.check(self._L.alll_set_assignment(self._ctx, _p(a, _u8p), a.size), "set_assignment")

    def violated_mask(self) -> np.ndarray:
        w = np.zeros(max(1, (self.m + 63) // 64), np.uint64)
        N.check(self._L.alll_get_violated_mask(self._ctx, _p(w, _u64p), w.size), "violated_mask")
        return w

    def mis(self) -> np.ndarray:
        n = ctypes.c_uint64()
        N.check(self._L.alll_get_mis(self._ctx, None, 0, ctypes.byref(n)), "get_mis")
        out = np.zeros(max(1, n.value), np.uint32)
        N.check(self._L.alll_get_mis(self._ctx, _p(out, _u32p), out.size, ctypes.byref(n)), "get_mis")
        return out[: n.value]

    # measurement
    def bench_eval(self, reps: int = 20):
        ms = ctypes.c_double()
        nv = ctypes.c_uint64()
        N.check(self._L.alll_bench_eval(self._ctx, reps, ctypes.byref(ms), ctypes.byref(nv)), "bench_eval")
        return float(ms.value), int(nv.value)

    def profile(self, n_iters: int) -> dict:
        pt = N.PhaseTimes()
        N.check(self._L.alll_profile(self._ctx, n_iters, ctypes.byref(pt)), "profile")
        return pt.as_dict()

    def loop_times(self, first_iter: int, n_iters: int) -> dict:
        """In-loop phase times of iterations [first_iter, first_iter+n_iters) from the kernels'
        own wall-clock stamps (needs flags |= FLAG_KERNEL_TIMING)."""
        pt = N.PhaseTimes()
        N.check(self._L.alll_loop_times(self._ctx, first_iter, n_iters, ctypes.byref(pt)), "loop_times")
        return pt.as_dict()

    def eval_bytes(self) -> int:
        return int(self._L.alll_eval_bytes(self._ctx))

    def layout(self) -> int:
        return int(self._L.alll_layout(self._ctx))

    def eval_kernel(self) -> str:
        return self._L.alll_eval_kernel(self._ctx).decode()

    def uses_graphs(self):
        """(True, "") when the loop replays captured hipGraphs; (False, reason) when it launches
        eagerly (ALLL_FLAG_NO_GRAPH, a host-staged exchange, or a failed capture)."""
        why = ctypes.c_char_p()
        r = int(self._L.alll_uses_graphs(self._ctx, ctypes.byref(why)))
        return r == 1, (why.value or b"").decode()

    def rr_pass_log(self):
        """Round robin: per pass of the last iteration (dirty entries, repair rounds, entries
        decided, decisions changed) of its incremental passes (measurement)."""
        return self._rr_log()[0]

    def rr_round_log(self):
        """Round robin: per pass of the last iteration, the repair's clock stamps (100 MHz;
        detect, wide repair, repair, rounds end, repair end, LDS loaded) and its rounds
        {entries, stamp}, then a row of k_fp_bbuild's phase stamps (measurement, written only
        with FLAG_KERNEL_TIMING; rows of 64 words, zeros where not reached)."""
        return self._rr_log()[1]

    def _rr_log(self):
        out = np.zeros(256 + 64 * 65, np.uint32)
        n = self._L.alll_rr_pass_log(self._ctx, _p(out, _u32p), out.size)
        if n < 0:
            N.check(n, "rr_pass_log")
        return out[:min(n, 256)].reshape(-1, 4), out[256:max(n, 256)].reshape(-1, 64)

    def rr_barrier_timeouts(self) -> int:
        """Round robin: wide-repair grid barriers that timed out since create (measurement)."""
        n = int(self._L.alll_rr_barrier_timeouts(self._ctx))
        if n < 0:
            raise N.AlllError(N.ALLL_ERR_HIP, "alll_rr_barrier_timeouts failed")
        return n

    def epoch_counters(self) -> dict:
        """Owner-epoch counters since create (test support): round-robin iterations that started
        their epochs over and those left to the batch kernel for want of epochs, restarts of the
        one-set loop's 32-bit epochs, and that loop's first unused epoch."""
        out = np.zeros(4, np.uint64)
        N.check(self._L.alll_epoch_counters(self._ctx, _p(out, _u64p)), "epoch_counters")
        return dict(zip(("rr_restarts", "rr_fails", "restarts", "round_next"), (int(x) for x in out)))

    def comm_size(self) -> int:
        """Ranks in the solve: the RCCL communicator's count (or world with a host exchange)."""
        n = int(self._L.alll_comm_size(self._ctx))
        if n < 1:
            raise N.AlllError(N.ALLL_ERR_RCCL, "ncclCommCount failed")
        return n


def device_count() -> int:
    return int(N.lib().alll_device_count())


# ------------------------------------------------------------------------ BatchSolver
def batch_fits(n_vars: int, n_clauses: int, n_literals: int) -> bool:
    """True when an instance of this size can be an item of a BatchSolver (host-only)."""
    return bool(N.lib().alll_batch_fits(n_vars, n_clauses, n_literals))


class _ItemSolver:
    """What BatchSolver and GroupSolver share: item i is problems[i] = (n_vars, offsets, literals)
    with seeds[i]; the entry points are alll_<_KIND>_*, the handle is self._h."""

    _KIND = ""          # "batch" or "group"
    _FIRST_SOLVED = 0   # the kind's ALLL_*_FIRST_SOLVED

    def _fn(self, name: str):
        return getattr(self._L, f"alll_{self._KIND}_{name}")

    def __init__(self, problems, seeds, max_iters: int, device: int, flags: Optional[int]):
        self._L = N.lib()
        problems = list(problems)
        self._seeds = np.ascontiguousarray(seeds, np.uint64)
        if self._seeds.size != len(problems):
            raise ValueError(f"{len(problems)} problems, {self._seeds.size} seeds")
        self.n_items = len(problems)
        keep = {}  # one converted copy per distinct pair of arrays: shared problems stay shared
        arr = (N.Problem * max(1, self.n_items))()
        self.n_vars = []
        self._sizes = []  # per item (n_vars, n_clauses, n_literals)
        for i, (n_vars, offsets, literals) in enumerate(problems):
            key = (id(offsets), id(literals))
            if key not in keep:
                keep[key] = (offsets, literals, np.ascontiguousarray(offsets, np.uint64),
                             np.ascontiguousarray(literals, np.uint32))
            _, _, offs, lits = keep[key]
            arr[i] = N.Problem(int(n_vars), 0, max(0, offs.size - 1), _p(offs, _u64p), _p(lits, _u32p))
            self.n_vars.append(int(n_vars))
            self._sizes.append((int(n_vars), max(0, offs.size - 1), int(offs[-1]) if offs.size else 0))
        opt = N.Options()
        self._L.alll_default_options(ctypes.byref(opt))
        opt.max_iters, opt.device = max_iters, device
        if flags is not None:  # (None: the default options' flags)
            opt.flags = flags
        self._h = ctypes.c_void_p()
        N.check(self._fn("create")(arr, _p(self._seeds, _u64p), self.n_items, ctypes.byref(opt), ctypes.byref(self._h)),
                f"alll_{self._KIND}_create")
        # (the library keeps no caller pointer)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def solve(self, first_solved: bool = False) -> List[dict]:
        st = (N.Stats * self.n_items)()
        status = (ctypes.c_int32 * self.n_items)()
        N.check(self._fn("solve")(self._h, self._FIRST_SOLVED if first_solved else 0, st, status),
                f"alll_{self._KIND}_solve")
        return [dict(st[i].as_dict(), status=int(status[i])) for i in range(self.n_items)]

    def run(self, n_iters: int) -> List[dict]:
        """n_iters more full iterations of every unfinished item (Solver.run for each)."""
        st = (N.Stats * self.n_items)()
        N.check(self._fn("run")(self._h, n_iters, st), f"alll_{self._KIND}_run")
        return [st[i].as_dict() for i in range(self.n_items)]

    def stats(self, i: int) -> dict:
        st = N.Stats()
        N.check(self._fn("get_stats")(self._h, i, ctypes.byref(st)), f"alll_{self._KIND}_get_stats")
        return st.as_dict()

    def assignment_words(self, i: int) -> np.ndarray:
        w = np.zeros((self.n_vars[i] + 31) // 32, np.uint32)
        N.check(self._fn("get_assignment_words")(self._h, i, _p(w, _u32p), w.size), f"{self._KIND} get_assignment")
        return w

    def set_assignment_words(self, i: int, w):
        w = np.ascontiguousarray(w, np.uint32)
        N.check(self._fn("set_assignment_words")(self._h, i, _p(w, _u32p), w.size), f"{self._KIND} set_assignment")

    def set_probabilities(self, i: int, p):
        """Solver.set_probabilities for item i: it then computes what a Solver with seeds[i] and the
        same probabilities computes.  Items that are one instance under different pinned variables
        and solve(first_solved=True) make a cube portfolio (solve_cubes)."""
        self.set_thresholds(i, None if p is None else var_thresholds(p))

    def set_thresholds(self, i: int, thr):
        """alll_batch_set_var_thresholds / alll_group_set_var_thresholds: the item's n_vars uint32
        thresholds, or None."""
        if thr is None:
            N.check(self._fn("set_var_thresholds")(self._h, i, None, 0), f"{self._KIND} set_var_thresholds")
            return
        thr = np.ascontiguousarray(thr, np.uint32)
        N.check(self._fn("set_var_thresholds")(self._h, i, _p(thr, _u32p), thr.size), f"{self._KIND} set_var_thresholds")

    def propagate_pins(self, max_rounds: int = 0) -> List[dict]:
        """Solver.propagate_pins for every item that has thresholds, at once; one dict per item, an
        item without thresholds gets status PROP_NONE.  Before the first iteration only."""
        res = (N.PropagateResult * max(1, self.n_items))()
        N.check(self._fn("propagate_pins")(self._h, max_rounds, res), f"alll_{self._KIND}_propagate_pins")
        return [res[i].as_dict() for i in range(self.n_items)]

    def thresholds(self, i: int) -> np.ndarray:
        """Solver.thresholds of item i."""
        n = self.n_vars[i] if 0 <= i < self.n_items else 0  # (an item out of range: the library refuses it)
        thr = np.zeros(n, np.uint32)
        N.check(self._fn("get_var_thresholds")(self._h, i, _p(thr, _u32p), thr.size),
                f"alll_{self._KIND}_get_var_thresholds")
        return thr

    def track_best(self, on: bool = True):
        """Solver.track_best for every item at once; before the first iteration only."""
        N.check(self._fn("track_best")(self._h, 1 if on else 0), f"alll_{self._KIND}_track_best")

    def best(self, i: int) -> dict:
        """Solver.best of item i, in its own variable numbering and pass count.  The best of a
        portfolio that does not solve: min(range(n), key=lambda i: s.best(i)["n_violated"])."""
        nv, it = ctypes.c_uint64(), ctypes.c_uint64()
        n = self.n_vars[i] if 0 <= i < self.n_items else 0  # (an item out of range: the library refuses it)
        w = np.zeros((n + 31) // 32, np.uint32)
        N.check(self._fn("get_best")(self._h, i, ctypes.byref(nv), ctypes.byref(it), _p(w, _u32p), w.size),
                f"alll_{self._KIND}_get_best")
        return {"n_violated": int(nv.value), "iteration": int(it.value), "words": w}


class BatchSolver(_ItemSolver):
    """Owns one batch of LDS-resident instances (alll_batch): item i is problems[i] =
    (n_vars, offsets, literals) with seeds[i], solved by one workgroup; entries of `problems`
    may repeat the same arrays (many seeds of one instance), which the device then holds once.
    Every item computes exactly what Solver(n_vars, offsets, literals, seed=seeds[i],
    max_iters=max_iters) computes."""

    _KIND, _FIRST_SOLVED = "batch", N.BATCH_FIRST_SOLVED

    def __init__(self, problems, seeds, max_iters: int = 0, device: int = -1):
        super().__init__(problems, seeds, max_iters, device, None)

    def solve(self, first_solved: bool = False) -> List[dict]:
        """Runs every item until it is solved or capped; one dict per item: the statistics and
        "status" (ALLL_OK or ALLL_ERR_MAX_ITERS).  first_solved: return after the first slice
        in which an item became solved; a later call continues."""
        return super().solve(first_solved)

    def set_slice(self, n: int):
        """Iterations per kernel launch (0: the default)."""
        N.check(self._L.alll_batch_set_slice(self._h, n), "alll_batch_set_slice")


class GroupSolver(_ItemSolver):
    """Owns one block-diagonal group (alll_group): item i is problems[i] = (n_vars, offsets,
    literals) with seeds[i], of any size; the items are laid side by side as one instance and the
    one-instance loop advances all of them together.  Every item computes exactly what
    Solver(n_vars, offsets, literals, seed=seeds[i], max_iters=max_iters) computes.  flags: the
    FLAG_* that do not change results (NO_GRAPH, GENERIC_CSR, NO_RANGED, KERNEL_TIMING,
    ATOMIC_CLAIMS)."""

    _KIND, _FIRST_SOLVED = "group", N.GROUP_FIRST_SOLVED

    def __init__(self, problems, seeds, max_iters: int = 0, device: int = -1, flags: int = 0):
        super().__init__(problems, seeds, max_iters, device, flags)

    def solve(self, first_solved: bool = False) -> List[dict]:
        """Runs every item until it is solved or capped; one dict per item: the statistics and
        "status" (ALLL_OK or ALLL_ERR_MAX_ITERS).  first_solved: return once at least one item
        is solved (the winner: the solved item with the fewest iterations, the lowest index on a
        tie); a later call continues."""
        return super().solve(first_solved)

    def layout(self) -> int:
        """Layout of the union: 0 generic CSR, k > 0 fixed width k."""
        return int(self._L.alll_group_layout(self._h))

    def eval_kernel(self) -> str:
        return self._L.alll_group_eval_kernel(self._h).decode()

    def var_scores(self, with_scores: bool = False):
        """alll_group_var_scores: Solver.var_scores for every item in one pass over the union.  Returns
        the list of split records, one dict per item in its own variable numbering; with_scores=True:
        (that list, the list of the items' score arrays)."""
        res = (N.SplitResult * max(1, self.n_items))()
        if not with_scores:
            N.check(self._L.alll_group_var_scores(self._h, res, None, 0), "alll_group_var_scores")
            return [res[i].as_dict() for i in range(self.n_items)]
        scores = np.zeros(2 * sum(self.n_vars), np.uint64)
        N.check(self._L.alll_group_var_scores(self._h, res, _p(scores, _u64p), scores.size), "alll_group_var_scores")
        cuts = np.cumsum([2 * n for n in self.n_vars])[:-1]
        return [res[i].as_dict() for i in range(self.n_items)], np.split(scores, cuts)

    def probes(self, probes, max_rounds: int = 0, rows: bool = False) -> list:
        """alll_group_probe_literals: Solver.probe for every item in one call -- the items' variables are
        disjoint, so one pass over the union's clauses advances 64 probes of every item.  probes: one
        sequence of literals per item, in the item's own numbering (an empty one: the item is not
        probed); max_rounds is the call's.  At any time; nothing of the group changes.  Returns a list
        with, per item, what Solver.probe returns: the list of result dicts, or with rows=True (results,
        pm, pv), uint32[n_probes_i, n_words_i] each."""
        per = [np.ascontiguousarray(q, np.uint32).ravel() for q in probes]
        if len(per) != self.n_items:
            raise ValueError(f"{len(per)} probe lists for {self.n_items} items")
        offs = np.zeros(self.n_items + 1, np.uint64)
        offs[1:] = np.cumsum([q.size for q in per])
        flat = np.concatenate(per) if per else np.zeros(0, np.uint32)
        total = int(offs[-1])
        res = (N.PropagateResult * max(1, total))()
        nws = [(n + 31) // 32 for n in self.n_vars]
        n_row_words = sum(q.size * nw for q, nw in zip(per, nws))
        pm = np.zeros(n_row_words, np.uint32) if rows else None
        pv = np.zeros(n_row_words, np.uint32) if rows else None
        N.check(self._L.alll_group_probe_literals(self._h, _p(flat, _u32p), _p(offs, _u64p), max_rounds, res,
                                                  _p(pm, _u32p) if rows else None, _p(pv, _u32p) if rows else None,
                                                  n_row_words), "alll_group_probe_literals")
        out, at = [], 0
        for i, (q, nw) in enumerate(zip(per, nws)):
            first = int(offs[i])
            r = [res[first + j].as_dict() for j in range(q.size)]
            if rows:
                out.append((r, pm[at:at + q.size * nw].reshape(q.size, nw), pv[at:at + q.size * nw].reshape(q.size, nw)))
                at += q.size * nw
            else:
                out.append(r)
        return out

    def residuals(self, with_arrays: bool = True) -> List[dict]:
        """alll_group_residual: Solver.residual for every item in one pass over the union.  Returns one
        dict per item, in the item's own clause and variable numbering; an item without thresholds has
        every variable free.  with_arrays=False: the counts alone."""
        out = _ResidualArrays(self._sizes, with_arrays)
        res = (N.ResidualResult * max(1, self.n_items))()
        N.check(self._L.alll_group_residual(self._h, res, *out.args()), "alll_group_residual")
        return out.items([res[i].as_dict() for i in range(self.n_items)])

    def epoch_counters(self) -> dict:
        """Solver.epoch_counters of the union."""
        out = np.zeros(4, np.uint64)
        N.check(self._L.alll_group_epoch_counters(self._h, _p(out, _u64p)), "group_epoch_counters")
        return dict(zip(("rr_restarts", "rr_fails", "restarts", "round_next"), (int(x) for x in out)))


def solve_portfolio(n_vars: int, offsets, literals, seeds, max_iters: int = 0):
    """Many seeds of one instance at once.  Returns (winning_seed, stats, assignment_words) of the
    solved item with the fewest iterations (on a tie the lowest index), or (None, None, None)
    when max_iters capped every seed.  The batch stops after the first slice that solved an item:
    every item still unsolved then has run more iterations than the winner."""
    seeds = [int(s) for s in seeds]
    with BatchSolver([(n_vars, offsets, literals)] * len(seeds), seeds, max_iters=max_iters) as b:
        res = b.solve(first_solved=True)
        solved = [i for i, r in enumerate(res) if r["solved"]]
        if not solved:
            return None, None, None
        best = min(solved, key=lambda i: (res[i]["n_iterations"], i))
        return seeds[best], res[best], b.assignment_words(best)


def cube_thresholds(n_vars: int, cube) -> np.ndarray:
    """The thresholds of a cube, a sequence of encoded literals assumed true: 2v pins x_v = 1, 2v+1
    pins x_v = 0, every other variable is a fair coin.  ValueError for a variable >= n_vars and for
    a cube that names both polarities of one."""
    thr = np.full(n_vars, 1 << 31, np.uint32)
    seen = {}
    for l in cube:
        l = int(l)
        v = l >> 1
        if l < 0 or v >= n_vars:
            raise ValueError(f"cube literal {l} names variable {v} >= n_vars {n_vars}")
        if seen.setdefault(v, l) != l:
            raise ValueError(f"cube names both polarities of variable {v}")
        thr[v] = 0 if l & 1 else 0xFFFFFFFF
    return thr


def _run_cubes(cls, n_vars, offsets, literals, live, seeds, thrs, max_iters, propagate):
    """One solver of solve_cubes over the cubes `live` under thrs[cube index].  -> (result, None); or,
    when the propagation found cubes in conflict, (None, (the surviving cubes, their propagated
    thresholds by cube index)): the caller builds a second solver from them."""
    with cls([(n_vars, offsets, literals)] * len(live), [seeds[i] for i in live], max_iters=max_iters) as b:
        for k, i in enumerate(live):
            b.set_thresholds(k, thrs[i])
        if propagate:
            keep = [k for k, r in enumerate(b.propagate_pins()) if r["status"] != N.PROP_CONFLICT]
            if len(keep) < len(live):
                return None, ([live[k] for k in keep], {live[k]: b.thresholds(k) for k in keep})
        res = b.solve(first_solved=True)
        solved = [k for k, r in enumerate(res) if r["solved"]]
        if not solved:
            return (None, None, None), None
        best = min(solved, key=lambda k: (res[k]["n_iterations"], k))
        return (live[best], res[best], b.assignment_words(best)), None


def _solve_cubes(n_vars, offsets, literals, cubes, seeds, max_iters, propagate):
    offsets = np.ascontiguousarray(offsets, np.uint64)
    literals = np.ascontiguousarray(literals, np.uint32)
    cubes = list(cubes)
    seeds = list(range(1, len(cubes) + 1)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(cubes):
        raise ValueError(f"{len(cubes)} cubes, {len(seeds)} seeds")
    thrs = [cube_thresholds(n_vars, c) for c in cubes]
    live = [i for i, t in enumerate(thrs) if pinned_conflict(n_vars, offsets, literals, t) is None]
    if not live:
        return None, None, None
    fits = batch_fits(n_vars, max(0, offsets.size - 1), literals.size)
    cls = BatchSolver if fits else GroupSolver
    out, left = _run_cubes(cls, n_vars, offsets, literals, live, seeds, thrs, max_iters, propagate)
    if left is not None:  # cubes conflicted: a second solver of the same kind from the survivors
        live, thrs = left
        if not live:
            return None, None, None
        out, _ = _run_cubes(cls, n_vars, offsets, literals, live, seeds, thrs, max_iters, False)
    return out


def solve_cubes(n_vars: int, offsets, literals, cubes, seeds=None, max_iters: int = 0):
    """A cube portfolio: one instance under every cube's pins (cube_thresholds) at once, the first
    cube solved wins.  seeds: one per cube, default 1 .. len(cubes).  Cubes that pin every literal
    of some clause false (pinned_conflict) are dropped on the host; the others run in a BatchSolver
    when the instance fits one, else in a GroupSolver.  Returns (cube index, stats,
    assignment_words) of the solved cube with the fewest iterations (on a tie the lowest index), or
    (None, None, None) when no cube is left or max_iters capped every one."""
    return _solve_cubes(n_vars, offsets, literals, cubes, seeds, max_iters, False)


def solve_cubes_propagated(n_vars: int, offsets, literals, cubes, seeds=None, max_iters: int = 0):
    """solve_cubes with unit propagation: the pins of the cubes left by the depth-0 filter are
    propagated on the device first (propagate_pins); the cubes that turn out conflicting are dropped
    as well, and the others run, in a second solver of the same kind, under their propagated
    thresholds.  The return value is solve_cubes', the indices are the caller's."""
    return _solve_cubes(n_vars, offsets, literals, cubes, seeds, max_iters, True)


def solve_cubes_residual(n_vars: int, offsets, literals, cubes, seeds=None, max_iters: int = 0):
    """solve_cubes_propagated on the residual formulas: after the depth-0 filter and the propagation
    (a GroupSolver of the live cubes), every surviving cube's instance is reduced under its propagated
    thresholds on the device (GroupSolver.residuals) and the residual problems run, under their
    carried thresholds and the cubes' seeds, in a BatchSolver when every one of them fits a batch item
    (batch_fits), else in a GroupSolver -- the choice is made on the residuals' sizes, not on the
    instance's.  The winner is solve_cubes': the solved cube with the fewest iterations, the lowest
    index on a tie; its words are lifted (lift_assignment).  Returns (cube index, stats, the full
    assignment_words), or (None, None, None) when no cube is left or max_iters capped every one.  A
    residual's trajectory is not the pinned instance's (other variable indices, other Philox
    streams): the iteration counts differ from solve_cubes_propagated's."""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    literals = np.ascontiguousarray(literals, np.uint32)
    cubes = list(cubes)
    seeds = list(range(1, len(cubes) + 1)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != len(cubes):
        raise ValueError(f"{len(cubes)} cubes, {len(seeds)} seeds")
    thrs = [cube_thresholds(n_vars, c) for c in cubes]
    live = [i for i, t in enumerate(thrs) if pinned_conflict(n_vars, offsets, literals, t) is None]
    if not live:
        return None, None, None
    with GroupSolver([(n_vars, offsets, literals)] * len(live), [seeds[i] for i in live]) as g:
        for k, i in enumerate(live):
            g.set_thresholds(k, thrs[i])
        keep = [k for k, r in enumerate(g.propagate_pins()) if r["status"] != N.PROP_CONFLICT]
        if not keep:
            return None, None, None
        res = g.residuals()
        full = {k: g.thresholds(k) for k in keep}
    fits = all(batch_fits(res[k]["n_vars"], res[k]["n_clauses"], res[k]["n_literals"]) for k in keep)
    cls = BatchSolver if fits else GroupSolver
    with cls([(res[k]["n_vars"], res[k]["offsets"], res[k]["literals"]) for k in keep], [seeds[live[k]] for k in keep],
             max_iters=max_iters) as b:
        for j, k in enumerate(keep):
            b.set_thresholds(j, res[k]["thr"])
        st = b.solve(first_solved=True)
        solved = [j for j, r in enumerate(st) if r["solved"]]
        if not solved:
            return None, None, None
        best = min(solved, key=lambda j: (st[j]["n_iterations"], j))
        k = keep[best]
        return live[k], st[best], lift_assignment(n_vars, full[k], res[k]["var_map"], b.assignment_words(best))


def split_cubes(n_vars: int, offsets, literals, depth: int, base=(), device: int = -1):
    """Grows a tree of cubes from the split scores (the other half of cube-and-conquer), every cube
    of a level in one pass on the device: a GroupSolver of 2^depth items of the instance, all under
    cube_thresholds(base) at first.  At every level 0 .. depth the pins of all items are propagated
    (an item in conflict is a dead leaf and is left alone from then on) and all items scored (an item
    whose pins satisfy every clause is a leaf); below `depth` every other item i pins its split
    variable: its preferred literal p is 2 var when score_pos >= score_neg, else 2 var + 1, and it
    takes p ^ b with b bit depth - 1 - level of i.  Items that share a prefix of bits stay identical,
    so the leaves are the distinct cubes, in order of their smallest item: depth-first order.
    Returns the list of leaves {"cube": base + the decisions, "status": "open" | "conflict" |
    "satisfied", "thr": the propagated thresholds (None for a conflict)}.  1 <= depth <= 10."""
    if not 1 <= int(depth) <= 10:
        raise ValueError(f"depth {depth} is not in 1 .. 10")
    depth, n_items = int(depth), 1 << int(depth)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    literals = np.ascontiguousarray(literals, np.uint32)
    base = [int(l) for l in base]
    thr0 = cube_thresholds(n_vars, base)
    cubes = [list(base) for _ in range(n_items)]
    status: List[Optional[str]] = [None] * n_items  # (None: live)
    thrs: List[Optional[np.ndarray]] = [None] * n_items
    with GroupSolver([(n_vars, offsets, literals)] * n_items, range(1, n_items + 1), device=device) as g:
        for i in range(n_items):
            g.set_thresholds(i, thr0)
        for level in range(depth + 1):
            for i, r in enumerate(g.propagate_pins()):
                if status[i] is None and r["status"] == N.PROP_CONFLICT:
                    status[i] = "conflict"
            split = g.var_scores()
            for i in range(n_items):
                if status[i] is not None:
                    continue
                s = split[i]
                if s["var"] == n_vars:
                    status[i], thrs[i] = "satisfied", g.thresholds(i)
                elif level == depth:
                    status[i], thrs[i] = "open", g.thresholds(i)
                else:
                    p = 2 * s["var"] + (0 if s["score_pos"] >= s["score_neg"] else 1)
                    d = p ^ ((i >> (depth - 1 - level)) & 1)
                    t = g.thresholds(i)
                    t[s["var"]] = 0 if d & 1 else 0xFFFFFFFF
                    g.set_thresholds(i, t)
                    cubes[i].append(d)
    leaves, seen = [], set()
    for i in range(n_items):
        if tuple(cubes[i]) not in seen:
            seen.add(tuple(cubes[i]))
            leaves.append({"cube": cubes[i], "status": status[i], "thr": thrs[i]})
    return leaves


def solve_cubes_split(n_vars: int, offsets, literals, depth: int, base=(), seeds=None, max_iters: int = 0):
    """A cube portfolio without cubes from the caller: split_cubes, then solve_cubes_propagated on the
    cubes of the leaves that are not in conflict, in leaf order (seeds: None, or one per such leaf).
    Returns (leaves, (leaf index, stats, assignment_words)): the winner's index in `leaves`;
    (leaves, (None, None, None)) when no leaf is left or max_iters capped every one."""
    leaves = split_cubes(n_vars, offsets, literals, depth, base)
    live = [j for j, leaf in enumerate(leaves) if leaf["status"] != "conflict"]
    if not live:
        return leaves, (None, None, None)
    win, st, words = solve_cubes_propagated(n_vars, offsets, literals, [leaves[j]["cube"] for j in live], seeds, max_iters)
    return leaves, ((None, None, None) if win is None else (live[win], st, words))


def _lookahead_candidates(S, n_candidates: int):
    """Step 3 and 4 of failed_literal_reduce from the scores S -> (T, the candidates, their probes)."""
    T = S[0::2].astype(np.int64) + S[1::2].astype(np.int64)
    order = np.argsort(-T, kind="stable")[:n_candidates]  # (stable: the lowest variable first on a tie)
    cands = order[T[order] > 0]
    probes = np.stack([2 * cands, 2 * cands + 1], 1).astype(np.uint32).ravel()
    return T, cands, probes


def _lookahead_judge(n: int, thr, T, cands, results, pm, pv):
    """Steps 5 to 7 of failed_literal_reduce from the candidates' probes -> (candidates, conflict, the
    pass's new pins {variable: value}, failed literals, necessary assignments, lookahead_var); with
    conflict nothing after it is counted."""
    candidates = [(int(v), results[2 * i], results[2 * i + 1]) for i, v in enumerate(cands)]
    status = [(rp["status"], rn["status"]) for _, rp, rn in candidates]
    if any(sp == N.PROP_CONFLICT and sn == N.PROP_CONFLICT for sp, sn in status):
        return candidates, True, {}, 0, 0, n
    new = {}
    for (v, _, _), (sp, sn) in zip(candidates, status):
        if sp == N.PROP_CONFLICT or sn == N.PROP_CONFLICT:
            new[v] = 0 if sp == N.PROP_CONFLICT else 1
    n_failed, n_necessary = len(new), 0
    free = (thr != 0) & (thr != 0xFFFFFFFF)
    best = None
    for i, ((v, rp, rn), (sp, sn)) in enumerate(zip(candidates, status)):
        if sp != N.PROP_FIXPOINT or sn != N.PROP_FIXPOINT:
            continue
        key = ((rp["n_forced"] + 1) * (rn["n_forced"] + 1), int(T[v]), -v)
        if best is None or key > best[0]:
            best = (key, v)
        both = np.unpackbits((pm[2 * i] & pm[2 * i + 1] & ~(pv[2 * i] ^ pv[2 * i + 1])).view(np.uint8),
                             bitorder="little")[:n].astype(bool) & free
        val = np.unpackbits(pv[2 * i].view(np.uint8), bitorder="little")
        for u in np.flatnonzero(both).tolist():
            if u not in new:
                new[u] = int(val[u])
                n_necessary += 1
    return candidates, False, new, n_failed, n_necessary, n if best is None else best[1]


def failed_literal_reduce(n_vars: int, offsets, literals, thr=None, n_candidates: int = 64, max_passes: int = 0,
                          device: bool = True) -> dict:
    """Failed-literal and necessary-assignment reduction of thresholds thr (None: every variable a fair
    coin) by look-ahead probing; device=False: the host path (propagate_pins, var_scores,
    probe_literals), else one Solver and its propagate_pins, var_scores and probe.  A pass
      1. propagates the pins (a conflict ends the call: status "conflict");
      2. takes the split scores (no open clause: status "satisfied");
      3. takes as candidates the n_candidates free variables with the largest T(v) = S[2v] + S[2v+1] > 0,
         ties to the lowest variable;
      4. probes both literals of each, with rows;
      5. both in PROP_CONFLICT: status "conflict";
      6. one in PROP_CONFLICT: its negation is pinned (a failed literal);
      7. both in PROP_FIXPOINT: a variable that both rows pin to the same value and the base leaves free
         is pinned (a necessary assignment);
      8. nothing new pinned: the call ends, status "open"; else after max_passes passes (when non-zero);
         else the next pass.
    The pins of a pass are collected in the candidates' order, the failed literals first; a variable
    already pinned in the pass is not pinned again.  Returns {"thr", "status", "passes", "n_failed",
    "n_necessary", "lookahead_var", "candidates"}: candidates is the last pass's list of (var, result of
    2 var, result of 2 var + 1), empty when that pass ended in step 1 or 2; lookahead_var the candidate,
    among those whose two probes ended in PROP_FIXPOINT, with the largest (n_forced_pos + 1) *
    (n_forced_neg + 1), ties to the larger T, then the lowest variable; n_vars when there is none.
    Integers and fixed tie rules only: both paths return equal dicts."""
    n = int(n_vars)
    if n_candidates < 1:
        raise ValueError("n_candidates must be at least 1")
    thr = np.full(n, 1 << 31, np.uint32) if thr is None else np.array(thr, np.uint32)
    if thr.size != n:
        raise ValueError(f"{thr.size} thresholds for {n} variables")
    solver = Solver(n, offsets, literals) if device else None
    out = {"status": "open", "passes": 0, "n_failed": 0, "n_necessary": 0, "lookahead_var": n, "candidates": []}
    try:
        while True:
            out["passes"] += 1
            out["candidates"], out["lookahead_var"] = [], n
            if device:
                solver.set_thresholds(thr)
                res = solver.propagate_pins()
                thr = solver.thresholds()
            else:
                thr, res = propagate_pins(n, offsets, literals, thr)
            if res["status"] == N.PROP_CONFLICT:
                out["status"] = "conflict"
                break
            S, split = solver.var_scores() if device else var_scores(n, offsets, literals, thr)
            if split["n_open"] == 0:
                out["status"] = "satisfied"
                break
            T, cands, probes = _lookahead_candidates(S, n_candidates)
            if device:
                results, pm, pv = solver.probe(probes, rows=True)
            else:
                results, pm, pv = probe_literals(n, offsets, literals, thr, probes, rows=True)
            out["candidates"], conflict, new, n_failed, n_necessary, look = _lookahead_judge(n, thr, T, cands, results, pm, pv)
            if conflict:
                out["status"] = "conflict"
                break
            out["n_failed"] += n_failed
            out["n_necessary"] += n_necessary
            out["lookahead_var"] = look
            if not new:
                break
            for u, x in new.items():
                thr[u] = 0xFFFFFFFF if x else 0
            if max_passes and out["passes"] >= max_passes:
                break
    finally:
        if solver is not None:
            solver.close()
    out["thr"] = thr
    return out


def _lookahead_split(n: int, S, lookahead_var: int):
    """The split variable of a look-ahead node and its preferred literal from the scores S under the
    node's reduced thresholds: lookahead_var, else (n: no candidate's probes both ended in a fixpoint) the
    arg-max of S[2v] + S[2v+1], the lowest variable on a tie."""
    v = int(lookahead_var)
    if v == n:
        v = int(np.argmax(S[0::2].astype(np.int64) + S[1::2].astype(np.int64)))
    return v, 2 * v + (0 if int(S[2 * v]) >= int(S[2 * v + 1]) else 1)


def split_cubes_lookahead(n_vars: int, offsets, literals, depth: int, base=(), n_candidates: int = 32, device: int = -1,
                          host: bool = False):
    """split_cubes with look-ahead: the same tree and leaf order, but a node first reduces its thresholds
    with r = failed_literal_reduce(thr, n_candidates, max_passes=0): r["status"] "conflict" is a dead leaf
    (thr None), "satisfied" a satisfied one; at `depth` the node is an open leaf with r["thr"]; else it
    splits on r["lookahead_var"] (the arg-max of the scores under r["thr"] when there is none), preferred
    literal 2v when S[2v] >= S[2v+1] else 2v + 1, first child the preferred literal.  Returns the leaves
    {"cube", "status", "thr", "n_failed", "n_necessary", "passes"}, the last three r's.
    host=False: one GroupSolver of 2^depth items in lockstep -- per level, passes of propagate_pins,
    var_scores and one GroupSolver.probes call for all items, until no item pins anything new; at level
    l only the 2^l items whose low depth - l bits are 0 probe, the others copy their thresholds.
    host=True: the same tree from failed_literal_reduce(device=False) and var_scores, no device touched.
    Integers and fixed tie rules only: both return equal lists.  1 <= depth <= 10, n_candidates >= 1."""
    if not 1 <= int(depth) <= 10:
        raise ValueError(f"depth {depth} is not in 1 .. 10")
    if int(n_candidates) < 1:
        raise ValueError("n_candidates must be at least 1")
    depth, n_candidates, n = int(depth), int(n_candidates), int(n_vars)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    literals = np.ascontiguousarray(literals, np.uint32)
    base = [int(l) for l in base]
    thr0 = cube_thresholds(n, base)
    pin = lambda d: 0 if d & 1 else 0xFFFFFFFF  # noqa: E731
    if host:
        leaves = []

        def node(cube, thr, level):
            r = failed_literal_reduce(n, offsets, literals, thr, n_candidates, 0, device=False)
            leaf = {"cube": cube, "status": r["status"], "thr": None if r["status"] == "conflict" else r["thr"],
                    "n_failed": r["n_failed"], "n_necessary": r["n_necessary"], "passes": r["passes"]}
            if r["status"] != "open" or level == depth:
                leaves.append(leaf)
                return
            S, _ = var_scores(n, offsets, literals, r["thr"])
            v, p = _lookahead_split(n, S, r["lookahead_var"])
            for b in (0, 1):
                t = r["thr"].copy()
                t[v] = pin(p ^ b)
                node(cube + [p ^ b], t, level + 1)

        node(list(base), thr0, 0)
        return leaves
    n_items = 1 << depth
    cubes = [list(base) for _ in range(n_items)]
    leaf: List[Optional[dict]] = [None] * n_items  # (None: live)
    count = [{"n_failed": 0, "n_necessary": 0, "passes": 0} for _ in range(n_items)]
    with GroupSolver([(n, offsets, literals)] * n_items, range(1, n_items + 1), device=device) as g:
        for i in range(n_items):
            g.set_thresholds(i, thr0)
        for level in range(depth + 1):
            span = 1 << (depth - level)
            reps = [i for i in range(0, n_items, span) if leaf[i] is None]
            for i in reps:
                count[i] = {"n_failed": 0, "n_necessary": 0, "passes": 0}
            done = {}  # representative -> (status, thr, scores, lookahead_var) once its reduction has ended
            while len(done) < len(reps):
                todo = [i for i in reps if i not in done]
                res = g.propagate_pins()
                for i in todo:
                    count[i]["passes"] += 1
                    if res[i]["status"] == N.PROP_CONFLICT:
                        done[i] = ("conflict", None, None, n)
                todo = [i for i in todo if i not in done]
                if not todo:
                    break
                split, scores = g.var_scores(with_scores=True)
                probes, look = [()] * n_items, {}
                for i in todo:
                    if split[i]["n_open"] == 0:
                        done[i] = ("satisfied", g.thresholds(i), None, n)
                    else:
                        look[i] = _lookahead_candidates(scores[i], n_candidates)
                        probes[i] = look[i][2]
                todo = [i for i in todo if i not in done]
                if not todo:
                    break
                out = g.probes(probes, rows=True)
                for i in todo:
                    thr = g.thresholds(i)
                    T, cands, _ = look[i]
                    _, conflict, new, n_failed, n_necessary, var = _lookahead_judge(n, thr, T, cands, *out[i])
                    if conflict:
                        done[i] = ("conflict", None, None, n)
                        continue
                    count[i]["n_failed"] += n_failed
                    count[i]["n_necessary"] += n_necessary
                    if not new:
                        done[i] = ("open", thr, scores[i], var)
                        continue
                    for u, x in new.items():
                        thr[u] = 0xFFFFFFFF if x else 0
                    g.set_thresholds(i, thr)
            for i in reps:
                status, thr, S, var = done[i]
                if status != "open" or level == depth:
                    for j in range(i, i + span):  # (the items that share the prefix are one leaf)
                        leaf[j] = dict(cube=cubes[j], status=status, thr=thr, **count[i])
                    continue
                v, p = _lookahead_split(n, S, var)
                for j in range(i, i + span):
                    d = p ^ ((j >> (depth - 1 - level)) & 1)
                    t = thr.copy()
                    t[v] = pin(d)
                    g.set_thresholds(j, t)
                    cubes[j].append(d)
    leaves, seen = [], set()
    for i in range(n_items):
        if tuple(cubes[i]) not in seen:
            seen.add(tuple(cubes[i]))
            leaves.append(leaf[i])
    return leaves


def solve_cubes_lookahead(n_vars: int, offsets, literals, depth: int, base=(), n_candidates: int = 32, seeds=None,
                          max_iters: int = 0):
    """solve_cubes_split on the leaves of split_cubes_lookahead: the cubes of the leaves that are not in
    conflict go, in leaf order, through solve_cubes_propagated (seeds: None, or one per such leaf).
    Returns (leaves, (leaf index, stats, assignment_words)): the winner's index in `leaves`;
    (leaves, (None, None, None)) when no leaf is left or max_iters capped every one."""
    leaves = split_cubes_lookahead(n_vars, offsets, literals, depth, base, n_candidates)
    live = [j for j, leaf in enumerate(leaves) if leaf["status"] != "conflict"]
    if not live:
        return leaves, (None, None, None)
    win, st, words = solve_cubes_propagated(n_vars, offsets, literals, [leaves[j]["cube"] for j in live], seeds, max_iters)
    return leaves, ((None, None, None) if win is None else (live[win], st, words))


def shard_plan(n_clauses: int, world: int, rank: int):
    """(clause_begin, clause_end, mask_words_per_rank) of `rank` in the clause-sharded mode."""
    b, e, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    N.check(N.lib().alll_shard_plan(n_clauses, world, rank, ctypes.byref(b), ctypes.byref(e),
                                    ctypes.byref(w)), "shard_plan")
    return int(b.value), int(e.value), int(w.value)


class _MultiPlan(ctypes.Structure):
    _fields_ = [("eval_us_1gpu", ctypes.c_double), ("eval_saved_us", ctypes.c_double),
                ("exchange_us", ctypes.c_double), ("violated_est", ctypes.c_double),
                ("plan", ctypes.c_int), ("pad", ctypes.c_int)]


def plan_multi_gpu(n_clauses: int, n_literals: int, n_vars: int, world: int) -> dict:
    """alll_plan_multi_gpu: {"plan": "shard" | "replicate", and the model's predicted
    microseconds} for one instance on `world` GPUs."""
    p = _MultiPlan()
    N.check(N.lib().alll_plan_multi_gpu(n_clauses, n_literals, n_vars, world, ctypes.byref(p)), "plan_multi_gpu")
    return {"plan": "shard" if p.plan == 1 else "replicate", "eval_us_1gpu": p.eval_us_1gpu,
            "eval_saved_us": p.eval_saved_us, "exchange_us": p.exchange_us, "violated_est": p.violated_est}


def gloo_exchange(group=None):
    """Host exchange over torch.distributed (gloo) for Solver(exchange=...)."""
    import torch
    import torch.distributed as dist

    def ex(op, arr, nbytes):
        world = dist.get_world_size(group)
        if op == N.XCHG_ALLGATHER:
            rank = dist.get_rank(group)
            mine = torch.from_numpy(arr[rank * nbytes:(rank + 1) * nbytes].copy())
            parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(parts, mine, group=group)
            arr[:] = torch.cat(parts).numpy()
        else:
            t = torch.from_numpy(arr.view(np.uint32).astype(np.int64))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            arr.view(np.uint32)[:] = (t.numpy() & 0xFFFFFFFF).astype(np.uint32)

    return ex


def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    N.check(N.lib().alll_comm_unique_id(buf), "comm_unique_id")
    return bytes(buf)


# ------------------------------------------------- reference-shaped API (SATInstance.h)
class Clause:
    """Clause<T> (Clause.h:17-28): encoded literals + the chunk id t_id."""

    def __init__(self, literals: Sequence[int], t_id: int = 0):
        self.literals = list(literals)
        self.t_id = t_id

    def is_not_satisfied(self, vars_) -> bool:  # Clause.h:34-46
        return not any((not vars_[l >> 1]) if (l & 1) else vars_[l >> 1] for l in self.literals)


class VariablesArray:
    """VariablesArray<T> (VariablesArray.h:17-35).  The initial values come from the device
    solver's Philox stream (seeded), not std::random_device."""

    def __init__(self, n_vars: int):
        self.n_vars = int(n_vars)
        self.vars = np.zeros(self.n_vars, np.bool_)


@dataclass
class Statistics:
    """Statistics (SATInstance.h:25-32)."""
    n_iterations: int = 0
    n_resamples: int = 0
    avg_mis_size: int = 0
    n_thread_resamples: List[int] = field(default_factory=list)


class SATInstance:
    """SATInstance<T> (SATInstance.h:39-452) over the MI355X solver.  `seed` and `device`
    are additive keyword arguments; existing call shapes are unchanged."""

    def __init__(self, var_arr: VariablesArray, n_threads: int, seed: int = 1, device: int = -1,
                 max_iters: int = 0):
        self.var_arr = var_arr
        self.n_vars = var_arr.n_vars
        self.n_clauses = 0
        self.n_threads = max(1, int(n_threads))
        self._seed, self._device, self._max_iters = seed, device, max_iters

    @staticmethod
    def _flatten(clauses):
        flat = [cl for chunk in clauses for cl in chunk]
        offs = np.zeros(len(flat) + 1, np.uint64)
        offs[1:] = np.cumsum([len(c.literals) for c in flat])
        lits = np.fromiter((l for c in flat for l in c.literals), np.uint32, int(offs[-1]))
        return offs, lits

    def solve(self, clauses, n_clauses: Optional[int] = None, batch_size: Optional[int] = None) -> Statistics:
        """solve(clauses) -- SATInstance.h:60-66; solve(getEnumeratedClause, n_clauses, batch_size)
        -- the streaming overload, SATInstance.h:70-153 (getEnumeratedClause(index, t_id) -> Clause)."""
        if callable(clauses):
            return self._solve_stream(clauses, int(n_clauses), int(batch_size))
        self.n_clauses += sum(len(c) for c in clauses)
        offs, lits = self._flatten(clauses)
        starts = None
        if self.n_threads > 1:  # the MIS works on the caller's chunks (SATInstance.h:270-276, 414-447)
            if len(clauses) != self.n_threads:
                raise ValueError(f"{self.n_threads} threads need {self.n_threads} clause chunks, got {len(clauses)}")
            starts = np.zeros(self.n_threads + 1, np.uint64)
            starts[1:] = np.cumsum([len(c) for c in clauses])
        with Solver(self.n_vars, offs, lits, seed=self._seed, device=self._device,
                    n_threads=self.n_threads, max_iters=self._max_iters, set_starts=starts) as s:
            d = s.solve()
            self.var_arr.vars[:] = s.assignment().astype(np.bool_)
        thr = [0] * self.n_threads
        thr[0] = d["n_resamples"]
        return Statistics(d["n_iterations"], d["n_resamples"], d["avg_mis_size"], thr)

    def _generated(self, fn, n_clauses: int):
        """Clauses 0 .. n-1 from the callback, each with the t_id of the generator whose range
        holds it (SATInstance.h:74-86: n / T each, the last one the remainder)."""
        T = self.n_threads
        per = n_clauses // T
        out = []
        for i in range(n_clauses):
            t = min(i // per, T - 1) if per else T - 1
            cl = fn(i, t)
            if cl is None:
                raise ValueError(f"clause generator returned None for index {i}")
            out.append(cl)
        return out

    def _solve_stream(self, fn, n_clauses: int, batch_size: int) -> Statistics:
        self.n_clauses = n_clauses
        offs, lits = self._flatten([self._generated(fn, n_clauses)])
        with Solver(self.n_vars, offs, lits, seed=self._seed, device=self._device, n_threads=self.n_threads,
                    max_iters=self._max_iters, stream_batch=max(1, batch_size)) as s:
            d = s.solve()
            self.var_arr.vars[:] = s.assignment().astype(np.bool_)
        thr = [0] * self.n_threads
        thr[0] = d["n_resamples"]
        return Statistics(d["n_iterations"], d["n_resamples"], d["avg_mis_size"], thr)

    def writeDIMACS(self, fn, n_clauses: int, out_f) -> None:  # SATInstance.h:175-203
        self.n_clauses = n_clauses
        out_f.write(f"p cnf {self.n_vars} {n_clauses}\n")
        for i in range(n_clauses):
            cl = fn(i, 0)
            if cl is None:
                raise ValueError(f"clause generator returned None for index {i}")
            toks = [str(-(l >> 1) - 1) if (l & 1) else str((l >> 1) + 1) for l in cl.literals]
            out_f.write("".join(" " + x for x in toks) + " 0\n")

    def verify_validity(self, clauses) -> bool:  # SATInstance.h:156-173
        v = self.var_arr.vars
        return not any(cl.is_not_satisfied(v) for chunk in clauses for cl in chunk)
