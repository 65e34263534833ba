"""Crafted conflict graphs for the LFMIS paths (test-side only; DESIGN.md, tests).

Random k-SAT has shallow, low-degree conflict graphs: an iteration settles in a handful of claim
rounds and no variable is claimed by more than a few clauses.  The instances here have a known
MIS and a known dependency depth, so that the deep and the dense ends of every LFMIS path run:

  chain(m), rchain(m)     clause i = (x_i or x_{i+1}): one dependent round per MIS clause
  combs(P, D, k)          P independent chains of D clauses, interleaved over the clause ids
  ragged_combs(P, D)      the same with widths alternating 2 and 5
  star(m, H)              clause c = (hub_{c % H} or private_c): hub degree m / H
  dense(m, n, k)          random literals over a handful of variables
  copies(m)               m copies of one clause

Every generator returns (n_vars, offs uint64, lits uint32) with lit = 2 * var + sign.  All but
`dense` hold positive literals only, so the all-false assignment violates every clause.

claim_rounds() is the synchronous claim/join scheme the kernels implement, in plain numpy: its
MIS must equal the serial greedy's, and its round count is the depth of the instance.
"""
import functools

import numpy as np


def _csr(widths, var_rows):
    offs = np.zeros(len(widths) + 1, np.uint64)
    offs[1:] = np.cumsum(widths)
    lits = (np.concatenate(var_rows).astype(np.uint32) << np.uint32(1)) if len(var_rows) else np.zeros(0, np.uint32)
    return offs, lits


def chain(m):
    """Clause i = (x_i or x_{i+1}): MIS = the even clauses, ceil(m / 2) dependent rounds."""
    i = np.arange(m, dtype=np.uint32)
    lits = np.stack([2 * i, 2 * (i + 1)], 1).ravel().astype(np.uint32)
    return m + 1, np.arange(m + 1, dtype=np.uint64) * np.uint64(2), lits


def rchain(m):
    """Clause i = (x_{m-i} or x_{m-i-1}): the chain with clause ids against the variable order."""
    i = np.arange(m, dtype=np.uint32)
    lits = np.stack([2 * (m - i), 2 * (m - i - 1)], 1).ravel().astype(np.uint32)
    return m + 1, np.arange(m + 1, dtype=np.uint64) * np.uint64(2), lits


def _combs(P, D, widths):
    """P chains of D clauses; clause c is position c // P of chain c % P and has widths[c // P]
    variables, the last of which is the first of the chain's next clause."""
    widths = np.asarray(widths, np.int64)
    start = np.zeros(D, np.int64)
    start[1:] = np.cumsum(widths[:-1] - 1)
    per_chain = int(start[-1] + widths[-1])
    c = np.arange(P * D, dtype=np.int64)
    pos, ch = c // P, c % P
    w = widths[pos]
    offs = np.zeros(P * D + 1, np.uint64)
    offs[1:] = np.cumsum(w)
    within = np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1].astype(np.int64), w)
    var = np.repeat(ch * per_chain + start[pos], w) + within
    return P * per_chain, offs, (var.astype(np.uint32) << np.uint32(1))


def combs(P, D, k):
    return _combs(P, D, np.full(D, k))


def ragged_combs(P, D):
    return _combs(P, D, np.where(np.arange(D) % 2 == 0, 2, 5))


def star(m, H):
    """Clause c = (hub_{c % H} or private_c); hubs are variables 0 .. H-1.  MIS = clauses 0 .. H-1."""
    c = np.arange(m, dtype=np.uint32)
    lits = np.stack([2 * (c % np.uint32(H)), 2 * (np.uint32(H) + c)], 1).ravel().astype(np.uint32)
    return H + m, np.arange(m + 1, dtype=np.uint64) * np.uint64(2), lits


def dense(m, n, k, seed=3):
    """Random literals over n variables (tautologies and repeated variables allowed)."""
    rng = np.random.default_rng(seed)
    lits = rng.integers(0, 2 * n, m * k).astype(np.uint32)
    return n, np.arange(m + 1, dtype=np.uint64) * np.uint64(k), lits


def copies(m):
    """m copies of (x0 or x1 or x2) over three variables."""
    return 3, np.arange(m + 1, dtype=np.uint64) * np.uint64(3), np.tile(np.array([0, 2, 4], np.uint32), m)


# name -> (generator, arguments, (|U|, |M|) of the first iteration from all-false at T = 1,
#          claim rounds of that iteration or None where the issue states none)
STRUCTURES = {
    "chain513": (chain, (513,), (513, 257), 257),
    "chain4097": (chain, (4097,), (4097, 2049), 2049),          # one tile (4096) plus one clause
    "chain20000": (chain, (20000,), (20000, 10000), 10000),     # five tiles, a link across each boundary
    "rchain4097": (rchain, (4097,), (4097, 2049), 2049),
    "combs64x300": (combs, (64, 300, 3), (19200, 9600), 150),
    "combs5000x6": (combs, (5000, 6, 2), (30000, 15000), 3),
    "ragged_combs64x300": (ragged_combs, (64, 300), (19200, 9600), 150),
    "star1023": (star, (1023, 1), (1023, 1), 1),                # hub degree below HOT_THR_MIN = 1024
    "star1024": (star, (1024, 1), (1024, 1), 1),                # ... and at it
    "star20000": (star, (20000, 1), (20000, 1), 1),
    "star20000x7": (star, (20000, 7), (20000, 7), 1),
    "star513hubs": (star, (513 * 1024, 513), (513 * 1024, 513), 1),  # HOT_MAX = 512 hubs plus one
    "dense8": (dense, (5000, 8, 3), (574, 3), None),
    "dense40": (dense, (5000, 40, 3), (629, 11), None),
    "copies9000": (copies, (9000,), (9000, 1), 1),
}
DEEP = ("chain513", "chain4097", "chain20000", "rchain4097", "combs64x300", "combs5000x6", "ragged_combs64x300")


@functools.lru_cache(maxsize=None)
def structure(name):
    """(n_vars, offs, lits) of STRUCTURES[name]; built once, the arrays are read-only."""
    gen, args = STRUCTURES[name][:2]
    n, offs, lits = gen(*args)
    offs.setflags(write=False)
    lits.setflags(write=False)
    return n, offs, lits


def all_false(n_vars):
    return np.zeros((n_vars + 31) // 32, np.uint32)


def claim_rounds(n_vars, offs, lits, U):
    """The synchronous claim/join rounds over the clauses U (ascending ids): in every round a
    live clause joins iff it has the smallest id among the live clauses on each of its
    variables; clauses sharing a variable with a joiner die; until none is live.  Returns (M
    ascending uint32, rounds)."""
    offs = np.asarray(offs).astype(np.int64)
    live = np.sort(np.asarray(U, np.int64))
    w = (offs[1:] - offs[:-1])[live]
    if (w == 0).any():
        raise ValueError("claim_rounds: empty clause")
    # variables of the clauses in U as a matrix padded with each clause's first variable
    wmax = int(w.max()) if live.size else 1
    col = np.minimum(np.arange(wmax)[None, :], (w - 1)[:, None])
    V = (np.asarray(lits)[offs[live][:, None] + col] >> 1).astype(np.int64)
    ids = live.copy()
    owner = np.full(max(1, n_vars), -1, np.int64)
    used = np.zeros(max(1, n_vars), bool)
    joined, rounds = [], 0
    while ids.size:
        rounds += 1
        # claims in descending id order: of repeated indices the last assignment (smallest id) stays
        owner[V[::-1].ravel()] = np.repeat(ids[::-1], wmax)
        mine = owner[V] == ids[:, None]
        join = mine[:, 0].copy()
        for j in range(1, wmax):
            join &= mine[:, j]
        joined.append(ids[join])
        used[V[join].ravel()] = True
        hit = used[V]
        keep = ~hit[:, 0]
        for j in range(1, wmax):
            keep &= ~hit[:, j]
        ids, V = ids[keep], V[keep]
    M = np.sort(np.concatenate(joined)) if joined else np.zeros(0, np.int64)
    return M.astype(np.uint32), rounds
