"""Per-variable resample probabilities (test-side only): the biased stream and one
iteration of the loop under it, composed from the oracle's own primitives (philox4x32_10, eval_mask,
mask_to_list, lfmis / rr_mis, clause_vars) -- nothing of the code under test.

    u(v, it) = Philox4x32-10(key = seed, ctr = {v >> 2, it lo, 1, it hi})[v & 3]
    u0(v)    = Philox4x32-10(key = seed, ctr = {v >> 2, 0, 0xFFFFFFFE, 0})[v & 3]     (initial fill)
    bit      = thr[v] == 0xFFFFFFFF ? 1 : (u < thr[v])"""
import numpy as np

PIN1 = 0xFFFFFFFF


def biased_bits(o, seed, it, vs, thr):
    """The draws of variables vs at resample round `it` (None: the initial fill) -> uint32 0/1."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    calls, out = {}, []
    for v in np.asarray(vs, np.int64).tolist():
        q = v >> 2
        if q not in calls:
            ctr = (q, 0, 0xFFFFFFFE, 0) if it is None else (q, it & 0xFFFFFFFF, 1, it >> 32)
            calls[q] = [int(x) for x in o.philox4x32_10(ctr, key)]
        t = int(thr[v])
        out.append(1 if t == PIN1 else int(calls[q][v & 3] < t))
    return np.array(out, np.uint32)


def biased_init(o, seed, n, thr):
    """The biased initial assignment as packed words (the bits above n clear)."""
    return o.pack_bools(biased_bits(o, seed, None, np.arange(n), thr)) if n else np.zeros(0, np.uint32)


def biased_step(o, n, offs, lits, A, seed, it, thr, T=1):
    """One iteration from assignment A at resample round `it`: -> (violated mask words, violated
    list, MIS in clause order, next assignment).  T > 1: the round-robin MIS over T chunks."""
    m = len(offs) - 1
    _, vm = o.eval_mask(offs, lits, A)
    U = o.mask_to_list(m, vm)
    M = o.lfmis(n, offs, lits, U) if T == 1 else np.sort(o.rr_mis(n, offs, lits, U, T))
    vs = np.unique(o.clause_vars(offs, lits, M)).astype(np.int64)  # a variable repeated in a clause is drawn once
    B = A.copy()
    if vs.size:
        bits = biased_bits(o, seed, it, vs, thr)
        w, sh = vs >> 5, (vs & 31).astype(np.uint32)
        np.bitwise_and.at(B, w, ~(np.uint32(1) << sh))
        np.bitwise_or.at(B, w, bits << sh)
    return vm, U, M, B


def mixed_thresholds(n, seed, must=()):
    """Random thresholds: ~10 % pinned to 0, ~10 % pinned to 1, the rest uniform in (0, 2^32 - 1);
    `must` = (variable, threshold) pairs imposed afterwards."""
    rng = np.random.default_rng(seed)
    thr = rng.integers(1, PIN1, n, dtype=np.uint64).astype(np.uint32)
    r = rng.random(n)
    thr[r < 0.1] = 0
    thr[r > 0.9] = PIN1
    for v, t in must:
        if v < n:
            thr[v] = t
    return thr
