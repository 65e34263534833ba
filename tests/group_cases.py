"""Block-diagonal groups (test-side only): the numpy restatement of the union the
planner builds, and the item sets the CPU and GPU tests share.

An item is (n_vars, offsets uint64, literals uint32).  compose() lays items side by side: every item
starts a new 32-variable assignment word, keeps its clause order and gets its literals shifted to
its variables."""
import numpy as np


def compose(items):
    """-> (n_vars, offsets, literals, places) of the union; places[i] = dict(var_base, word_base,
    n_words, clause_base, n_clauses, lit_base)."""
    places, offs, lits = [], [np.zeros(1, np.uint64)], []
    words = clauses = nlit = 0
    for n, o, l in items:
        o, l = np.asarray(o, np.uint64), np.asarray(l, np.uint32)
        m = o.size - 1
        places.append(dict(var_base=32 * words, word_base=words, n_words=(n + 31) // 32, clause_base=clauses,
                           n_clauses=m, lit_base=nlit, n_vars=n))
        offs.append(o[1:] + np.uint64(nlit))
        lits.append(l[:int(o[-1])] + np.uint32(2 * 32 * words))
        words += (n + 31) // 32
        clauses += m
        nlit += int(o[-1])
    n_vars = places[-1]["var_base"] + places[-1]["n_vars"]
    return n_vars, np.concatenate(offs), (np.concatenate(lits) if lits else np.zeros(0, np.uint32)), places


def word_table(items, seeds):
    """The planner's per-word table: rows {seed lo, seed hi, local word, tail mask}."""
    rows = []
    for (n, _, _), s in zip(items, seeds):
        nw = (n + 31) // 32
        for w in range(nw):
            tail = (1 << (n & 31)) - 1 if (w == nw - 1 and n & 31) else 0xFFFFFFFF
            rows.append((s & 0xFFFFFFFF, s >> 32, w, tail))
    return rows


def mixed_bag():
    """Six items with distinct seeds (the issue's mixed bag): past the batch's clause limit and
    unsolved at the cap; past its variable limit and quickly solved; tiny 2-SAT with n = 33; no
    clause at all; mixed widths 1-5 (the union becomes ragged); the first problem's arrays again."""
    from alllsatisfiabilitysolver_amd import generate_ksat, generate_mixed

    big = (2500, *generate_ksat(1, 2500, 10000, 3))
    items = [big,
             (9000, *generate_ksat(2, 9000, 9000, 3)),
             (33, *generate_ksat(3, 33, 20, 2)),
             (10, np.zeros(1, np.uint64), np.zeros(0, np.uint32)),
             (300, *generate_mixed(5, 300, 700, 1, 5)),
             big]
    return items, [11, 12, 13, 14, 15, 16]


def oracle_step(o, n, offs, lits, A, seed, it):
    """One iteration of the loop from assignment A at resample round `it` with the oracle's own
    primitives: -> (violated list, MIS, next assignment)."""
    m = len(offs) - 1
    _, vm = o.eval_mask(offs, lits, A)
    U = o.mask_to_list(m, vm)
    M = o.lfmis(n, offs, lits, U)
    return U, M, o.resample_words(A.copy(), seed, it, o.clause_vars(offs, lits, M))
