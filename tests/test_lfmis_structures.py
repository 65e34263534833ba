"""The crafted conflict graphs of tests/lfmis_structures.py on the CPU: the synchronous
claim/join rounds (claim_rounds, plain numpy) pick exactly the serial greedy's MIS
(oracle.lfmis), in exactly the number of rounds the construction implies.  This pins the values
the GPU tests expect, and shows that the depth figures are properties of the instances, not of
the kernels."""
import numpy as np
import pytest

from lfmis_structures import STRUCTURES, all_false, claim_rounds, structure


@pytest.mark.parametrize("name", list(STRUCTURES))
def test_claim_rounds_equal_the_greedy(oracle_mod, name):
    o = oracle_mod
    n, offs, lits = structure(name)
    m = offs.size - 1
    (nu_want, nm_want), rounds_want = STRUCTURES[name][2:]
    nu, vm = o.eval_mask(offs, lits, all_false(n))
    U = o.mask_to_list(m, vm)
    assert nu == U.size == nu_want
    if not name.startswith("dense"):
        np.testing.assert_array_equal(U, np.arange(m, dtype=np.uint32))
    M_greedy = o.lfmis(n, offs, lits, U)
    assert M_greedy.size == nm_want
    M, rounds = claim_rounds(n, offs, lits, U)
    np.testing.assert_array_equal(M, M_greedy)
    if rounds_want is not None:
        assert rounds == rounds_want
    # the first row of the oracle's loop from all-false: the same figures
    _, _, rows = o.solve(n, offs, lits, 1, max_iters=2, A0=all_false(n), trace=True)
    assert rows[0][1:3] == (nu_want, nm_want)


def test_structure_shapes():
    """The literal shapes the table in DESIGN.md states."""
    n, offs, lits = structure("chain4097")
    assert n == 4098 and lits[:4].tolist() == [0, 2, 2, 4] and lits[-2:].tolist() == [2 * 4096, 2 * 4097]
    n, offs, lits = structure("rchain4097")
    assert lits[:4].tolist() == [2 * 4097, 2 * 4096, 2 * 4096, 2 * 4095] and lits[-2:].tolist() == [2, 0]
    n, offs, lits = structure("combs64x300")
    v = (lits >> 1).reshape(-1, 3)
    assert n == 64 * 601 and v[64, 0] == v[0, 2] and v[1, 0] == 601  # neighbours share one variable
    assert np.unique(v).size == n
    n, offs, lits = structure("ragged_combs64x300")
    w = np.diff(offs.astype(np.int64))
    assert w[:64].tolist() == [2] * 64 and w[64:128].tolist() == [5] * 64 and offs[-1] == 64 * 150 * 7
    assert lits[int(offs[64])] == lits[int(offs[1]) - 1]
    n, offs, lits = structure("star513hubs")
    assert n == 513 * 1025 and np.bincount(lits[0::2] >> 1).tolist() == [1024] * 513
    n, offs, lits = structure("star1023")
    assert offs[-1] // n == 1  # L / n = 1: the hot threshold is HOT_THR_MIN itself
