"""The look-ahead cube splitter on the GPU (split_cubes_lookahead,
solve_cubes_lookahead): the lockstep GroupSolver path against host=True and against the restatement of
lookahead_cases.py -- equal lists of leaves -- and the portfolio built from them."""
import numpy as np
import pytest

import lookahead_cases as L
from test_gpu_prop import satisfied

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(native):
    from alllsatisfiabilitysolver_amd import device_count

    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return True


@pytest.mark.parametrize("name", ["S40_8", "S40_32", "S33_8", "random14", "crafted", "B_16"])
def test_device_equals_host_equals_restatement(gpu, name):
    """8. The leaves of the device path, of host=True and of the restatement are equal: cubes, statuses,
    thresholds, failed literals, necessary assignments and passes."""
    from alllsatisfiabilitysolver_amd import split_cubes_lookahead

    n, offs, lits, depth, base, k = L.split_input(name)
    dev = split_cubes_lookahead(n, offs, lits, depth, base, n_candidates=k)
    print(name, [(leaf["status"], len(leaf["cube"]) - len(base), leaf["n_failed"], leaf["n_necessary"]) for leaf in dev])
    L.same_leaves(dev, L.split_case(name))
    L.same_leaves(dev, split_cubes_lookahead(n, offs, lits, depth, base, n_candidates=k, host=True))


def test_solve_cubes_lookahead(gpu):
    """On S40 at depth 4: the winner satisfies the instance and extends its leaf's cube; the leaves are
    the splitter's."""
    from alllsatisfiabilitysolver_amd import solve_cubes_lookahead, split_cubes_lookahead

    n, offs, lits, _, base, k = L.split_input("S40_8")
    leaves, (win, st, words) = solve_cubes_lookahead(n, offs, lits, 4, base, n_candidates=k, max_iters=500)
    L.same_leaves(leaves, L.split(n, offs, lits, 4, base, k))
    L.same_leaves(leaves, split_cubes_lookahead(n, offs, lits, 4, base, n_candidates=k, host=True))
    assert win is not None and leaves[win]["status"] != "conflict"
    assert st["solved"] == 1 and satisfied(offs, lits, words)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    for d in leaves[win]["cube"]:
        assert bits[d >> 1] == 1 - (d & 1)


def test_a_refuted_instance_has_no_winner(gpu):
    """On S33 every leaf is dead: nothing is left to solve."""
    from alllsatisfiabilitysolver_amd import solve_cubes_lookahead

    n, offs, lits, depth, base, k = L.split_input("S33_8")
    leaves, result = solve_cubes_lookahead(n, offs, lits, depth, base, n_candidates=k)
    L.same_leaves(leaves, L.split_case("S33_8"))
    assert all(leaf["status"] == "conflict" for leaf in leaves) and result == (None, None, None)
