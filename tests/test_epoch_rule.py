"""The one-set loop's restart rule for its owner epochs (k_tail / epochs_start_over, alll_create;
DESIGN.md §4.1), restated in plain Python with the epoch width as a parameter and checked against
a brute-force walk: for every first epoch and every number of epochs an iteration may use, no key
epoch of any iteration reaches 2^bits, and a restart is never later than needed by more than one
iteration's worth of epochs.

  an iteration that starts at epoch R uses R, R + 1, ..., R + u with 1 <= u <= cap,
    cap = grid rounds + the tail's cap of 2^20 rounds (u = 1: the reduce's epoch, when no round ran)
  its tail hands next = R + u to the following iteration, whose pre-reduce scatter uses it first;
  next >= restart_at = 2^bits - (cap + 2): the keys are cleared and next = 1
  create: a first epoch >= restart_at is taken as 1 (the keys are fresh)
"""
import itertools
import random

import pytest


def restart_at(bits, cap):
    return (1 << bits) - (cap + 2)


def at_device():
    """EP_RESTART_AT (alll_internal.h): GRID_ROUNDS_MAX = 64 grid rounds, MAX_TAIL_ROUNDS = 2^20."""
    return (1 << 32) - (64 + (1 << 20) + 2)


def first_epoch(bits, cap, e0):
    """alll_create: ALLL_EPOCH0 (clamped to [1, 2^bits - 1]) under the rule."""
    e0 = max(1, min((1 << bits) - 1, e0))
    return (1, 1) if e0 >= restart_at(bits, cap) else (e0, 0)


def tail_end(bits, cap, R, u):
    """k_tail after an iteration that started at R and used the epochs R .. R + u: the epoch it
    hands on and whether it cleared the keys.  The arithmetic is the kernel's: modulo 2^bits."""
    nxt = (R + u) & ((1 << bits) - 1)
    return (1, True) if nxt >= restart_at(bits, cap) else (nxt, False)


def walk(bits, cap, e0, uses):
    """Brute force: every epoch every iteration puts into a key, as unbounded integers."""
    R, restarts = first_epoch(bits, cap, e0)
    top = 0
    for u in uses:
        assert 1 <= u <= cap
        top = max(top, R + u)           # (the largest epoch of the iteration, without the modulus)
        R, over = tail_end(bits, cap, R, u)
        restarts += over
        assert R >= 1
    return top, restarts, R


@pytest.mark.parametrize("cap", [1, 2, 5, 37, 300])
def test_no_epoch_overflows_exhaustive_at_12_bits(cap):
    """bits = 12: every first epoch, and for each the worst case (every iteration uses cap epochs),
    the best case (one each) and one iteration of every size followed by worst cases."""
    bits = 12
    for e0 in range(0, 1 << bits):
        for uses in ([cap] * 40, [1] * 40):
            top, restarts, R = walk(bits, cap, e0, uses)
            assert top < 1 << bits, (e0, uses[0])
        for u in range(1, cap + 1, max(1, cap // 40)):
            top, _, _ = walk(bits, cap, e0, [u] + [cap] * 3)
            assert top < 1 << bits, (e0, u)


def test_restart_comes_when_due_and_not_early():
    """A run that needs the epochs past restart_at restarts exactly once per 2^bits - cap - 2 epochs or
    so; one that stays below never does; after a restart the epochs are small."""
    bits, cap = 12, 37
    at = restart_at(bits, cap)
    assert walk(bits, cap, 1, [cap] * ((at - 2) // cap))[1] == 0
    top, restarts, R = walk(bits, cap, 1, [cap] * ((at - 2) // cap + 1))
    assert restarts == 1 and R == 1 and top >= at
    assert walk(bits, cap, at - 1, [1])[1:] == (1, 1)          # the last start the iteration runs at
    assert first_epoch(bits, cap, at) == (1, 1)               # the first one past the rule: at create
    assert first_epoch(bits, cap, (1 << bits) - 1) == (1, 1)
    assert first_epoch(bits, cap, 0) == (1, 0)
    assert walk(bits, cap, at - 1, [cap])[0] == at - 1 + cap < 1 << bits


def test_sampled_sweep_at_32_bits():
    """The device's width and cap (64 grid rounds at most + 2^20), sampled: starts around restart_at,
    2^31 and 2^32, iterations of random and of extreme sizes."""
    rng = random.Random(5)
    bits = 32
    for grid in (1, 4, 7, 64):  # (the grid rounds a context runs; the rule counts on the most)
        cap = 64 + (1 << 20)
        assert at_device() == restart_at(bits, cap)
        at = restart_at(bits, cap)
        starts = [1, 2, 1 << 31, at - cap - 1, at - cap, at - 2, at - 1, at, at + 1, (1 << 32) - 40, (1 << 32) - 3,
                  (1 << 32) - 1] + [rng.randrange(at - 3 * cap, 1 << 32) for _ in range(200)]
        for e0, big in itertools.product(starts, (True, False)):
            uses = [grid + (1 << 20) if big else rng.randint(1, grid + (1 << 20)) for _ in range(12)]
            top, restarts, R = walk(bits, cap, e0, uses)
            assert top < 1 << 32, (grid, e0)
            assert restarts <= 1 + (e0 >= at - 12 * cap), (grid, e0)
            if e0 >= at - min(uses):
                assert restarts >= 1 and R < 13 * cap
