"""Batch entry points (alll_batch_*) without a GPU: the limits, and the validation that
alll_batch_create runs on the host before it touches a device."""
import ctypes

import numpy as np
import pytest


def _create(native, problems, seeds, **opts):
    """alll_batch_create over (n_vars, offsets, literals) tuples; returns (rc, message)."""
    L = native.lib()
    keep = [(np.ascontiguousarray(o, np.uint64), np.ascontiguousarray(l, np.uint32)) for _, o, l in problems]
    arr = (native.Problem * max(1, len(problems)))()
    for i, ((n, _, _), (o, l)) in enumerate(zip(problems, keep)):
        arr[i] = native.Problem(n, 0, o.size - 1, o.ctypes.data_as(native._u64p), l.ctypes.data_as(native._u32p))
    sd = np.ascontiguousarray(seeds, np.uint64)
    opt = native.Options()
    L.alll_default_options(ctypes.byref(opt))
    for k, v in opts.items():
        setattr(opt, k, v)
    out = ctypes.c_void_p()
    rc = L.alll_batch_create(arr, sd.ctypes.data_as(native._u64p), len(problems), ctypes.byref(opt), ctypes.byref(out))
    msg = native.last_error() if rc else ""
    if rc == 0:
        L.alll_batch_destroy(out)
    return rc, msg


GOOD = (4, np.array([0, 2, 3], np.uint64), np.array([0, 3, 6], np.uint32))


def test_batch_fits_limits(native):
    from alllsatisfiabilitysolver_amd import batch_fits

    V, C, Lt = native.BATCH_MAX_VARS, native.BATCH_MAX_CLAUSES, native.BATCH_MAX_LITERALS
    assert V >= 8192 and C >= 8192 and Lt >= 24576
    assert batch_fits(V, C, Lt) and batch_fits(0, 0, 0)
    assert not batch_fits(V + 1, C, Lt)
    assert not batch_fits(V, C + 1, Lt)
    assert not batch_fits(V, C, Lt + 1)
    assert native.lib().alll_batch_fits(V, C, Lt) == 1 and native.lib().alll_batch_fits(V, C, Lt + 1) == 0


def test_batch_symbols_declared(native):
    from test_abi import header_functions

    declared = header_functions()
    for name in ("alll_batch_fits", "alll_batch_create", "alll_batch_destroy", "alll_batch_solve", "alll_batch_run",
                 "alll_batch_get_stats", "alll_batch_get_assignment_words", "alll_batch_set_assignment_words",
                 "alll_batch_set_slice"):
        assert name in declared and name in native.EXPORTED and hasattr(native.lib(), name)
    assert sorted(declared) == sorted(native.EXPORTED)


def test_batch_create_null_and_empty(native):
    L = native.lib()
    out = ctypes.c_void_p()
    seeds = (ctypes.c_uint64 * 1)(1)
    prob = (native.Problem * 1)()
    assert L.alll_batch_create(None, seeds, 1, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_create(prob, None, 1, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_create(prob, seeds, 1, None, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_create(prob, seeds, 0, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_solve(None, 0, None, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_run(None, 1, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_set_slice(None, 1) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_destroy(None) == native.ALLL_OK


def test_batch_create_validates_items(native):
    n, offs, lits = GOOD
    # bad offsets: not starting at 0, decreasing
    rc, msg = _create(native, [GOOD, (n, np.array([1, 2, 3], np.uint64), lits)], [1, 2])
    assert rc == native.ALLL_ERR_BAD_INPUT and "item 1" in msg
    rc, msg = _create(native, [GOOD, GOOD, (n, np.array([0, 3, 2], np.uint64), lits)], [1, 2, 3])
    assert rc == native.ALLL_ERR_BAD_INPUT and "item 2" in msg
    # a literal whose variable is n_vars
    rc, msg = _create(native, [GOOD, (3, offs, lits)], [1, 2])
    assert rc == native.ALLL_ERR_LITERAL_RANGE and "item 1" in msg


def test_batch_create_refuses_items_past_the_limits(native):
    V, C, Lt = native.BATCH_MAX_VARS, native.BATCH_MAX_CLAUSES, native.BATCH_MAX_LITERALS
    big_v = (V + 1, GOOD[1], GOOD[2])
    big_c = (4, np.zeros(C + 2, np.uint64), np.zeros(0, np.uint32))
    big_l = (4, np.array([0, Lt + 1], np.uint64), np.zeros(Lt + 1, np.uint32))
    for item in (big_v, big_c, big_l):
        rc, msg = _create(native, [GOOD, GOOD, GOOD, item], [1, 2, 3, 4])
        assert rc == native.ALLL_ERR_UNSUPPORTED and "item 3" in msg, msg
    # exactly at the limits: accepted by the validation (the device comes after it)
    at = (V, np.arange(C + 1, dtype=np.uint64) * 3, np.zeros(Lt, np.uint32))
    rc, msg = _create(native, [at], [1])
    assert rc in (native.ALLL_OK, native.ALLL_ERR_NO_DEVICE), msg


@pytest.mark.parametrize("opts", [{"n_threads": 2}, {"n_threads": 0}, {"world": 2}, {"stream_batch": 64},
                                  {"flags": 1 << 7}, {"flags": 1 << 0}, {"flags": 1 << 6}])
def test_batch_create_refuses_options(native, opts):
    rc, msg = _create(native, [GOOD], [1], **opts)
    assert rc == native.ALLL_ERR_UNSUPPORTED, msg
    # refused before the item is looked at, and before any device
    rc2, _ = _create(native, [(3, GOOD[1], GOOD[2])], [1], **opts)
    assert rc2 == native.ALLL_ERR_UNSUPPORTED


def test_batch_create_fails_loudly_without_gpu(native):
    from alllsatisfiabilitysolver_amd import AlllError, BatchSolver

    if native.lib().alll_device_count() > 0:
        pytest.skip("GPU visible")
    rc, _ = _create(native, [GOOD, GOOD], [1, 2])
    assert rc == native.ALLL_ERR_NO_DEVICE
    with pytest.raises(AlllError) as ei:
        BatchSolver([GOOD, GOOD], [1, 2], max_iters=10)
    assert ei.value.code == native.ALLL_ERR_NO_DEVICE
    # validation still comes first
    with pytest.raises(AlllError) as ei:
        BatchSolver([GOOD, (3, GOOD[1], GOOD[2])], [1, 2])
    assert ei.value.code == native.ALLL_ERR_LITERAL_RANGE
