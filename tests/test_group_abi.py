"""Group entry points (alll_group_*) without a GPU: the symbols, and the validation that
alll_group_create runs on the host before it opens a device."""
import ctypes

import numpy as np
import pytest


def _create(native, problems, seeds, **opts):
    """alll_group_create over (n_vars, offsets, literals) tuples; returns (rc, message)."""
    L = native.lib()
    keep = [(np.ascontiguousarray(o, np.uint64), np.ascontiguousarray(l, np.uint32)) for _, o, l in problems]
    arr = (native.Problem * max(1, len(problems)))()
    for i, ((n, _, _), (o, l)) in enumerate(zip(problems, keep)):
        arr[i] = native.Problem(n, 0, o.size - 1, o.ctypes.data_as(native._u64p), l.ctypes.data_as(native._u32p))
    sd = np.ascontiguousarray(seeds, np.uint64)
    opt = native.Options()
    L.alll_default_options(ctypes.byref(opt))
    for k, v in opts.items():
        if k == "comm_byte":
            opt.comm_id[17] = v
        else:
            setattr(opt, k, v)
    out = ctypes.c_void_p()
    rc = L.alll_group_create(arr, sd.ctypes.data_as(native._u64p), len(problems), ctypes.byref(opt), ctypes.byref(out))
    msg = native.last_error() if rc else ""
    if rc == 0:
        L.alll_group_destroy(out)
    return rc, msg


GOOD = (4, np.array([0, 2, 3], np.uint64), np.array([0, 3, 6], np.uint32))
GROUP_FUNCS = ("alll_group_create", "alll_group_destroy", "alll_group_solve", "alll_group_run", "alll_group_get_stats",
               "alll_group_get_assignment_words", "alll_group_set_assignment_words", "alll_group_layout",
               "alll_group_eval_kernel")


def test_group_symbols_declared(native):
    from test_abi import header_functions

    declared = header_functions()
    for name in GROUP_FUNCS:
        assert name in declared and name in native.EXPORTED and hasattr(native.lib(), name)
    assert sorted(declared) == sorted(native.EXPORTED)
    import alllsatisfiabilitysolver_amd as pkg

    assert hasattr(pkg, "GroupSolver") and native.GROUP_FIRST_SOLVED == 1


def test_group_create_null_and_empty(native):
    L = native.lib()
    out = ctypes.c_void_p()
    seeds = (ctypes.c_uint64 * 1)(1)
    prob = (native.Problem * 1)()
    assert L.alll_group_create(None, seeds, 1, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_create(prob, None, 1, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_create(prob, seeds, 1, None, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_create(prob, seeds, 0, None, ctypes.byref(out)) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_solve(None, 0, None, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_run(None, 1, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_get_stats(None, 0, None) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_get_assignment_words(None, 0, None, 0) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_set_assignment_words(None, 0, None, 0) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_destroy(None) == native.ALLL_OK


def test_group_create_validates_items(native):
    n, offs, lits = GOOD
    # bad offsets: not starting at 0, decreasing (the codes alll_create gives, the item named)
    rc, msg = _create(native, [GOOD, (n, np.array([1, 2, 3], np.uint64), lits)], [1, 2])
    assert rc == native.ALLL_ERR_BAD_INPUT and "item 1" in msg
    rc, msg = _create(native, [GOOD, GOOD, (n, np.array([0, 3, 2], np.uint64), lits)], [1, 2, 3])
    assert rc == native.ALLL_ERR_BAD_INPUT and "item 2" in msg
    # a literal whose variable is n_vars
    rc, msg = _create(native, [GOOD, (3, offs, lits)], [1, 2])
    assert rc == native.ALLL_ERR_LITERAL_RANGE and "item 1" in msg


def test_group_accepts_items_past_the_batch_limits(native):
    V, C = native.BATCH_MAX_VARS, native.BATCH_MAX_CLAUSES
    big = (V + 1, np.arange(C + 2, dtype=np.uint64) * 3, np.zeros(3 * (C + 1), np.uint32))
    rc, msg = _create(native, [GOOD, big, big], [1, 2, 3])
    assert rc in (native.ALLL_OK, native.ALLL_ERR_NO_DEVICE), msg  # (the device comes after the validation)


@pytest.mark.parametrize("opts", [{"n_threads": 2}, {"n_threads": 0}, {"world": 2}, {"stream_batch": 64},
                                  {"comm_byte": 1}, {"flags": 1 << 7}, {"flags": 1 << 6}, {"flags": 1 << 1},
                                  {"flags": 1 << 9}])
def test_group_create_refuses_options(native, opts):
    rc, msg = _create(native, [GOOD], [1], **opts)
    assert rc == native.ALLL_ERR_UNSUPPORTED, msg
    # refused before the item is looked at, and before any device
    rc2, _ = _create(native, [(3, GOOD[1], GOOD[2])], [1], **opts)
    assert rc2 == native.ALLL_ERR_UNSUPPORTED


@pytest.mark.parametrize("flags", [1 << 0, 1 << 2, 1 << 3, 1 << 4, 1 << 5])
def test_group_create_honours_result_neutral_flags(native, flags):
    rc, msg = _create(native, [GOOD, GOOD], [1, 2], flags=flags)
    assert rc in (native.ALLL_OK, native.ALLL_ERR_NO_DEVICE), msg


def test_group_validation_comes_before_the_device(native):
    """Without a GPU a good group fails with ALLL_ERR_NO_DEVICE and a bad one with its own code;
    with one, the bad group is refused all the same."""
    from alllsatisfiabilitysolver_amd import AlllError, GroupSolver

    with pytest.raises(AlllError) as ei:
        GroupSolver([GOOD, (3, GOOD[1], GOOD[2])], [1, 2])
    assert ei.value.code == native.ALLL_ERR_LITERAL_RANGE
    with pytest.raises(ValueError):
        GroupSolver([GOOD, GOOD], [1])
    if native.lib().alll_device_count() == 0:
        rc, _ = _create(native, [GOOD, GOOD], [1, 2])
        assert rc == native.ALLL_ERR_NO_DEVICE
        with pytest.raises(AlllError) as ei:
            GroupSolver([GOOD, GOOD], [1, 2], max_iters=10)
        assert ei.value.code == native.ALLL_ERR_NO_DEVICE
