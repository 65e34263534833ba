"""Best-assignment tracking entry points (alll_*track_best, alll_*get_best) without a
GPU: the symbols, their Python front-end, and the argument checks that come before any device work.
A context cannot be created without a GPU (alll_create fails earlier), so the ALLL_ERR_UNSUPPORTED
contexts and everything behind a handle are tested in tests/test_gpu_best.py."""
import ctypes
import inspect

BEST_FUNCS = ("alll_track_best", "alll_get_best", "alll_group_track_best", "alll_group_get_best",
              "alll_batch_track_best", "alll_batch_get_best")


def test_best_symbols_declared(native):
    from test_abi import header_functions

    declared = header_functions()
    for name in BEST_FUNCS:
        assert name in declared and name in native.EXPORTED and hasattr(native.lib(), name), name
    assert sorted(declared) == sorted(native.EXPORTED)


def test_best_python_front_end(native):
    from alllsatisfiabilitysolver_amd import BatchSolver, GroupSolver, Solver, solve_cubes, solve_portfolio

    assert inspect.signature(Solver.__init__).parameters["track_best"].default is False
    assert inspect.signature(Solver.track_best).parameters["on"].default is True
    for cls in (BatchSolver, GroupSolver):
        assert inspect.signature(cls.track_best).parameters["on"].default is True
        assert list(inspect.signature(cls.best).parameters) == ["self", "i"]
    assert list(inspect.signature(Solver.best).parameters) == ["self"]
    # the portfolios keep their signatures
    assert list(inspect.signature(solve_portfolio).parameters) == ["n_vars", "offsets", "literals", "seeds", "max_iters"]
    assert list(inspect.signature(solve_cubes).parameters) == ["n_vars", "offsets", "literals", "cubes", "seeds", "max_iters"]


def test_best_null_handles(native):
    L = native.lib()
    nv, it = ctypes.c_uint64(7), ctypes.c_uint64(7)
    w = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    for on in (0, 1):
        assert L.alll_track_best(None, on) == native.ALLL_ERR_INVALID_ARG
        assert "null" in native.last_error()
        assert L.alll_group_track_best(None, on) == native.ALLL_ERR_INVALID_ARG
        assert L.alll_batch_track_best(None, on) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_get_best(None, ctypes.byref(nv), ctypes.byref(it), w, 4) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_group_get_best(None, 0, ctypes.byref(nv), ctypes.byref(it), w, 4) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_batch_get_best(None, 0, ctypes.byref(nv), ctypes.byref(it), w, 4) == native.ALLL_ERR_INVALID_ARG
    assert L.alll_get_best(None, None, None, None, 0) == native.ALLL_ERR_INVALID_ARG
    # a refused call writes nothing
    assert (nv.value, it.value, list(w)) == (7, 7, [1, 2, 3, 4])
