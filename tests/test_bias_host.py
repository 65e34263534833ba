"""Per-variable resample probabilities on the host: alll_var_threshold and
alll_biased_initial_assignment through the library, against bias_cases.py (the oracle's Philox),
and through tests/cpp/bias_host_dump.cpp, a stand-alone program built with a plain host compiler
under the address and undefined-behaviour sanitizers.  No GPU; no sanitizer on anything loaded
into Python."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from bias_cases import PIN1, biased_init, mixed_thresholds
from conftest import ROOT

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
OK, INVALID_ARG = 0, 1
BELOW_ONE = math.nextafter(1.0, 0.0)  # the largest double below 1
# (probability, return code, threshold)
THRESHOLDS = [(0.0, OK, 0), (1.0, OK, PIN1), (0.5, OK, 1 << 31), (2.0 ** -32, OK, 1), (BELOW_ONE, OK, 0xFFFFFFFE),
              (-0.0, OK, 0), (2.0 ** -33, OK, 0), (0.25, OK, 1 << 30), (1.0 - 2.0 ** -32, OK, 0xFFFFFFFE),
              (float("nan"), INVALID_ARG, None), (-0.1, INVALID_ARG, None), (1.5, INVALID_ARG, None),
              (float("inf"), INVALID_ARG, None)]
SIZES = [1, 3, 4, 5, 31, 32, 33, 203]


def thresholds_for(n):
    """Both pins, biases, and pins at the first and last variable and around the call (4) and word
    (32) boundaries."""
    return mixed_thresholds(n, 100 + n, must=[(0, PIN1), (3, 0), (4, PIN1), (31, 0), (32, PIN1),
                                              (n - 1, 0 if n & 1 else PIN1), (1, 0)])


def test_var_threshold(native):
    L = native.lib()
    for p, rc, want in THRESHOLDS:
        t = ctypes.c_uint32(12345)
        assert L.alll_var_threshold(p, ctypes.byref(t)) == rc, p
        if rc == OK:
            assert t.value == want, p
    assert L.alll_var_threshold(0.5, None) == INVALID_ARG


def test_var_thresholds_vectorised(native):
    from alllsatisfiabilitysolver_amd import AlllError, var_thresholds

    good = [(p, t) for p, rc, t in THRESHOLDS if rc == OK]
    got = var_thresholds([p for p, _ in good])
    assert got.dtype == np.uint32 and got.tolist() == [t for _, t in good]
    for p, rc, _ in THRESHOLDS:
        if rc != OK:
            with pytest.raises(AlllError) as ei:
                var_thresholds([0.5, p])
            assert ei.value.code == INVALID_ARG


@pytest.mark.parametrize("n", SIZES)
def test_biased_initial_assignment_matches_the_oracle_stream(native, oracle_mod, n):
    from alllsatisfiabilitysolver_amd import biased_initial_assignment

    thr = thresholds_for(n)
    assert n < 2 or ((thr == 0).any() and (thr == PIN1).any())  # both pins
    for seed in (1, (7 << 32) | 5):
        got = biased_initial_assignment(seed, n, thr)
        np.testing.assert_array_equal(oracle_mod.pack_bools(got), biased_init(oracle_mod, seed, n, thr))
        assert (got[thr == PIN1] == 1).all() and (got[thr == 0] == 0).all()


def test_fair_threshold_is_not_the_unbiased_stream(native):
    """thr = 2^31 everywhere is a fair coin drawn from other Philox calls than the unbiased fill."""
    from alllsatisfiabilitysolver_amd import biased_initial_assignment

    n = 4096
    plain = np.zeros(n, np.uint8)
    assert native.lib().alll_initial_assignment(1, n, plain.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == OK
    fair = biased_initial_assignment(1, n, np.full(n, 1 << 31, np.uint32))
    assert 0.4 < np.mean(fair != plain) < 0.6


def test_frequency_of_ones(native):
    """n = 100,000 variables at p = 0.25: the share of ones within 5 sigma of 0.25,
    sigma = sqrt(p (1 - p) / n) = 0.00137."""
    from alllsatisfiabilitysolver_amd import biased_initial_assignment, var_thresholds

    n, p = 100_000, 0.25
    thr = np.full(n, var_thresholds(p)[0], np.uint32)
    share = float(biased_initial_assignment(3, n, thr).mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"share of ones {share:.5f}, sigma {sigma:.5f}")
    assert abs(share - p) <= 5 * sigma


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("bias_host")
    exe = str(d / "bias_host_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "bias_host_dump.cpp"), os.path.join(CSRC, "alll_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return [ln.split() for ln in r.stdout.splitlines()]

    return d, run


def test_sanitized_var_threshold(dump):
    _, run = dump
    rows = run("thr", *[f"{struct.unpack('<Q', struct.pack('<d', p))[0]:x}" for p, _, _ in THRESHOLDS])
    assert len(rows) == len(THRESHOLDS)
    for (p, rc, want), row in zip(THRESHOLDS, rows):
        assert row[0] == "thr" and int(row[1]) == rc, p
        assert int(row[2]) == (want if rc == OK else 12345), p  # (a refused call leaves the output alone)


@pytest.mark.parametrize("n", SIZES)
def test_sanitized_biased_initial_assignment(dump, oracle_mod, n):
    d, run = dump
    thr = thresholds_for(n)
    f = d / f"thr{n}.bin"
    f.write_bytes(thr.astype("<u4").tobytes())
    seed = (9 << 32) | 11
    rows = dict((r[0], r[1] if len(r) > 1 else "") for r in run("init", seed, n, f))
    assert int(rows["rc"]) == OK
    got = np.array([int(ch) for ch in rows["bits"]], np.uint8)
    np.testing.assert_array_equal(oracle_mod.pack_bools(got), biased_init(oracle_mod, seed, n, thr))
