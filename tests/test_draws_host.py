"""The random streams of alll_draws.h, the one definition that the kernels and
the host helpers share, against the oracle's primitives: Philox itself (the Random123 known-answer
vectors), the fill and resample words, the biased fill and one biased resample round.  Through
tests/cpp/draws_dump.cpp, a stand-alone program that includes the header alone, built with a plain
host compiler under the address and undefined-behaviour sanitizers.  No GPU; no sanitizer on
anything loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from bias_cases import PIN1, biased_bits, biased_init
from conftest import ROOT
from test_bias_host import SIZES, thresholds_for  # n in {1, 3, 4, 5, 31, 32, 33, 203}; both pins, pins at the call and word edges

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
SEEDS = (1, (7 << 32) | 5)
ROUNDS = (0, 1, (1 << 32) + 3)
N_WORDS = 7
KAT = [((0, 0, 0, 0), (0, 0)), ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))]  # tests/test_oracle.py::test_philox_kat
KAT_OUT = [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
           [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("draws_host")
    exe = str(d / "draws_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "draws_dump.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        return [[ln.split()[0]] + [int(x, 16) for x in ln.split()[1:]] for ln in r.stdout.splitlines()]

    return d, run


def test_philox_known_answers(dump, oracle_mod):
    rows = dump[1]("kat")
    assert [r[0] for r in rows] == ["kat"] * 3
    for (ctr, key), want, row in zip(KAT, KAT_OUT, rows):
        assert row[1:] == want == [int(x) for x in oracle_mod.philox4x32_10(ctr, key)]


@pytest.mark.parametrize("seed", SEEDS)
def test_fill_and_resample_words(dump, oracle_mod, seed):
    o = oracle_mod
    rows = dump[1]("words", seed, N_WORDS, *ROUNDS)
    assert [r[0] for r in rows] == ["fill"] + ["resample"] * len(ROUNDS)
    assert rows[0][1:] == o.init_assignment(seed, 32 * N_WORDS).tolist()
    for it, row in zip(ROUNDS, rows[1:]):
        assert row[1] == it
        assert row[2:] == o.pack_bools(o.philox_bits(seed, it, np.arange(32 * N_WORDS))).tolist(), it


@pytest.mark.parametrize("n", SIZES)
def test_biased_fill_and_resample_round(dump, oracle_mod, n):
    d, run = dump
    thr = thresholds_for(n)
    assert n < 2 or ((thr == 0).any() and (thr == PIN1).any())  # both pins
    f = d / f"thr{n}.bin"
    f.write_bytes(thr.astype("<u4").tobytes())
    for seed, it in zip(SEEDS, ROUNDS[1:]):
        rows = dict((r[0], r[1:]) for r in run("biased", seed, it, n, f))
        assert sorted(rows) == ["draw16", "fill", "var"]
        assert rows["fill"] == biased_init(oracle_mod, seed, n, thr).tolist()
        want = oracle_mod.pack_bools(biased_bits(oracle_mod, seed, it, np.arange(n), thr)).tolist()
        assert rows["draw16"] == want and rows["var"] == want
