"""bench.py --dump-outputs off the GPU: read_outputs over a stand-in solver (the arrays a caller
of the timed loop receives, as 0/1 float32 and float64 statistics), whole below
bench.DUMP_MAX_ELEMS and otherwise a fixed sample that is the same in every run."""
import os

import numpy as np

import bench


class FakeSolver:
    def __init__(self, n, m, seed):
        rng = np.random.default_rng(seed)
        self.n, self.m = n, m
        self.a = rng.integers(0, 2, n).astype(np.uint8)
        self.v = rng.integers(0, 2, m).astype(np.uint8)
        self.in_mis = self.v & rng.integers(0, 2, m).astype(np.uint8)

    def stats(self):
        return {"n_iterations": 7, "n_resamples": 2**40 + 1, "sum_mis_size": 33, "avg_mis_size": 4,
                "n_violated": int(self.v.sum()), "solved": 0, "lfmis_rounds_max": 3}

    def assignment_words(self):
        return np.packbits(np.pad(self.a, (0, -self.n % 32)), bitorder="little").view(np.uint32)

    def violated_mask(self):
        return np.packbits(np.pad(self.v, (0, -self.m % 64)), bitorder="little").view(np.uint64)

    def mis(self):
        return np.flatnonzero(self.in_mis).astype(np.uint32)


def test_outputs_whole_below_the_cap():
    s = FakeSolver(1001, 4099, 1)  # neither a multiple of the 32- and 64-bit words
    o = bench.read_outputs(s, s.n, s.m)
    assert sorted(o) == ["assignment", "mis", "stats", "violated"]
    assert o["stats"].dtype == np.float64
    assert o["stats"].tolist() == [7, 2**40 + 1, 33, 4, int(s.v.sum()), 0]
    for name, want in (("assignment", s.a), ("violated", s.v), ("mis", s.in_mis)):
        assert o[name].dtype == np.float32
        np.testing.assert_array_equal(o[name], want.astype(np.float32), err_msg=name)


def test_outputs_fixed_sample_above_the_cap(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 500)
    s = FakeSolver(400, 4099, 2)  # the assignment stays whole, the clause arrays are sampled
    o = bench.read_outputs(s, s.n, s.m)
    np.testing.assert_array_equal(o["assignment"], s.a.astype(np.float32))
    idx = np.sort(np.random.default_rng([bench.DUMP_SAMPLE_SEED, 1]).integers(0, s.m, 500))
    assert o["violated"].shape == o["mis"].shape == (500,)
    np.testing.assert_array_equal(o["violated"], s.v[idx].astype(np.float32))
    np.testing.assert_array_equal(o["mis"], s.in_mis[idx].astype(np.float32))  # the same clauses
    again = bench.read_outputs(s, s.n, s.m)
    for name in o:
        np.testing.assert_array_equal(o[name], again[name], err_msg=name)
    bench.dump_outputs(o, str(tmp_path / "d" / "e"))
    assert sorted(os.listdir(tmp_path / "d" / "e")) == ["assignment.npy", "mis.npy", "stats.npy", "violated.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "e" / "mis.npy"), o["mis"])


def test_dump_stays_below_64_mb_at_every_config():
    for name, (n, m, *_rest) in bench.CONFIGS.items():
        size = 4 * (min(n, bench.DUMP_MAX_ELEMS) + 2 * min(m, bench.DUMP_MAX_ELEMS)) + 8 * 6 + 4 * 128
        assert size <= 64_000_000, name
