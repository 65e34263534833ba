"""The host-only layout planner (csrc/alll_layout.cpp) checked as a layout, without a GPU.

tests/cpp/layout_dump.cpp links the planner directly (no liballl.so, nothing loaded into
Python), is built under the address and undefined-behaviour sanitizers and writes what the
planner decided as raw arrays.  Every check below restates a rule in numpy the way the comments
of the planner state it; none compares against recorded output.  A solve's results do not
depend on any of this (perm, windows, packed ids, bucket widths, skew test), so the GPU suite
cannot see a mistake here: it would only make the loop slower."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "alllsatisfiabilitysolver_amd", "csrc")
TILE, CHUNK = 4096, 256
INVALID_ARG, BAD_INPUT, LITERAL_RANGE, UNSUPPORTED = 1, 2, 3, 10
FLAG_REFERENCE_RNG = 1 << 7
P_STREAM = 9223372036854775783


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout")
    exe = str(d / "layout_dump")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",  # (the runtimes in the program: it starts in any environment)
                        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-pthread", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "layout_dump.cpp"), os.path.join(CSRC, "alll_layout.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    count = [0]

    def run(inst, world=1, rank=0, T=1, flags=0, batch=0, n_cu=256, starts=(), raw=False, **env):
        n, offs, lits = inst
        count[0] += 1
        src, out = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        with open(src, "wb") as f:
            f.write(struct.pack("<QQ", n, len(offs) - 1))
            f.write(np.asarray(offs, dtype=np.uint64).tobytes())
            f.write(np.asarray(lits, dtype=np.uint32).tobytes())
        e = {k: v for k, v in os.environ.items() if not k.startswith("ALLL_")}
        e.update({k: str(v) for k, v in env.items()})
        r = subprocess.run([exe, str(src), str(out)] + [str(x) for x in (world, rank, T, flags, batch, n_cu, *starts)],
                           capture_output=True, text=True, env=e)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a sanitizer report ends the program)
        data = out.read_bytes()
        if raw:
            return data
        res, at = {}, 0
        while at < len(data):
            (nl,) = struct.unpack_from("<I", data, at)
            name = data[at + 4:at + 4 + nl].decode()
            esize, cnt = struct.unpack_from("<IQ", data, at + 4 + nl)
            at += 16 + nl
            a = np.frombuffer(data, dtype={1: np.uint8, 4: np.uint32, 8: np.uint64}[esize], count=cnt, offset=at)
            at += esize * cnt
            res[name] = a.tobytes().decode() if name == "err" else (int(a[0]) if esize == 8 else a)
        return res

    return run


def ksat(n, m, k, seed, lo=0):
    rng = np.random.default_rng(seed)
    lits = (2 * rng.integers(lo, n, size=m * k) + rng.integers(0, 2, size=m * k)).astype(np.uint32)
    return n, np.arange(m + 1, dtype=np.uint64) * k, lits


def planted(n, m, degrees, seed):
    """Random 3-SAT over the variables [100, n); variable v < 100 then takes degrees[v] slots."""
    n, offs, lits = ksat(n, m, 3, seed, lo=100)
    slots = np.random.default_rng(seed + 1).permutation(3 * m)
    at = 0
    for v, d in degrees.items():
        lits[slots[at:at + d]] = 2 * v + (np.arange(d) & 1)
        at += d
    return n, offs, lits


def ragged_instance(n, m, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 6, size=m)
    w[[0, 1, 2, 3, 4, 5, 777]] = [1, 2, 3, 4, 5, 0, 0]  # every width, two empty clauses
    offs = np.concatenate([[0], np.cumsum(w)]).astype(np.uint64)
    lits = (2 * rng.integers(0, n, size=int(offs[-1])) + rng.integers(0, 2, size=int(offs[-1]))).astype(np.uint32)
    return n, offs, lits


C1 = ksat(200, 800, 3, 1)
C2 = ksat(2500, 10000, 3, 2)
C5 = ragged_instance(600, 5000, 5)
C6 = planted(4000, 6000, {7: 1500, 31: 1100, 64: 1023}, 6)
C6_SAT = planted(4000, 70000, {}, 7)
C6_SAT[2][0::3] = 2 * 9 + (np.arange(70000) & 1)  # variable 9 in every clause
# half of C2's clauses inside the last, partial block of 512 variables (2048..2499): a tile starts there
C2_TOP = (C2[0], C2[1], np.where(np.arange(30000) < 15000, 2 * (2048 + (C2[2] >> 1) % 452) + (C2[2] & 1), C2[2]).astype(np.uint32))
W16 = dict(ALLL_WIN_WORDS=16)  # windows of 512 variables


def fixed_key_order(inst, c0, c1, win_vars=None):
    """perm of clauses [c0, c1): by (block of the smallest variable,) largest, second largest, id"""
    n, offs, lits = inst
    v = np.sort(lits.reshape(-1, 3) >> 1, axis=1)[c0:c1]
    ids = np.arange(c0, c1)
    keys = [ids, v[:, 1], v[:, 2]] + ([v[:, 0] // win_vars] if win_vars else [])
    return ids[np.lexsort(keys)]


def check_fixed_stream(inst, r, c0=0, c1=None, hot=None):
    """the transposed stream of positions [c0, c1): slots by descending variable, the clause's
    literals in the low bits, the packed id above them, bit 31 on the hot variables' literals"""
    n, offs, lits = inst
    m, K = len(offs) - 1, 3
    c1 = m if c1 is None else c1
    t = r["lits_t"].reshape(-1, K, CHUNK).transpose(0, 2, 1).reshape(-1, K)  # [position - first][slot]
    first = r["t_chunk0"] * CHUNK
    assert first == c0 // CHUNK * CHUNK and len(t) == -(-c1 // CHUNK) * CHUNK - first
    rows = t[c0 - first:c1 - first]
    assert not t[c1 - first:].any()
    perm = r["perm"][c0:c1].astype(np.int64)
    plain = rows & np.uint32(r["lit_mask"])
    assert (np.diff((plain >> 1).astype(np.int64), axis=1) <= 0).all()
    assert np.array_equal(np.sort(plain, axis=1), np.sort(lits.reshape(-1, K)[perm], axis=1))
    is_hot = np.zeros(n, dtype=bool) if hot is None else hot
    assert np.array_equal(rows >> 31 != 0, is_hot[plain >> 1])
    if r["id_bits"]:
        ids = (rows.astype(np.int64) >> r["id_shift"]) & ((1 << r["id_bits"]) - 1)
        assert np.array_equal(sum(ids[:, j] << (j * r["id_bits"]) for j in range(K)), perm)
    else:
        assert np.array_equal(rows & np.uint32(0x7FFFFFFF), plain)


def test_fixed_order_and_packed_ids(dump):
    r = dump(C1)
    assert (r["rc"], r["fixed_k"], r["windows"]) == (0, 3, 0)
    assert np.array_equal(r["perm"], fixed_key_order(C1, 0, 800))
    # 400 literal values: 9 bits; 800 ids: 10 bits over 3 slots
    assert (r["id_shift"], r["id_bits"], r["lit_mask"]) == (9, 4, 511)
    check_fixed_stream(C1, r)


def test_fixed_without_packed_ids(dump):
    r = dump(C1, ALLL_PACKED_IDS=0)
    assert (r["id_bits"], r["id_shift"], r["lit_mask"]) == (0, 0, 0x7FFFFFFF)
    assert np.array_equal(r["perm"], fixed_key_order(C1, 0, 800))  # (the device reads perm: it is uploaded)
    check_fixed_stream(C1, r)


def check_windows(inst, r, t0, t1, win_words=16):
    n, offs, lits = inst
    m = len(offs) - 1
    lo = (lits.reshape(-1, 3) >> 1).min(axis=1)[r["perm"].astype(np.int64)]
    wb = r["win_base"]
    assert len(wb) == r["n_tiles"]
    for t in range(r["n_tiles"]):
        if not t0 <= t < t1:
            assert wb[t] == 0
            continue
        base = min(int(lo[t * TILE]) // (32 * win_words) * win_words, r["n_words"] - win_words)
        assert wb[t] & 0x7FFFFFFF == base
        words = lo[t * TILE:min(m, (t + 1) * TILE)] // 32
        assert bool(wb[t] >> 31) == bool(((words >= base) & (words < base + win_words)).all())


def test_windows(dump):
    r = dump(C2, **W16)
    assert (r["windows"], r["n_tiles"], r["win_words"], r["n_words"]) == (1, 3, 16, 79)
    assert np.array_equal(r["perm"], fixed_key_order(C2, 0, 10000, win_vars=512))
    check_windows(C2, r, 0, 3)
    assert len({int(w) >> 31 for w in r["win_base"]}) == 2  # both kinds of tile occur
    check_fixed_stream(C2, r)
    # a window that would end past the assignment starts at n_words - win_words instead
    r = dump(C2_TOP, **W16)
    assert np.array_equal(r["perm"], fixed_key_order(C2_TOP, 0, 10000, win_vars=512))
    check_windows(C2_TOP, r, 0, 3)
    assert r["win_base"][2] == 0x80000000 | (79 - 16)
    r = dump(C2, ALLL_EVAL_WINDOWS=0, **W16)
    assert r["windows"] == 0 and len(r["win_base"]) == 0
    assert np.array_equal(r["perm"], fixed_key_order(C2, 0, 10000))


def test_own_shard_only(dump):
    r = dump(C2, world=3, rank=1, **W16)
    assert (r["own_begin"], r["own_end"]) == (1, 2)
    perm = r["perm"]
    assert np.array_equal(perm[:4096], np.arange(4096)) and np.array_equal(perm[8192:], np.arange(8192, 10000))
    assert np.array_equal(perm[4096:8192], fixed_key_order(C2, 4096, 8192, win_vars=512))
    check_fixed_stream(C2, r, 4096, 8192)
    check_windows(C2, r, 1, 2)


def test_ragged_order(dump):
    n, offs, lits = C5
    m = len(offs) - 1
    r = dump(C5, ALLL_EVAL_WINDOWS=1, **W16)
    assert (r["rc"], r["fixed_k"], r["ragged"], r["windows"], r["n_words"]) == (0, 0, 1, 1, 19)
    o = offs.astype(np.int64)
    w = np.diff(o)
    cl = [lits[o[c]:o[c + 1]] >> 1 for c in range(m)]
    hi = np.array([c.max() if len(c) else 0 for c in cl])
    lo = np.array([c.min() if len(c) else 0 for c in cl])  # (an empty clause: block 0, window 0)
    perm = np.lexsort((np.arange(m), hi, lo // 512, w))
    assert np.array_equal(r["perm"], perm) and w[perm[0]] == 0
    n_chunks = -(-m // CHUNK)
    wmax = np.array([w[perm[g * CHUNK:(g + 1) * CHUNK]].max() for g in range(n_chunks)])
    off = np.concatenate([[0], np.cumsum(wmax)])
    assert np.array_equal(r["rg_off"], off)
    t = r["lits_t"]
    assert len(t) == off[-1] * CHUNK
    pad = 64 * 19
    for p in range(n_chunks * CHUNK):
        g, row = divmod(p, CHUNK)
        col = t[off[g] * CHUNK + row:off[g + 1] * CHUNK:CHUNK]
        k = w[perm[p]] if p < m else 0
        assert (col[k:] == pad).all()
        if k:
            assert (np.diff((col[:k] >> 1).astype(np.int64)) <= 0).all()
            assert np.array_equal(np.sort(col[:k]), np.sort(lits[o[perm[p]]:o[perm[p] + 1]]))
    assert list(r["win_base"]) == [min(int(lo[perm[t0 * TILE]]) // 512 * 16, 19 - 16) for t0 in range(2)]


def test_hot_variables(dump):
    n, offs, lits = C6
    r = dump(C6)
    hot = np.zeros(n, dtype=bool)
    hot[[7, 31]] = True  # threshold max(1024, 32 * (18000 // 4000 + 1)): degree 1023 stays cold
    assert r["n_hot"] == 2 and np.array_equal(r["is_hot"] != 0, hot)
    assert np.array_equal(r["flagged"], lits | (hot[lits >> 1].astype(np.uint32) << 31))
    check_fixed_stream(C6, r, hot=hot)
    assert (r["vmix_mul"], r["vmix_mask"], r["vrange"]) == (0x9E3779B1, 4095, 4096)
    assert r["vmix_inv"] * r["vmix_mul"] % 2**32 == 1
    # one thread's 16-bit count saturates at 65535: the exact recount still finds the variable
    r = dump(C6_SAT, OMP_NUM_THREADS=1)
    assert r["n_hot"] == 1 and list(np.flatnonzero(r["is_hot"])) == [9]
    r = dump(C1)
    assert (r["n_hot"], len(r["is_hot"]), r["vmix_mul"], r["vmix_mask"], r["vmix_inv"]) == (0, 0, 1, 0xFFFFFFFF, 1)


def check_runs(r, n_cu):
    rt = r["run_t0"].astype(np.int64)
    assert rt[0] == 0 and rt[-1] == r["n_tiles"] and (np.diff(rt) >= 0).all() and np.diff(rt).max() <= 16
    assert len(rt) == r["n_runs"] + 1 and r["n_runs"] % min(r["n_tiles"], n_cu) == 0
    assert r["run_tiles"] == np.diff(rt).max()


def test_round0_bucket_plan(dump):
    r = dump(C1)  # 200 variables: one bucket of the smallest width
    assert (r["bucketed"], r["skewed"], r["bkt_width"], r["n_bkt"]) == (1, 0, 1024, 1)
    check_runs(r, 256)
    big = ksat(300000, 40000, 3, 8)
    r = dump(big)  # a bucket per CU: ceil(300000 / 256) variables each
    assert (r["bucketed"], r["skewed"], r["bkt_width"], r["n_bkt"]) == (1, 0, 1172, 256)
    assert r["bkt_magic"] == 2**32 // 1172 and r["bucket_min_u"] == 65536
    check_runs(r, 256)
    r = dump(C6_SAT, n_cu=1)  # 18 tiles on one workgroup: two runs
    assert r["n_runs"] == 2
    check_runs(r, 1)
    # every literal in the first bucket: skewed, so no bucket plan (and no pair buffers)
    r = dump((300000, big[1], (2 * ((big[2] >> 1) % 1000) + (big[2] & 1)).astype(np.uint32)))
    assert (r["bucketed"], r["skewed"], r["n_runs"], r["run_tiles"], r["n_bkt"]) == (0, 1, 0, 0, 0)


def reference_chunk_starts(m, T):
    """example/main.cpp:149-178: clause c moves to the next chunk when c > (t + 1) * chunk_size"""
    chunk, t, owner = -(-m // T), 0, []
    for c in range(m):
        if c > (t + 1) * chunk:
            t += 1
        owner.append(t)
    return [sum(o < q for o in owner) for q in range(T)] + [m]


@pytest.mark.parametrize("m,T", [(10, 3), (800, 16), (7, 8)])
def test_round_robin_chunk_starts(dump, m, T):
    r = dump(ksat(50, m, 3, 3), T=T)
    assert r["rr_T"] == T and list(r["rr_sets"]) == reference_chunk_starts(m, T)


def test_round_robin_explicit_starts(dump):
    r = dump(C1, T=3, starts=(0, 100, 100, 800))
    assert list(r["rr_sets"]) == [0, 100, 100, 800]
    r = dump(C1, T=3, starts=(0, 200, 100, 800))
    assert r["rc"] == INVALID_ARG and r["err"] == "set_starts decrease at 2"
    r = dump(C1, T=3, starts=(0, 100, 200, 799))
    assert r["rc"] == INVALID_ARG and r["err"] == "set_starts must run from 0 to n_clauses"


@pytest.mark.parametrize("inst,mask,n_bkt", [(C2, 0xFFFFFFFF, 3), (C6, 4095, 4)], ids=["plain", "vmix"])
def test_round_robin_claimant_buckets(dump, inst, mask, n_bkt):
    n, offs, lits = inst
    r = dump(inst, T=4)
    assert (r["fp"], r["bkt_width"], r["n_bkt"], r["vmix_mask"]) == (1, 1024, n_bkt, mask)
    assert r["bkt_span"] == (n if mask == 0xFFFFFFFF else 4096)
    deg = np.bincount(lits >> 1, minlength=n)
    assert np.array_equal(r["fp_soff"], np.concatenate([[0], np.cumsum(deg)]))
    bucket = ((np.arange(n, dtype=np.uint64) * np.uint64(r["vmix_mul"])) & np.uint64(r["vmix_mask"] & 0xFFFFFFFF)) // 1024
    per = np.bincount(bucket.astype(np.int64), weights=deg, minlength=n_bkt).astype(np.int64)
    assert np.array_equal(r["fp_breg"], np.concatenate([[0], np.cumsum(per)]))


def test_epoch_knobs_reach_the_plan(dump):
    """ALLL_RR_EP_BUDGET caps the round robin's epoch budget (LoopBuffers::fp_ep_cap), clamped from
    below to 2 (FP_G_MAX + 2) and from above to the key layout's 2^31 - 1; ALLL_EPOCH0 is the one-set
    loop's first owner epoch (32-bit, at least 1).  Unset: no cap, and create's start at epoch 1."""
    r = dump(C2, T=4)
    assert (r["fp"], r["fp_ep_cap"], r["epoch0"]) == (1, 0, 1)
    assert r["fp_ep_cap_min"] == 2 * (r["fp_g_max"] + 2) == 16
    for given, want in ((4096, 4096), (17, 17), (16, 16), (15, 16), (1, 16), (0, 16), (2**31 - 1, 2**31 - 1),
                        (2**31, 2**31 - 1), (2**40, 2**31 - 1)):
        assert dump(C2, T=4, ALLL_RR_EP_BUDGET=given)["fp_ep_cap"] == want, given
    # (the one-set loop and the batch kernel alone have no claim keys to budget: the cap stays 0)
    assert dump(C2, ALLL_RR_EP_BUDGET=64)["fp_ep_cap"] == 0
    assert dump(C2, T=4, ALLL_RR_FP=0, ALLL_RR_EP_BUDGET=64)["fp_ep_cap"] == 0
    for given, want in ((1, 1), (0, 1), (2**31, 2**31), (2**32 - 3, 2**32 - 3), (2**32 - 1, 2**32 - 1), (2**32, 2**32 - 1),
                        (2**40, 2**32 - 1)):
        for T in (1, 4):
            assert dump(C2, T=T, ALLL_EPOCH0=given)["epoch0"] == want, (given, T)
    assert dump(C2, ALLL_EPOCH0=77, ALLL_RR_EP_BUDGET=99)["epoch0"] == 77


@pytest.mark.parametrize("m", [1, 2, 3, 800, 2**20])
def test_streaming_inverse(dump, m):
    r = dump(ksat(64, m, 1, 4), batch=64)
    assert r["rc"] == 0 and r["fixed_k"] == 0 and r["ragged"] == 0
    assert r["stream_pinv"] == 0 if m == 1 else (P_STREAM % m) * r["stream_pinv"] % m == 1


@pytest.mark.parametrize("inst,env", [(C2, W16), (C5, dict(ALLL_EVAL_WINDOWS=1, **W16)), (C6, {}), (C6_SAT, {})],
                         ids=["windows", "ragged", "hot", "parallel-sort"])
def test_thread_independence(dump, inst, env):
    assert dump(inst, raw=True, OMP_NUM_THREADS=1, **env) == dump(inst, raw=True, OMP_NUM_THREADS=7, **env)


def test_validation(dump):
    n, offs, lits = C1
    bad = offs.copy()
    bad[5] = 1
    r = dump((n, bad, lits))
    assert (r["rc"], r["err"]) == (BAD_INPUT, "offsets decrease at 4")
    bad = offs.copy()
    bad[0] = 1
    r = dump((n, bad, lits))
    assert (r["rc"], r["err"]) == (BAD_INPUT, "offsets[0] != 0")
    bad = lits.copy()
    bad[77] = 400
    r = dump((n, offs, bad))
    assert (r["rc"], r["err"]) == (LITERAL_RANGE, "literal 400 at position 77 exceeds n_vars 200")
    r = dump(C5, T=3, batch=64)
    assert (r["rc"], r["err"]) == (UNSUPPORTED, "streaming solve with n_threads > 1: clause 5 is empty")
    r = dump(C1, T=2, flags=FLAG_REFERENCE_RNG)
    assert r["rc"] == UNSUPPORTED and r["err"].startswith("reference-RNG mode: n_threads must be 1")
