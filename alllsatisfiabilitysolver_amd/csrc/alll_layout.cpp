// alll_layout.cpp -- the host-only layout planner of alll_create (alll_layout.h).  A solve's
// results do not depend on perm, the windows, the packed ids, the bucket widths or the skew test
// (the violated set is a set, the LFMIS priorities are clause ids): tests/test_layout.py checks them.
#include "alll_layout.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <sched.h>
#include <thread>

namespace alll {

namespace {

int fail(Layout& l, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    l.err = buf;
    return code;
}

// Runs f(i) for i in [0, n) on up to nt threads (contiguous blocks of indices).
template <typename F>
void parallel_for(uint64_t n, unsigned nt, F f) {
    nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt, n / 4096 + 1));
    if (nt <= 1) { for (uint64_t i = 0; i < n; ++i) f(i); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] { for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) f(i); });
    for (auto& x : th) x.join();
}

// f(t, begin, end) on up to nt threads over contiguous blocks of [0, n); returns the threads used
template <typename F>
unsigned parallel_chunks(uint64_t n, unsigned nt, F f) {
    nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt, n / 65536 + 1));
    if (nt <= 1) { f(0u, (uint64_t)0, n); return 1; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t] { f(t, n * t / nt, n * (t + 1) / nt); });
    for (auto& x : th) x.join();
    return nt;
}

// std::sort of a[0, n) on nt threads: sorted blocks, then pairwise merges level by level.
template <typename T, typename Cmp>
void parallel_sort(T* a, size_t n, Cmp cmp, unsigned nt) {
    if (nt <= 1 || n < (1u << 16)) { std::sort(a, a + n, cmp); return; }
    std::vector<size_t> cut(nt + 1);
    for (unsigned i = 0; i <= nt; ++i) cut[i] = n * i / nt;
    {
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; ++i) th.emplace_back([&, i] { std::sort(a + cut[i], a + cut[i + 1], cmp); });
        for (auto& x : th) x.join();
    }
    for (unsigned w = 1; w < nt; w *= 2) {
        std::vector<std::thread> th;
        for (unsigned i = 0; i + w < nt; i += 2 * w)
            th.emplace_back([&, i, w] { std::inplace_merge(a + cut[i], a + cut[i + w], a + cut[std::min(i + 2 * w, nt)], cmp); });
        for (auto& x : th) x.join();
    }
}

// ---- what the two evaluation orders share

// perm: the identity outside the own shard (the other ranks' shards keep clause order: their
// violated lists come from the all-gathered clause-order mask), the own shard's clauses sorted
// by key_of(clause) under less (Key carries the clause in .id)
template <typename Key, typename KeyOf, typename Less>
void sort_own_shard(Layout& l, KeyOf key_of, Less less) {
    const unsigned nt = host_threads();
    std::vector<uint32_t>& perm = l.perm;
    perm.resize(l.m);
    parallel_for(l.m, nt, [&](uint64_t i) { perm[i] = (uint32_t)i; });
    const uint64_t cb0 = l.own_c0;
    if (l.own_c1 <= cb0) return;
    std::vector<Key> kv(l.own_c1 - cb0);
    parallel_for(kv.size(), nt, [&](uint64_t i) { kv[i] = key_of(cb0 + i); });
    parallel_sort(kv.data(), kv.size(), less, nt);
    parallel_for(kv.size(), nt, [&](uint64_t i) { perm[cb0 + i] = kv[i].id; });
}

// Windows (instances with more than win_vars variables; ALLL_EVAL_WINDOWS=0/1 overrides): the
// evaluation's LDS holds win_vars consecutive variables; clauses are first grouped by the block
// of their smallest variable and each tile's LDS window starts at its block, so the smallest
// variable (looked up by every clause) is an LDS hit.
bool use_windows(const Knobs& kn, const Layout& l) {
    return kn.eval_windows >= 0 ? kn.eval_windows != 0 : l.n_vars > (uint64_t)l.b.win_words * 32;
}

// smallest variable of literals [j0, j1) (~0u: none)
uint32_t min_var(const uint32_t* lits, uint64_t j0, uint64_t j1) {
    uint32_t lo = ~0u;
    for (uint64_t j = j0; j < j1; ++j) lo = std::min(lo, lits[j] >> 1);
    return lo;
}

// LDS window of every own tile: the block of its first clause's smallest variable (an empty
// clause counts as variable 0); clause cl's literals are [begin(cl), begin(cl + 1))
template <typename Begin>
void first_clause_windows(const alll_problem& prob, Layout& l, Begin begin) {
    const uint64_t win_vars = (uint64_t)l.b.win_words * 32;
    const uint32_t lds_words = std::min<uint32_t>(l.b.n_words, l.b.win_words);
    l.win_base.assign(l.b.n_tiles, 0u);
    for (uint32_t tt = l.b.own_begin; tt < l.b.own_end; ++tt) {
        const uint64_t p = (uint64_t)tt * TILE;
        if (p >= l.m) break;
        const uint64_t cl = l.perm[p];
        uint32_t lo = min_var(prob.literals, begin(cl), begin(cl + 1));
        if (lo == ~0u) lo = 0;
        l.win_base[tt] = std::min<uint64_t>((uint64_t)(lo / win_vars) * l.b.win_words, l.b.n_words - lds_words);
    }
}

// ---- stages of plan_instance

// offsets monotone from 0, the 2^32 limits, the common width (the reference has UB here: Clause.h:40)
int check_offsets(const alll_problem& prob, unsigned hnt, Layout& l) {
    const uint64_t m = prob.n_clauses;
    if (m && (!prob.offsets)) return fail(l, ALLL_ERR_INVALID_ARG, "null offsets");
    if (m >= 0xFFFFFFFFull - TILE) return fail(l, ALLL_ERR_UNSUPPORTED, "more than 2^32-4097 clauses");
    const uint64_t L = m ? prob.offsets[m] : 0;
    if (m && prob.offsets[0] != 0) return fail(l, ALLL_ERR_BAD_INPUT, "offsets[0] != 0");
    if (L && !prob.literals) return fail(l, ALLL_ERR_INVALID_ARG, "null literals");
    if (L >= 0xFFFFFFFFull) return fail(l, ALLL_ERR_UNSUPPORTED, "more than 2^32-1 literals");
    l.m = m;
    l.n_lits = L;
    l.n_vars = prob.n_vars;
    if (!m) return ALLL_OK;
    const uint64_t w0 = prob.offsets[1] - prob.offsets[0];
    std::vector<uint64_t> bad(hnt, ~0ull);
    std::vector<uint8_t> ragged(hnt, 0);
    parallel_chunks(m, hnt, [&](unsigned t, uint64_t c0, uint64_t c1) {
        for (uint64_t c = c0; c < c1; ++c) {
            if (prob.offsets[c + 1] < prob.offsets[c]) { bad[t] = c; return; }
            if (prob.offsets[c + 1] - prob.offsets[c] != w0) ragged[t] = 1;
        }
    });
    const uint64_t first_bad = *std::min_element(bad.begin(), bad.end());
    if (first_bad != ~0ull) return fail(l, ALLL_ERR_BAD_INPUT, "offsets decrease at %llu", (unsigned long long)first_bad);
    l.width = *std::max_element(ragged.begin(), ragged.end()) ? 0 : (int)std::min<uint64_t>(w0, 1 << 30);
    return ALLL_OK;
}

// what the modes of opt refuse, and the round robin's chunk starts
int check_modes(const alll_problem& prob, const alll_options& opt, Layout& l) {
    const uint64_t m = l.m;
    // the round-robin MIS of T > 1 chunks (the reference's n_threads > 1) walks clause-order
    // lists of violated clauses: fixed widths keep the hybrid evaluation, whose lists are turned
    // into clause-order flags (k_rr_mark); ragged widths the CSR evaluation
    const uint32_t T = (opt.n_threads > 1 && !(opt.flags & ALLL_FLAG_LFMIS)) ? (uint32_t)opt.n_threads : 0u;
    l.b.rr_T = opt.stream_batch ? 0u : T;
    if (l.b.rr_T > RR_TMAX) return fail(l, ALLL_ERR_UNSUPPORTED, "n_threads %u > %u chunks", l.b.rr_T, RR_TMAX);
    // the streaming solve with n_threads > 1: T clause generators and the per-batch round robin
    // (SATInstance.h:70-153)
    l.b.srr_T = opt.stream_batch ? T : 0u;
    if (l.b.srr_T) {
        if (l.b.srr_T > RR_TMAX) return fail(l, ALLL_ERR_UNSUPPORTED, "streaming solve: n_threads %u > %u", l.b.srr_T, RR_TMAX);
        if (opt.world > 1) return fail(l, ALLL_ERR_UNSUPPORTED, "streaming solve with n_threads > 1 runs on one GPU");
        // an empty clause is violated forever and, sharing no variable, joins the MIS at every batch
        // step; the reference never returns on it (as with one thread), and here its repeats past the
        // materialised steps would be miscounted: refused
        for (uint64_t c = 0; c < m; ++c)
            if (prob.offsets[c + 1] == prob.offsets[c])
                return fail(l, ALLL_ERR_UNSUPPORTED, "streaming solve with n_threads > 1: clause %llu is empty",
                            (unsigned long long)c);
    }
    // the reference's own random stream (ALLL_FLAG_REFERENCE_RNG, alll_refrng.hip): defined for the
    // one-thread loop on one GPU (the reference's T > 1 resample draws from T engines inside a
    // schedule(dynamic) loop, so its bits follow the thread timing)
    l.refrng = (opt.flags & ALLL_FLAG_REFERENCE_RNG) != 0;
    for (int i = 0; i < 128; ++i) l.zero_id &= opt.comm_id[i] == 0;
    if (l.refrng) {
        if (opt.n_threads > 1)
            return fail(l, ALLL_ERR_UNSUPPORTED, "reference-RNG mode: n_threads must be 1 (the reference's T > 1 "
                                                 "resample draws from T engines in a schedule(dynamic) loop)");
        if (opt.world > 1 || !l.zero_id || (opt.flags & ALLL_FLAG_EXCHANGE_ALLREDUCE))
            return fail(l, ALLL_ERR_UNSUPPORTED, "reference-RNG mode runs on one GPU without the exchange path");
    }
    if (!l.b.rr_T) return ALLL_OK;
    l.rr_sets.resize(l.b.rr_T + 1);
    if (opt.set_starts) {
        if (opt.set_starts[0] != 0 || opt.set_starts[l.b.rr_T] != m)
            return fail(l, ALLL_ERR_INVALID_ARG, "set_starts must run from 0 to n_clauses");
        for (uint32_t q = 0; q <= l.b.rr_T; ++q) {
            if (q && opt.set_starts[q] < opt.set_starts[q - 1])
                return fail(l, ALLL_ERR_INVALID_ARG, "set_starts decrease at %u", q);
            l.rr_sets[q] = (uint32_t)opt.set_starts[q];
        }
    } else {
        // example/main.cpp:149-178: chunk_size = ceil(m / T); clause c moves to the next
        // chunk when c > (t + 1) * chunk_size, so chunk q >= 1 starts at q * chunk_size + 1
        const uint64_t chunk = (m + l.b.rr_T - 1) / l.b.rr_T;
        l.rr_sets[0] = 0;
        for (uint32_t q = 1; q <= l.b.rr_T; ++q) l.rr_sets[q] = (uint32_t)std::min<uint64_t>(m, q * chunk + 1);
        l.rr_sets[l.b.rr_T] = (uint32_t)m;
    }
    return ALLL_OK;
}

int check_literals(const alll_problem& prob, unsigned hnt, Layout& l) {
    const uint64_t lim = 2ull * prob.n_vars;
    std::vector<uint64_t> bad(hnt, ~0ull);
    parallel_chunks(l.n_lits, hnt, [&](unsigned t, uint64_t j0, uint64_t j1) {
        for (uint64_t j = j0; j < j1; ++j)
            if (prob.literals[j] >= lim) { bad[t] = j; return; }
    });
    const uint64_t j = *std::min_element(bad.begin(), bad.end());
    if (j != ~0ull)
        return fail(l, ALLL_ERR_LITERAL_RANGE, "literal %u at position %llu exceeds n_vars %u",
                    prob.literals[j], (unsigned long long)j, prob.n_vars);
    return ALLL_OK;
}

// Hot variables (skewed degree: power-law hubs): degree >= max(1024, 32 x mean degree), at most
// HOT_MAX of the highest; flagged in bit 31 of every literal copy the device uses (flag_hot)
void find_hot(const alll_problem& prob, unsigned hnt, Layout& l) {
    const uint64_t L = l.n_lits;
    if (!L || !prob.n_vars || prob.n_vars >= (1u << 30)) return;
    // degrees from per-thread 16-bit saturating histograms (4-5x faster than shared atomic
    // counters at 384M literals), exact recount for the rare saturated candidates
    const uint64_t thr = std::max<uint64_t>(HOT_THR_MIN, HOT_MEAN_X * (L / prob.n_vars + 1));
    const unsigned dnt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(hnt, (2ull << 30) / (2ull * prob.n_vars)));
    std::vector<std::vector<uint16_t>> hist(dnt);
    const unsigned used = parallel_chunks(L, dnt, [&](unsigned t, uint64_t j0, uint64_t j1) {
        std::vector<uint16_t>& h = hist[t];
        h.assign(prob.n_vars, 0);
        for (uint64_t j = j0; j < j1; ++j) {
            uint16_t& c = h[prob.literals[j] >> 1];
            c += c != 0xFFFF;
        }
    });
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> hot_t(hnt);
    std::vector<std::vector<uint32_t>> rec_t(hnt);
    parallel_chunks(prob.n_vars, hnt, [&](unsigned t, uint64_t v0, uint64_t v1) {
        for (uint64_t v = v0; v < v1; ++v) {
            uint64_t d = 0;
            bool sat = false;
            for (unsigned q = 0; q < used; ++q) { d += hist[q][v]; sat |= hist[q][v] == 0xFFFF; }
            // (a saturated count is a lower bound: such a variable is recounted exactly
            // whatever its sum, the threshold applies to exact sums only)
            if (sat) rec_t[t].push_back((uint32_t)v);
            else if (d >= thr) hot_t[t].push_back({(uint32_t)d, (uint32_t)v});
        }
    });
    hist.clear();
    std::vector<std::pair<uint32_t, uint32_t>> hot;
    std::vector<uint32_t> recount;  // (ascending: the chunks are in variable order)
    for (unsigned t = 0; t < hnt; ++t) {
        hot.insert(hot.end(), hot_t[t].begin(), hot_t[t].end());
        recount.insert(recount.end(), rec_t[t].begin(), rec_t[t].end());
    }
    if (!recount.empty()) {  // (a variable with >= 65535 literals in one thread's range)
        std::vector<uint64_t> d(recount.size(), 0);
        for (uint64_t j = 0; j < L; ++j) {
            const uint32_t v = prob.literals[j] >> 1;
            const auto it = std::lower_bound(recount.begin(), recount.end(), v);
            if (it != recount.end() && *it == v) ++d[it - recount.begin()];
        }
        for (size_t q = 0; q < recount.size(); ++q)
            if (d[q] >= thr) hot.push_back({(uint32_t)std::min<uint64_t>(d[q], 0xFFFFFFFFu), recount[q]});
    }
    if (hot.empty()) return;
    std::sort(hot.rbegin(), hot.rend());
    if (hot.size() > HOT_MAX) hot.resize(HOT_MAX);
    l.is_hot.assign(prob.n_vars, 0);
    for (auto& h : hot) l.is_hot[h.second] = 1;
    l.cv.n_hot = (uint32_t)hot.size();
}

// key of the streaming solve: position in the generator sequence j*P mod m, so the inverse of
// P mod m (P is prime, so it exists for every m < P)
int stream_inverse(Layout& l) {
    const uint64_t m = l.m;
    const uint64_t p = 9223372036854775783ull % m;
    int64_t r0 = (int64_t)m, r1 = (int64_t)p, t0 = 0, t1 = 1;
    while (r1) {
        const int64_t q = r0 / r1;
        int64_t x = r0 - q * r1; r0 = r1; r1 = x;
        x = t0 - q * t1; t0 = t1; t1 = x;
    }
    if (m > 1 && r0 != 1) return fail(l, ALLL_ERR_UNSUPPORTED, "generator step not invertible mod %llu", (unsigned long long)m);
    l.b.stream_pinv = m > 1 ? (uint64_t)((t0 % (int64_t)m + (int64_t)m) % (int64_t)m) : 0;
    return ALLL_OK;
}

// ---- stages of plan_buckets

// round robin: claimant lists by variable buckets (k_fp_bscatter / k_fp_bbuild): bucket =
// vmix(v) / width, width a multiple of 64, one bucket per CU when the width fits the LDS of
// k_fp_bbuild
int plan_claimants(const alll_problem& prob, uint32_t n_cu, Layout& l) {
    const uint64_t span = std::max<uint64_t>(l.vrange, 1);
    uint64_t width = (span + (uint64_t)n_cu - 1) / (uint64_t)n_cu;  // (two per CU: no faster)
    width = std::max<uint64_t>(1024, (width + 63) / 64 * 64);
    width = std::min<uint64_t>(width, 12288);
    uint64_t nb = (span + width - 1) / width;
    if (nb > BKT_MAX) {
        width = ((span + BKT_MAX - 1) / BKT_MAX + 63) / 64 * 64;
        nb = (span + width - 1) / width;
    }
    if (fp_bbuild_lds_bytes((uint32_t)width) > 160u * 1024 - 1024)
        return fail(l, ALLL_ERR_UNSUPPORTED, "round robin: %u variables exceed the claimant buckets", l.n_vars);
    l.b.bkt_width = (uint32_t)width;
    l.b.bkt_magic = (uint32_t)((1ull << 32) / width);
    l.b.n_bkt = (uint32_t)nb;
    l.b.bkt_span = (uint32_t)span;
    std::vector<uint32_t>& soff = l.fp_soff;
    std::vector<uint32_t>& breg = l.fp_breg;
    soff.assign((size_t)l.n_vars + 1, 0u);
    breg.assign(nb + 1, 0u);
    parallel_chunks(l.n_lits, host_threads(), [&](unsigned, uint64_t j0, uint64_t j1) {
        for (uint64_t j = j0; j < j1; ++j) __atomic_fetch_add(&soff[prob.literals[j] >> 1], 1u, __ATOMIC_RELAXED);
    });
    uint32_t acc = 0;
    for (uint32_t v = 0; v < l.n_vars; ++v) {
        const uint32_t d = soff[v];
        soff[v] = acc;
        acc += d;
        breg[((uint64_t)((v * l.b.vmix_mul) & l.b.vmix_mask)) / width] += d;
    }
    soff[l.n_vars] = acc;
    acc = 0;
    for (uint64_t k = 0; k <= nb; ++k) { const uint32_t d = breg[k]; breg[k] = acc; acc += d; }
    return ALLL_OK;
}

// Bucketed LFMIS round 0 (fixed width): one bucket per CU when a bucket's minima fit in LDS
// (else ~300-1000 power-of-2 buckets), runs of up to 16 tiles
void plan_round0(const alll_problem& prob, const Knobs& kn, uint32_t n_cu, Layout& l) {
    const unsigned hnt = host_threads();
    const uint32_t n_tiles = l.b.n_tiles;
    uint32_t shift = BKT_SHIFT_MIN;
    while (shift < BKT_SHIFT_MAX && (l.vrange >> shift) > 384) ++shift;
    uint64_t width = (l.vrange + (uint64_t)n_cu - 1) / (uint64_t)n_cu;
    width = std::max<uint64_t>(width, 1u << BKT_SHIFT_MIN);
    if (width > (1u << BKT_SHIFT_MAX)) width = 1u << shift;
    const uint64_t nb = (l.vrange + width - 1) / width;
    // skewed pair load (a literal distribution whose hubs are not all flagged hot): the
    // fullest bucket's workgroup would serialise the round; such instances keep the atomic
    // claims.  Hot literals never become pairs (LDS hash + owner), and vmix spreads the
    // remaining high-degree variables of power-law instances over the buckets.
    if (nb <= BKT_MAX) {
        std::vector<std::vector<uint64_t>> lt(hnt, std::vector<uint64_t>(nb, 0));
        std::vector<uint64_t> lp(hnt, 0);
        const unsigned used = parallel_chunks(l.n_lits, hnt, [&](unsigned t, uint64_t j0, uint64_t j1) {
            for (uint64_t j = j0; j < j1; ++j) {
                const uint32_t v = prob.literals[j] >> 1;
                if (l.cv.n_hot && l.is_hot[v]) continue;
                ++lt[t][((v * l.b.vmix_mul) & l.b.vmix_mask) / width];
                ++lp[t];
            }
        });
        std::vector<uint64_t> load(nb, 0);
        uint64_t L_pairs = 0;
        for (unsigned t = 0; t < used; ++t) {
            for (uint64_t k = 0; k < nb; ++k) load[k] += lt[t][k];
            L_pairs += lp[t];
        }
        const uint64_t mx = *std::max_element(load.begin(), load.end());
        l.skewed = mx > 4 * (L_pairs / nb + 1);
    }
    // Runs: the tile range of every evaluation workgroup (min(n_tiles, CUs) of them, the
    // split of k_eval_hybrid) cut into rpw runs of at most RUN_TILES_MAX tiles, so that one
    // GPU's evaluation workgroups scatter their own runs (k_eval_hybrid `scatter`).
    const uint32_t nblk = std::min<uint32_t>(n_tiles, n_cu);
    const uint32_t wmax = (n_tiles + nblk - 1) / nblk;
    const uint32_t rpw = (wmax + RUN_TILES_MAX - 1) / RUN_TILES_MAX;
    l.run_t0.assign((size_t)nblk * rpw + 1, 0u);
    uint32_t rt = 1;
    for (uint32_t w = 0; w < nblk; ++w) {
        const uint32_t t0 = (uint32_t)((uint64_t)n_tiles * w / nblk), t1 = (uint32_t)((uint64_t)n_tiles * (w + 1) / nblk);
        for (uint32_t j = 0; j < rpw; ++j) {
            const uint32_t a0 = t0 + (t1 - t0) * j / rpw, a1 = t0 + (t1 - t0) * (j + 1) / rpw;
            l.run_t0[(size_t)w * rpw + j] = a0;
            rt = std::max(rt, a1 - a0);
        }
    }
    l.run_t0.back() = n_tiles;
    const uint64_t area = (uint64_t)nblk * rpw * rt * TILE * l.fixed_k;  // pairs
    if (nb > BKT_MAX || l.skewed || area >= (1ull << 32)) return;  // pair positions are 32-bit in k_bresolve
    l.bucketed = true;
    l.b.bkt_width = (uint32_t)width;
    l.b.bkt_magic = (uint32_t)((1ull << 32) / width);
    l.b.n_bkt = (uint32_t)nb;
    l.b.run_tiles = rt;
    l.b.n_runs = nblk * rpw;
    // below this many violated clauses the atomic round 0 is cheaper (fixed costs)
    l.bucket_min_u = kn.has_bucket_min_u ? kn.bucket_min_u : std::max<uint64_t>(65536, l.m / 64);
}

}  // namespace

Knobs read_knobs() {
    Knobs k;
    auto on = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; };
    auto tri = [](const char* name) { const char* e = getenv(name); return e ? (int)(atoi(e) != 0) : -1; };
    if (const char* e = getenv("ALLL_SMALL_U")) k.small_u = strtoull(e, nullptr, 10);
    k.fuse_scatter = on("ALLL_FUSE_SCATTER", true);
    if (const char* e = getenv("ALLL_WIN_WORDS"))  // tests: small windows on small instances
        k.win_words = std::max<uint32_t>(16, std::min<uint32_t>(LDS_WORDS, (uint32_t)std::max(0, atoi(e)))) / 8 * 8;
    k.rr_fp = on("ALLL_RR_FP", true);  // 0: every iteration is left to the batch kernels
    if (const char* e = getenv("ALLL_RR_FP_MAX"))  // tests: iterations left to k_rr_mw mid-run
        k.rr_fp_max = (uint32_t)std::max(1, std::min(250, atoi(e)));
    k.rr_inc = on("ALLL_RR_INC", true);  // 0: full passes only (tests, A/B)
    // the repair's limits (tests lower them to force the fallbacks: a pass that gives up, wide
    // rounds on small instances, barriers that time out)
    if (const char* e = getenv("ALLL_RR_REP_CAP")) k.rr_rep_cap = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("ALLL_RR_RW_MIN")) k.rr_rw_min = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("ALLL_RR_RW_TIMEOUT")) k.rr_rw_timeout = strtoull(e, nullptr, 10);
    if (const char* e = getenv("ALLL_RR_INC_AFTER")) k.rr_inc_after = (uint32_t)std::max(1, atoi(e));
    // tests: a small epoch budget, so that small instances restart their owner epochs and run out of
    // them (FP_EP_CAP_MIN: the least budget with which an iteration still makes a pass)
    if (const char* e = getenv("ALLL_RR_EP_BUDGET"))
        k.rr_ep_budget = (uint32_t)std::max<unsigned long long>(FP_EP_CAP_MIN, std::min<unsigned long long>(0x7FFFFFFFull, strtoull(e, nullptr, 10)));
    // tests: the one-set loop's first owner epoch, so that a short run reaches the end of the 32-bit epochs
    // (at least 1, the epoch create starts at and a restart goes back to)
    if (const char* e = getenv("ALLL_EPOCH0"))
        k.epoch0 = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>(0xFFFFFFFFull, strtoull(e, nullptr, 10)));
    // (test knob: fewer engine positions, so that the parallel draws run past them and the
    // one-thread chain redoes the round)
    if (const char* e = getenv("ALLL_RRNG_NMAX"))
        if (*e) k.rrng_nmax = std::max<uint64_t>(8, strtoull(e, nullptr, 10));
    if (const char* e = getenv("ALLL_BUCKET_MIN_U")) { k.has_bucket_min_u = true; k.bucket_min_u = strtoull(e, nullptr, 10); }
    k.eval_windows = tri("ALLL_EVAL_WINDOWS");
    k.packed_ids = on("ALLL_PACKED_IDS", true);  // 0 keeps positions + perm
    k.eval_nt = tri("ALLL_EVAL_NT");
    k.debug_occupancy = getenv("ALLL_DEBUG_OCCUPANCY") != nullptr;
    // tests: plan and launch as on a device of fewer compute units (one or two evaluation
    // workgroups own many tiles each: several runs per workgroup, several tile-count passes)
    if (const char* e = getenv("ALLL_PLAN_CUS")) k.plan_cus = (uint32_t)std::max(0, atoi(e));
    return k;
}

unsigned host_threads() {
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t cs;
    if (sched_getaffinity(0, sizeof cs, &cs) == 0) n = std::max(1, CPU_COUNT(&cs));
    unsigned cap = 16;
    if (const char* e = getenv("OMP_NUM_THREADS")) { const int v = atoi(e); if (v > 0) cap = (unsigned)v; }
    return std::min(n, cap);
}

int plan_instance(const alll_problem& prob, const alll_options& opt, const Knobs& kn, Layout& l) {
    // (host passes over the instance run on the process's threads: at 128M clauses / 384M
    // literals a serial pass costs ~0.5 s, and every rank of a sharded run makes them)
    const unsigned hnt = host_threads();
    int rc;
    if ((rc = check_offsets(prob, hnt, l)) || (rc = check_modes(prob, opt, l))) return rc;
    // the streaming solve keeps the clause-order (CSR) layout: its window rule needs the first
    // violated clause index, read from a clause-order bitmask
    l.fixed_k = (l.width < 1 || l.width > MAX_FIXED_K || (opt.flags & ALLL_FLAG_GENERIC_CSR) || opt.stream_batch)
                    ? 0 : l.width;
    if ((rc = check_literals(prob, hnt, l))) return rc;
    find_hot(prob, hnt, l);
    const uint64_t m = l.m;
    if (opt.stream_batch && m && !l.b.srr_T) {
        if ((rc = stream_inverse(l))) return rc;
        l.b.stream_batch = opt.stream_batch;
    }
    l.b.n_vars = l.n_vars;
    l.b.m = l.cv.m = m;
    l.b.seed = opt.seed;
    l.cv.k = (uint32_t)l.fixed_k;
    l.cv.lit_mask = 0x7FFFFFFFu;  // (bit 31: hot-variable flag)
    l.b.n_tiles = (uint32_t)((m + TILE - 1) / TILE);
    l.tiles_per_rank = std::max<uint32_t>(1, (l.b.n_tiles + opt.world - 1) / opt.world);
    l.n_tiles_padded = l.tiles_per_rank * opt.world;
    l.b.own_begin = std::min<uint32_t>(l.b.n_tiles, (uint32_t)opt.rank * l.tiles_per_rank);
    l.b.own_end = std::min<uint32_t>(l.b.n_tiles, l.b.own_begin + l.tiles_per_rank);
    l.own_c0 = std::min<uint64_t>(m, (uint64_t)l.b.own_begin * TILE);
    l.own_c1 = std::min<uint64_t>(m, (uint64_t)l.b.own_end * TILE);
    l.b.n_words = (l.n_vars + 31) / 32;
    l.b.win_words = kn.win_words;
    l.epoch0 = kn.epoch0;
    // Ragged widths, T = 1, not streaming: chunk-transposed copy for k_eval_ragged (the CSR
    // arrays stay: the LFMIS kernels read clauses by id).  ALLL_FLAG_GENERIC_CSR and
    // ALLL_FLAG_NO_RANGED keep the clause-order CSR evaluation.  (the padding literal
    // 64 * n_words must decode to an out-of-range word through the 25 word-index bits
    // k_eval_ragged extracts, and leave bit 31 clear: n_words < 2^25)
    l.ragged = !l.fixed_k && m && !l.b.rr_T && !opt.stream_batch &&
               !(opt.flags & (ALLL_FLAG_GENERIC_CSR | ALLL_FLAG_NO_RANGED)) && l.b.n_words < (1u << 25);
    if (!l.b.rr_T) return ALLL_OK;
    l.b.rr_k = (l.width >= 1 && l.width <= 8) ? (uint32_t)l.width : 0u;
    l.b.rr_mw = std::min<uint32_t>(l.b.rr_T, 64);  // k_rr_mw: one workgroup per lane group, at most 64
    // the fixpoint passes: keys {epoch | turn | entry} need >= 10 epoch bits
    auto bits_of = [](uint64_t x) { uint32_t k = 1; while (k < 64 && (x >> k)) ++k; return k; };
    const uint32_t ib = bits_of(m), tb = bits_of(m + l.b.rr_T + 1);
    l.fp = l.b.rr_T <= FP_TMAX && ib + tb + 10 <= 64 && ib <= 28 && kn.rr_fp;  // (28: the claim pairs' slot tags)
    if (!l.fp) return ALLL_OK;
    l.fp_slots = (l.width >= 1 && l.width <= 4) ? 4 : 8;
    l.b.fp_ib = ib;
    l.b.fp_tb = tb;
    l.b.fp_hot = l.cv.n_hot ? 1 : 0;
    l.b.fp_max = kn.rr_fp_max;  // passes per iteration (graph unroll)
    l.b.fp_ep_cap = kn.rr_ep_budget;
    // incremental passes on instances without hot variables
    if (l.cv.n_hot || !kn.rr_inc) return ALLL_OK;
    l.b.fp_inc = 1;
    l.b.fp_inc_after = kn.rr_inc_after;
    l.b.fp_rep_cap = kn.rr_rep_cap;
    l.b.fp_rw_min = kn.rr_rw_min;
    l.b.fp_rw_timeout = kn.rr_rw_timeout;
    return ALLL_OK;
}

int plan_buckets(const alll_problem& prob, const alll_options& opt, const Knobs& kn, uint32_t n_cu, Layout& l) {
    // skewed instances (hot variables): owner slots and round-0 buckets by vmix (alll_internal.h)
    l.b.n_cu = n_cu;
    l.vrange = l.n_vars;
    l.b.vmix_mul = 1u;
    l.b.vmix_mask = 0xFFFFFFFFu;
    if (l.cv.n_hot) {
        l.vrange = 1024;
        while (l.vrange < l.n_vars) l.vrange <<= 1;
        l.b.vmix_mul = 0x9E3779B1u;
        l.b.vmix_mask = (uint32_t)(l.vrange - 1);
    }
    uint32_t inv = l.b.vmix_mul;  // Newton iteration for the inverse mod 2^32 (odd multiplier)
    for (int it = 0; it < 5; ++it) inv *= 2u - l.b.vmix_mul * inv;
    l.b.vmix_inv = inv;
    if (l.fp) return plan_claimants(prob, n_cu, l);
    if (l.fixed_k > 0 && !l.b.rr_T && !(opt.flags & ALLL_FLAG_ATOMIC_CLAIMS) && l.b.n_tiles > 0 && l.n_vars > 0)
        plan_round0(prob, kn, n_cu, l);
    return ALLL_OK;
}

void flag_hot(const alll_problem& prob, Layout& l) {
    if (!l.cv.n_hot) return;
    l.flagged.assign(prob.literals, prob.literals + l.n_lits);
    for (auto& x : l.flagged)
        if (l.is_hot[x >> 1]) x |= 0x80000000u;
}

std::vector<uint32_t> offsets32(const alll_problem& prob) {
    const uint64_t m = prob.n_clauses;
    std::vector<uint32_t> o32(m + 1);
    for (uint64_t i = 0; i <= m; ++i) o32[i] = m ? (uint32_t)prob.offsets[i] : 0u;
    return o32;
}

// Locality order for evaluation.  Inside every shard the clauses are evaluated sorted by
// (largest, second largest) variable and each clause's literals are stored by descending
// variable, so the gathers of slot 0 (and mostly slot 1) of a wave hit a few cache lines.
// perm[p] = original id of position p.
void order_fixed(const alll_problem& prob, const Knobs& kn, Layout& l) {
    const int K = l.fixed_k;
    const uint64_t win_vars = (uint64_t)l.b.win_words * 32;
    l.windows = use_windows(kn, l);
    struct Key { uint64_t k1; uint32_t k2, id; };
    sort_own_shard<Key>(l, [&](uint64_t cl) -> Key {
        uint32_t a = 0, b2 = 0, lo = ~0u;
        for (int j = 0; j < K; ++j) {
            const uint32_t v = prob.literals[cl * K + j] >> 1;
            if (v > a) { b2 = a; a = v; }
            else if (v > b2) b2 = v;
            lo = std::min(lo, v);
        }
        const uint64_t blk = l.windows ? lo / win_vars : 0;
        return {(blk << 32) | a, b2, (uint32_t)cl};
    }, [](const Key& x, const Key& y) {
        return x.k1 != y.k1 ? x.k1 < y.k1 : (x.k2 != y.k2 ? x.k2 < y.k2 : x.id < y.id);
    });
    // Packed clause ids: when the literals leave enough bits below the hot flag, slot j of
    // every clause also carries bits [j * id_bits, (j + 1) * id_bits) of its clause id, so
    // the evaluation emits clause ids and perm is never read on the device
    // (ALLL_PACKED_IDS=0 keeps positions + perm; tuning, tests).
    const uint64_t max_lit = 2ull * std::max<uint64_t>(l.n_vars, 1) - 1;
    // (at least 6: the evaluation takes a variable's bit index from literal bits 1..5
    // without masking)
    const uint32_t lit_bits = std::max<uint32_t>(6, 64 - (uint32_t)__builtin_clzll(max_lit));
    const uint32_t spare = lit_bits < 31 ? 31 - lit_bits : 0;
    const uint32_t idb = l.m > 1 ? 64 - (uint32_t)__builtin_clzll(l.m - 1) : 1;
    const uint32_t per = (idb + K - 1) / K;
    if (per <= spare && kn.packed_ids) {
        l.cv.id_shift = lit_bits;
        l.cv.id_bits = per;
        l.cv.lit_mask = (1u << lit_bits) - 1u;
    }
    // a literal stream larger than the 256 MB Infinity Cache is read non-temporally (it
    // cannot stay cached between iterations and would evict the assignment words of the L2
    // lookups); ALLL_EVAL_NT=0/1 overrides (tuning, tests)
    const uint64_t real_chunks = (l.m + CHUNK - 1) / CHUNK;
    l.cv.lits_nt = kn.eval_nt >= 0 ? (uint32_t)kn.eval_nt : (real_chunks * CHUNK * K * 4 > (256ull << 20) ? 1u : 0u);
}

// (the own shard's chunks only: shards are tile-aligned, so they are whole chunks)
void transpose_fixed(const alll_problem& prob, Layout& l) {
    const int K = l.fixed_k;
    const uint32_t id_bits = l.cv.id_bits, id_shift = l.cv.id_shift, id_mask = id_bits ? (1u << id_bits) - 1u : 0u;
    const uint32_t* src = l.flagged.empty() ? prob.literals : l.flagged.data();
    const uint64_t g0 = l.own_c0 / CHUNK, g1 = (l.own_c1 + CHUNK - 1) / CHUNK;
    l.t_chunk0 = g0;
    std::vector<uint32_t>& t = l.lits_t;
    t.assign((g1 - g0) * CHUNK * K, 0u);
    parallel_for(l.own_c1 - l.own_c0, host_threads(), [&](uint64_t q) {
        const uint64_t p2 = l.own_c0 + q;
        uint32_t tmp[MAX_FIXED_K];
        const uint64_t cl = l.perm[p2];
        for (int j = 0; j < K; ++j) tmp[j] = src[cl * K + j];
        // by descending variable (the hot flag, bit 31, is not part of it: slot K-1 must
        // hold the smallest variable, which the tile's window and bit 31 of win_base cover)
        std::sort(tmp, tmp + K, [](uint32_t x, uint32_t y) {
            return ((x & 0x7FFFFFFFu) >> 1) > ((y & 0x7FFFFFFFu) >> 1);
        });
        const uint64_t g = p2 / CHUNK - g0, r = p2 % CHUNK;
        for (int j = 0; j < K; ++j) {
            const uint32_t idp = id_bits ? ((uint32_t)(cl >> (j * id_bits)) & id_mask) << id_shift : 0u;
            t[(g * K + j) * CHUNK + r] = tmp[j] | idp;
        }
    });
}

void window_bases(const alll_problem& prob, Layout& l) {
    if (!l.windows || !l.m) return;
    const uint64_t K = (uint64_t)l.fixed_k, m = l.m;
    first_clause_windows(prob, l, [K](uint64_t cl) { return cl * K; });
    // bit 31: every clause of the tile has its smallest variable in the window (all but
    // the tiles at block boundaries), so k_eval_hybrid reads slot K-1 from LDS only
    const uint32_t lds_words = std::min<uint32_t>(l.b.n_words, l.b.win_words);
    std::vector<uint32_t>& wb = l.win_base;
    parallel_for(l.b.own_end - l.b.own_begin, host_threads(), [&](uint64_t q) {
        const uint64_t tt = l.b.own_begin + q;
        bool all_in = true;
        for (uint64_t p = tt * TILE; p < std::min<uint64_t>(m, (tt + 1) * TILE) && all_in; ++p) {
            const uint64_t cl = l.perm[p];
            all_in = (uint32_t)(min_var(prob.literals, cl * K, (cl + 1) * K) / 32) - wb[tt] < lds_words;
        }
        if (all_in) wb[tt] |= 0x80000000u;
    });
}

// Ragged-width evaluation layout (ClauseView::rg_off, k_eval_ragged): inside every shard the
// clauses are evaluated sorted by (width, block of the smallest variable, largest variable),
// so a chunk's 256 clauses share one width and the slot-0 lookups of a wave fall on few
// lines; every clause's literals are stored by descending variable (its smallest variable,
// looked up last, lies in the tile's LDS window) and padded to its chunk's width with an
// always-false literal.  perm maps positions to clause ids (CLAIM(0) translates the
// evaluation's positions; alll_get_violated_mask reorders the bitmask on the host).
int order_ragged(const alll_problem& prob, const Knobs& kn, Layout& l) {
    const uint64_t m = l.m;
    const uint64_t* offs = prob.offsets;
    const uint32_t* lits = prob.literals;
    const uint64_t win_vars = (uint64_t)l.b.win_words * 32;
    l.windows = use_windows(kn, l);
    struct Key { uint64_t k1; uint32_t id; };
    sort_own_shard<Key>(l, [&](uint64_t cl) -> Key {
        uint32_t hi = 0;
        for (uint64_t j = offs[cl]; j < offs[cl + 1]; ++j) hi = std::max(hi, lits[j] >> 1);
        const uint32_t lo = min_var(lits, offs[cl], offs[cl + 1]);
        const uint64_t w = std::min<uint64_t>(offs[cl + 1] - offs[cl], (1u << 20) - 1);
        const uint64_t blk = (l.windows && lo != ~0u) ? std::min<uint64_t>(lo / win_vars, 1023) : 0;
        return {(w << 40) | (blk << 30) | (hi & ((1u << 30) - 1)), (uint32_t)cl};
    }, [](const Key& x, const Key& y) { return x.k1 != y.k1 ? x.k1 < y.k1 : x.id < y.id; });
    const std::vector<uint32_t>& perm = l.perm;
    // chunk widths and offsets (units of CHUNK words)
    const uint64_t n_chunks = (m + CHUNK - 1) / CHUNK;
    std::vector<uint32_t>& off = l.rg_off;
    off.assign(n_chunks + 1, 0u);
    uint64_t acc = 0;
    for (uint64_t g = 0; g < n_chunks; ++g) {
        uint64_t w = 0;
        for (uint64_t p = g * CHUNK; p < std::min<uint64_t>(m, (g + 1) * CHUNK); ++p)
            w = std::max<uint64_t>(w, offs[perm[p] + 1] - offs[perm[p]]);
        off[g] = (uint32_t)acc;
        acc += w;
        if (acc >= (1ull << 32)) return fail(l, ALLL_ERR_UNSUPPORTED, "ragged layout exceeds 2^32 chunk slots");
    }
    off[n_chunks] = (uint32_t)acc;
    if (l.b.n_words >= (1u << 25)) return fail(l, ALLL_ERR_UNSUPPORTED, "ragged layout needs n_words < 2^25");
    const uint32_t false_lit = 64u * l.b.n_words;  // variable 32 * n_words: its word is out of range
    std::vector<uint32_t>& t = l.lits_t;
    t.assign((size_t)acc * CHUNK, false_lit);
    parallel_for(l.own_c1 - l.own_c0, host_threads(), [&](uint64_t q) {
        const uint64_t p = l.own_c0 + q;
        const uint64_t cl = perm[p], g = p / CHUNK, r = p % CHUNK;
        const uint64_t w = offs[cl + 1] - offs[cl];
        std::vector<uint32_t> tmp(lits + offs[cl], lits + offs[cl] + w);
        std::sort(tmp.begin(), tmp.end(), [](uint32_t x, uint32_t y) { return (x >> 1) > (y >> 1); });
        uint32_t* dst = t.data() + (size_t)off[g] * CHUNK + r;
        for (uint64_t j = 0; j < w; ++j) dst[j * CHUNK] = tmp[j];
    });
    if (l.windows) first_clause_windows(prob, l, [offs](uint64_t cl) { return offs[cl]; });
    return ALLL_OK;
}

}  // namespace alll
