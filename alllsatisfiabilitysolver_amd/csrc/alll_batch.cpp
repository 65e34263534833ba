// alll_batch.cpp -- the host-only planner of alll_batch_create (alll_batch.h): validation,
// deduplication of shared problems, the 16-bit device image, the LDS layout.
#include "alll_batch.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <tuple>

namespace alll {

namespace {

int fail(BatchPlan& p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    p.err = buf;
    return code;
}

constexpr uint32_t VEC = 8;  // 16-bit elements per 16-byte vector
uint32_t round_up(uint32_t x, uint32_t a) { return (x + a - 1) / a * a; }

// the options a batch honours are device and max_iters; everything that selects another loop is refused
int check_options(const alll_options& opt, BatchPlan& p) {
    if (opt.n_threads != 1) return fail(p, ALLL_ERR_UNSUPPORTED, "batch: n_threads %d (only 1)", opt.n_threads);
    if (opt.world != 1) return fail(p, ALLL_ERR_UNSUPPORTED, "batch: world %d (one GPU only)", opt.world);
    if (opt.stream_batch != 0) return fail(p, ALLL_ERR_UNSUPPORTED, "batch: the streaming solve is not supported");
    if (opt.flags & ALLL_FLAG_REFERENCE_RNG)
        return fail(p, ALLL_ERR_UNSUPPORTED, "batch: ALLL_FLAG_REFERENCE_RNG (its stream is sequential in pick order)");
    if (opt.flags) return fail(p, ALLL_ERR_UNSUPPORTED, "batch: flags 0x%x (none is supported)", opt.flags);
    return ALLL_OK;
}

// sizes within the limits, offsets monotone from 0, variables in range
int check_item(const alll_problem& pr, uint64_t i, BatchPlan& p) {
    const unsigned long long ii = i;
    const uint64_t m = pr.n_clauses;
    if (pr.n_vars > ALLL_BATCH_MAX_VARS || m > ALLL_BATCH_MAX_CLAUSES)
        return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: %u variables, %llu clauses (limits %u, %u)", ii, pr.n_vars,
                    (unsigned long long)m, ALLL_BATCH_MAX_VARS, ALLL_BATCH_MAX_CLAUSES);
    if (m && !pr.offsets) return fail(p, ALLL_ERR_INVALID_ARG, "item %llu: null offsets", ii);
    if (m && pr.offsets[0] != 0) return fail(p, ALLL_ERR_BAD_INPUT, "item %llu: offsets[0] != 0", ii);
    for (uint64_t c = 0; c < m; ++c)
        if (pr.offsets[c + 1] < pr.offsets[c])
            return fail(p, ALLL_ERR_BAD_INPUT, "item %llu: offsets decrease at %llu", ii, (unsigned long long)c);
    const uint64_t L = m ? pr.offsets[m] : 0;
    if (L > ALLL_BATCH_MAX_LITERALS)
        return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: %llu literals (limit %u)", ii, (unsigned long long)L,
                    ALLL_BATCH_MAX_LITERALS);
    if (L && !pr.literals) return fail(p, ALLL_ERR_INVALID_ARG, "item %llu: null literals", ii);
    for (uint64_t j = 0; j < L; ++j)
        if ((pr.literals[j] >> 1) >= pr.n_vars)
            return fail(p, ALLL_ERR_LITERAL_RANGE, "item %llu: literal %llu names variable %u >= n_vars %u", ii,
                        (unsigned long long)j, pr.literals[j] >> 1, pr.n_vars);
    return ALLL_OK;
}

}  // namespace

bool batch_fits(uint32_t n_vars, uint64_t n_clauses, uint64_t n_literals) {
    return n_vars <= ALLL_BATCH_MAX_VARS && n_clauses <= ALLL_BATCH_MAX_CLAUSES && n_literals <= ALLL_BATCH_MAX_LITERALS;
}

SmallLds small_lds_layout(uint32_t max_vars, uint32_t max_clauses, uint32_t max_lits) {
    SmallLds l{};
    const uint32_t groups = (max_clauses + 63) / 64;
    uint32_t at = 0;
    auto take = [&](uint32_t bytes) { const uint32_t a = at; at += round_up(bytes, 16); return a; };
    l.lits = take(2 * round_up(max_lits, VEC));
    l.offs = take(2 * round_up(max_clauses + 1, VEC));
    l.vmask = take(8 * groups);
    l.claim = take(4 * max_vars);
    l.A = take(4 * ((max_vars + 31) / 32));
    l.prefix = take(4 * (groups + 1));
    l.ctl = take(4 * 8);
    l.list_stride = round_up(max_clauses, VEC);
    l.list = take(2 * 2 * l.list_stride);
    l.bytes = std::max(at, 16u);
    return l;
}

SmallLds small_lds_layout(uint32_t max_vars, uint32_t max_clauses, uint32_t max_lits, uint32_t* thr_at) {
    SmallLds l = small_lds_layout(max_vars, max_clauses, max_lits);
    *thr_at = l.bytes;  // (every array ends at a multiple of 16; never 0: the control words come before)
    l.bytes += round_up(4 * max_vars, 16);
    return l;
}

int plan_batch(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options& opt,
               BatchPlan& p) {
    if (!probs || !seeds) return fail(p, ALLL_ERR_INVALID_ARG, "batch: null argument");
    if (n_items == 0) return fail(p, ALLL_ERR_INVALID_ARG, "batch: no items");
    if (n_items >= (1ull << 31)) return fail(p, ALLL_ERR_UNSUPPORTED, "batch: %llu items (limit 2^31)", (unsigned long long)n_items);
    if (int rc = check_options(opt, p)) return rc;

    // a problem is stored once: items whose arrays are equal in pointer and size share its copy
    using Key = std::tuple<const uint64_t*, const uint32_t*, uint64_t, uint32_t>;
    std::map<Key, std::pair<uint32_t, uint32_t>> seen;  // -> {lits_at, offs_at}
    uint64_t a_words = 0;
    p.items.resize(n_items);
    for (uint64_t i = 0; i < n_items; ++i) {
        const alll_problem& pr = probs[i];
        const Key key{pr.offsets, pr.literals, pr.n_clauses, pr.n_vars};
        auto it = seen.find(key);
        const uint64_t m = pr.n_clauses;
        if (it == seen.end()) {
            if (int rc = check_item(pr, i, p)) return rc;
            const uint64_t L = m ? pr.offsets[m] : 0;
            if (p.lits.size() + L + VEC >= (1ull << 32) || p.offs.size() + m + 1 + VEC >= (1ull << 32))
                return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: the batch's problems exceed 2^32 literals", (unsigned long long)i);
            const uint32_t lits_at = (uint32_t)p.lits.size(), offs_at = (uint32_t)p.offs.size();
            p.lits.resize(lits_at + round_up((uint32_t)L, VEC), 0);
            p.offs.resize(offs_at + round_up((uint32_t)m + 1, VEC), 0);
            for (uint64_t j = 0; j < L; ++j) p.lits[lits_at + j] = (uint16_t)pr.literals[j];
            for (uint64_t c = 0; c <= m; ++c) p.offs[offs_at + c] = (uint16_t)(m ? pr.offsets[c] : 0);
            it = seen.emplace(key, std::make_pair(lits_at, offs_at)).first;
            ++p.n_problems;
        }
        SmallItem& s = p.items[i];
        s.seed = seeds[i];
        s.n_vars = pr.n_vars;
        s.n_words = (pr.n_vars + 31) / 32;
        s.m = (uint32_t)m;
        s.n_lits = m ? (uint32_t)pr.offsets[m] : 0;
        s.lits_at = it->second.first;
        s.offs_at = it->second.second;
        if (a_words + s.n_words >= (1ull << 32))
            return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: the batch's assignments exceed 2^32 words", (unsigned long long)i);
        s.a_at = (uint32_t)a_words;
        s.pad = 0;
        a_words += s.n_words;
        p.max_vars = std::max(p.max_vars, s.n_vars);
        p.max_clauses = std::max(p.max_clauses, s.m);
        p.max_lits = std::max(p.max_lits, s.n_lits);
    }
    p.a_words = (uint32_t)a_words;
    p.lds = small_lds_layout(p.max_vars, p.max_clauses, p.max_lits);
    // a wave per 256 clauses of the largest item, 1 .. 16 waves: small items keep their barriers
    // cheap and pack several workgroups per CU, an item at the limits gets 1024 threads
    p.threads = 64 * std::min<uint32_t>(16, std::max<uint32_t>(1, (p.max_clauses + 255) / 256));
    return ALLL_OK;
}

}  // namespace alll
