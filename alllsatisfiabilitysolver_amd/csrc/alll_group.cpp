// alll_group.cpp -- the host-only planner of alll_group_create (alll_group.h): validation, the
// items' places in the block-diagonal union, the union's CSR with shifted literals, the per-word
// table of the keyed random stream.
#include "alll_group.h"

#include <cstdarg>
#include <cstdio>

namespace alll {

namespace {

int fail(GroupPlan& p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    p.err = buf;
    return code;
}

// the union's limits are the loop's own: 32-bit clause ids with a tile to spare,
// 32-bit literal positions, literals of 31 bits (bit 31 of a device literal flags a hot variable)
constexpr uint64_t MAX_CLAUSES = 0xFFFFFFFFull - 4096;  // n_clauses < this
constexpr uint64_t MAX_LITERALS = 0xFFFFFFFFull;        // n_literals < this
constexpr uint64_t MAX_WORDS = 1ull << 25;              // words <= this: 2^30 variables

// everything that selects another loop or another random stream is refused; the flags that do
// not change results (NO_GRAPH, GENERIC_CSR, NO_RANGED, KERNEL_TIMING, ATOMIC_CLAIMS) pass
int check_options(const alll_options& opt, GroupPlan& p) {
    if (opt.n_threads != 1) return fail(p, ALLL_ERR_UNSUPPORTED, "group: n_threads %d (only 1)", opt.n_threads);
    if (opt.world != 1) return fail(p, ALLL_ERR_UNSUPPORTED, "group: world %d (one GPU only)", opt.world);
    if (opt.stream_batch != 0) return fail(p, ALLL_ERR_UNSUPPORTED, "group: the streaming solve is not supported");
    for (int i = 0; i < 128; ++i)
        if (opt.comm_id[i]) return fail(p, ALLL_ERR_UNSUPPORTED, "group: a communicator id (no exchange path)");
    if (opt.flags & ALLL_FLAG_REFERENCE_RNG)
        return fail(p, ALLL_ERR_UNSUPPORTED, "group: ALLL_FLAG_REFERENCE_RNG (its stream is sequential in pick order)");
    if (opt.flags & ALLL_FLAG_LFMIS) return fail(p, ALLL_ERR_UNSUPPORTED, "group: ALLL_FLAG_LFMIS (n_threads is 1)");
    if (opt.flags & ALLL_FLAG_EXCHANGE_ALLREDUCE)
        return fail(p, ALLL_ERR_UNSUPPORTED, "group: ALLL_FLAG_EXCHANGE_ALLREDUCE (no exchange path)");
    const uint32_t known = ALLL_FLAG_NO_GRAPH | ALLL_FLAG_GENERIC_CSR | ALLL_FLAG_NO_RANGED | ALLL_FLAG_KERNEL_TIMING |
                           ALLL_FLAG_ATOMIC_CLAIMS;
    if (opt.flags & ~known) return fail(p, ALLL_ERR_UNSUPPORTED, "group: flags 0x%x", opt.flags & ~known);
    return ALLL_OK;
}

// offsets monotone from 0, variables in range (the codes of alll_create's validation)
int check_item(const alll_problem& pr, uint64_t i, GroupPlan& p) {
    const unsigned long long ii = i;
    const uint64_t m = pr.n_clauses;
    if (m && !pr.offsets) return fail(p, ALLL_ERR_INVALID_ARG, "item %llu: null offsets", ii);
    if (m >= MAX_CLAUSES) return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: more than 2^32-4097 clauses", ii);
    if (m && pr.offsets[0] != 0) return fail(p, ALLL_ERR_BAD_INPUT, "item %llu: offsets[0] != 0", ii);
    for (uint64_t c = 0; c < m; ++c)
        if (pr.offsets[c + 1] < pr.offsets[c])
            return fail(p, ALLL_ERR_BAD_INPUT, "item %llu: offsets decrease at %llu", ii, (unsigned long long)c);
    const uint64_t L = m ? pr.offsets[m] : 0;
    if (L && !pr.literals) return fail(p, ALLL_ERR_INVALID_ARG, "item %llu: null literals", ii);
    if (L >= MAX_LITERALS) return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: more than 2^32-1 literals", ii);
    const uint64_t lim = 2ull * pr.n_vars;
    for (uint64_t j = 0; j < L; ++j)
        if (pr.literals[j] >= lim)
            return fail(p, ALLL_ERR_LITERAL_RANGE, "item %llu: literal %u at position %llu exceeds n_vars %u", ii,
                        pr.literals[j], (unsigned long long)j, pr.n_vars);
    return ALLL_OK;
}

}  // namespace

int plan_group(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options& opt,
               GroupPlan& p) {
    if (!probs || !seeds) return fail(p, ALLL_ERR_INVALID_ARG, "group: null argument");
    if (n_items == 0) return fail(p, ALLL_ERR_INVALID_ARG, "group: no items");
    if (n_items >= (1ull << 31)) return fail(p, ALLL_ERR_UNSUPPORTED, "group: %llu items (limit 2^31)", (unsigned long long)n_items);
    if (int rc = check_options(opt, p)) return rc;

    // ---- every item, then its place: a new assignment word, the next clause, the next literal
    uint64_t words = 0, clauses = 0, lits = 0;
    p.items.resize(n_items);
    p.clause_base.resize(n_items + 1);
    for (uint64_t i = 0; i < n_items; ++i) {
        const alll_problem& pr = probs[i];
        if (int rc = check_item(pr, i, p)) return rc;
        const uint64_t m = pr.n_clauses, L = m ? pr.offsets[m] : 0;
        const uint64_t nw = ((uint64_t)pr.n_vars + 31) / 32;
        if (words + nw > MAX_WORDS || clauses + m >= MAX_CLAUSES || lits + L >= MAX_LITERALS)
            return fail(p, ALLL_ERR_UNSUPPORTED, "item %llu: the union exceeds the loop's limits (2^30 variables, "
                                                 "2^32-4097 clauses, 2^32-1 literals)", (unsigned long long)i);
        GroupItem& g = p.items[i];
        g.seed = seeds[i];
        g.lit_base = lits;
        g.n_vars = pr.n_vars;
        g.n_words = (uint32_t)nw;
        g.word_base = (uint32_t)words;
        g.var_base = (uint32_t)(32 * words);
        g.clause_base = (uint32_t)clauses;
        g.n_clauses = (uint32_t)m;
        p.clause_base[i] = g.clause_base;
        words += nw;
        clauses += m;
        lits += L;
    }
    p.clause_base[n_items] = (uint32_t)clauses;
    p.n_clauses = clauses;
    const GroupItem& last = p.items[n_items - 1];
    p.n_vars = last.var_base + last.n_vars;

    // ---- the union's CSR (clause order inside an item kept, literals shifted) and the word table
    p.offsets.resize(clauses + 1);
    p.literals.resize(lits);
    p.words.resize(words);
    p.offsets[0] = 0;
    for (uint64_t i = 0; i < n_items; ++i) {
        const alll_problem& pr = probs[i];
        const GroupItem& g = p.items[i];
        const uint64_t L = g.n_clauses ? pr.offsets[g.n_clauses] : 0;
        for (uint64_t c = 0; c < g.n_clauses; ++c) p.offsets[g.clause_base + c + 1] = g.lit_base + pr.offsets[c + 1];
        const uint32_t shift = 2u * g.var_base;
        for (uint64_t j = 0; j < L; ++j) p.literals[g.lit_base + j] = pr.literals[j] + shift;
        for (uint32_t w = 0; w < g.n_words; ++w) {
            GroupWord& gw = p.words[g.word_base + w];
            gw.seed_lo = (uint32_t)g.seed;
            gw.seed_hi = (uint32_t)(g.seed >> 32);
            gw.local_word = w;
            gw.tail_mask = (w == g.n_words - 1 && (g.n_vars & 31u)) ? (1u << (g.n_vars & 31u)) - 1u : ~0u;
        }
    }
    return ALLL_OK;
}

}  // namespace alll
