// alll_group_runtime.cpp -- device set-up and host loop of the group entry points (include/alll.h,
// alll_group_*).  alll_group.cpp plans the block-diagonal union on the host; this
// file creates a one-instance context from it (alll_create: the existing planner and device
// set-up), attaches the group's tables, so that the context's captured iteration ends with the
// per-item accounting and the keyed resample, and drives the context's own launch batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "alll.h"
#include "alll_group.h"
#include "alll_group_dev.h"
#include "alll_group_probe.h"
#include "alll_probe.h"
#include "alll_propagate.h"
#include "alll_rt_util.h"
#include "alll_residual.h"
#include "alll_score.h"

using namespace alll;

struct alll_group {
    alll_ctx* ctx = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;  // the context's
    uint64_t max_iters = 0;
    std::vector<GroupItem> items;
    GroupDev d{};                  // (the context keeps a pointer to it)
    GroupItemState* h_items = nullptr;  // pinned, n_items
    std::vector<void*> allocs;
    // per-variable probabilities, allocated at the first item that gets thresholds:
    // the union's thresholds (zeros for unbiased items and past every item's n_vars) and a bit per
    // assignment word of the union, set for the words of the biased items
    const uint32_t* d_thr = nullptr;
    const uint32_t* d_wbias = nullptr;
    std::vector<uint32_t> wbias;   // host copy
    std::vector<uint8_t> biased;   // per item
    const uint32_t* d_word_item = nullptr;  // unit propagation: the item of every word of the union
    // best-assignment tracking, allocated at the first alll_group_track_best(on):
    // the items' records and flags and the item of every word (the context keeps a pointer to it)
    GroupBest best{};
    bool tracking = false;
};

namespace {

template <typename T>
int upload(alll_group* g, const T** p, const T* src, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed", bytes);
    g->allocs.push_back(q);
    HIP_TRY(hipMemset(q, 0, bytes));
    if (count && src) HIP_TRY(hipMemcpy(q, src, count * sizeof(T), hipMemcpyHostToDevice));
    *p = static_cast<const T*>(q);
    return ALLL_OK;
}

// the loop state (the context's pinned mirror) and the items' states, stream drained
int read_all(alll_group* g) {
    if (int rc = ctx_read_state(g->ctx)) return rc;
    HIP_TRY(hipMemcpy(g->h_items, g->d.items, sizeof(GroupItemState) * g->d.n_items, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

void to_stats(const alll_group* g, uint64_t i, alll_stats* st) {
    const DevState& ds = *ctx_access(g->ctx).h_state;
    const GroupItemState& s = g->h_items[i];
    memset(st, 0, sizeof(*st));
    // an unfinished item has made every pass of the union (the items advance in lock step)
    st->n_iterations = s.end_iter ? s.end_iter : ds.n_iter;
    st->n_resamples = s.n_resamples;
    st->sum_mis_size = s.sum_mis;
    st->avg_mis_size = st->n_iterations ? s.sum_mis / st->n_iterations : 0;
    st->n_violated = s.n_violated;
    st->solved = s.end_iter ? 1 : 0;
    st->n_gpus = 1;
    st->lfmis_rounds_max = ds.max_rounds;   // (the union's)
    st->lfmis_tail_rounds = ds.tail_rounds;
    st->gpu_resamples[0] = s.n_resamples;
}

void fill_all(const alll_group* g, alll_stats* stats) {
    if (stats)
        for (uint32_t i = 0; i < g->d.n_items; ++i) to_stats(g, i, &stats[i]);
}

bool any_solved(const alll_group* g) {
    for (uint32_t i = 0; i < g->d.n_items; ++i)
        if (g->h_items[i].end_iter) return true;
    return false;
}

}  // namespace

extern "C" {

int alll_group_destroy(alll_group* g) {
    if (!g) return ALLL_OK;
    if (g->ctx) alll_destroy(g->ctx);  // (drains the stream; its graphs hold the group's pointers)
    (void)hipSetDevice(g->device);
    for (void* p : g->allocs) (void)hipFree(p);
    if (g->h_items) (void)hipHostFree(g->h_items);
    delete g;
    return ALLL_OK;
}

int alll_group_create(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options* opt_in,
                      alll_group** out) {
    if (!out) return fail(ALLL_ERR_INVALID_ARG, "group: null argument");
    *out = nullptr;
    alll_options opt;
    if (opt_in) opt = *opt_in; else alll_default_options(&opt);
    // ---- plan on the host: the group is validated before a device is touched
    GroupPlan plan;
    int rc;
    if ((rc = plan_group(probs, seeds, n_items, opt, plan))) return fail(rc, "%s", plan.err.c_str());

    alll_group* g = new (std::nothrow) alll_group();
    if (!g) return fail(ALLL_ERR_OOM, "host allocation failed");
    auto bail = [&](int code) { alll_group_destroy(g); return code; };
    g->max_iters = opt.max_iters;
    g->items = std::move(plan.items);
    g->d.n_items = (uint32_t)n_items;

    // ---- the union as one context (its seed is unused: every draw is keyed by an item)
    alll_problem un{};
    un.n_vars = plan.n_vars;
    un.n_clauses = plan.n_clauses;
    un.offsets = plan.offsets.data();
    un.literals = plan.literals.data();
    opt.set_starts = nullptr;
    if ((rc = alll_create(&un, &opt, &g->ctx))) return bail(rc);
    const CtxAccess a = ctx_access(g->ctx);
    g->device = a.device;
    g->stream = a.stream;
    if (hipSetDevice(g->device) != hipSuccess) return bail(fail(ALLL_ERR_HIP, "hipSetDevice failed"));

    // ---- the group's tables, the items' own initial assignments
    const GroupItemState* d_items = nullptr;
    const unsigned long long* d_scratch = nullptr;
    const GroupCtl* d_ctl = nullptr;
    if ((rc = upload(g, &g->d.words, plan.words.data(), plan.words.size())) ||
        (rc = upload(g, &g->d.clause_base, plan.clause_base.data(), plan.clause_base.size())) ||
        (a.n_perm && (rc = upload(g, &g->d.perm, a.perm, (size_t)a.n_perm))) ||
        (rc = upload<GroupItemState>(g, &d_items, nullptr, (size_t)n_items)) ||
        (rc = upload<unsigned long long>(g, &d_scratch, nullptr, (size_t)n_items * GROUP_SCRATCH)) ||
        (rc = upload<GroupCtl>(g, &d_ctl, nullptr, 1)))
        return bail(rc);
    g->d.items = const_cast<GroupItemState*>(d_items);
    g->d.scratch = const_cast<unsigned long long*>(d_scratch);
    g->d.ctl = const_cast<GroupCtl*>(d_ctl);
    if (hipHostMalloc((void**)&g->h_items, sizeof(GroupItemState) * n_items, 0) != hipSuccess)
        return bail(fail(ALLL_ERR_OOM, "hipHostMalloc failed"));
    memset(g->h_items, 0, sizeof(GroupItemState) * n_items);
    if (launch_group_init(*a.b, g->d, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "init kernel failed: %s", hipGetErrorString(hipGetLastError())));
    ctx_attach_group(g->ctx, &g->d);
    *out = g;
    return ALLL_OK;
}

int alll_group_solve(alll_group* g, uint32_t flags, alll_stats* stats, int32_t* status) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (flags & ~ALLL_GROUP_FIRST_SOLVED) return fail(ALLL_ERR_INVALID_ARG, "group solve: unknown flags 0x%x", flags);
    HIP_TRY(hipSetDevice(g->device));
    const bool first = (flags & ALLL_GROUP_FIRST_SOLVED) != 0;
    int rc;
    if ((rc = read_all(g))) return rc;
    const DevState* st = ctx_access(g->ctx).h_state;
    const uint64_t cap = g->max_iters ? g->max_iters : ~0ull;
    if (st->done != 1 && !(first && any_solved(g))) {
        if ((rc = ctx_write_limits(g->ctx, cap, cap))) return rc;
        uint64_t batch = 1;
        for (;;) {  // (launch batches as alll_solve's: every one ends with a read of the device state)
            if ((rc = ctx_launch_iterations(g->ctx, batch))) return rc;
            if ((rc = read_all(g))) return rc;
            if (st->done || st->n_iter >= cap || (first && any_solved(g))) break;
            batch = std::min<uint64_t>(batch * 2, 64);
        }
    }
    fill_all(g, stats);
    if (status)
        for (uint32_t i = 0; i < g->d.n_items; ++i) status[i] = g->h_items[i].end_iter ? ALLL_OK : ALLL_ERR_MAX_ITERS;
    return ALLL_OK;
}

int alll_group_run(alll_group* g, uint64_t n_iters, alll_stats* stats) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    HIP_TRY(hipSetDevice(g->device));
    int rc;
    if (n_iters) {
        // (the limit is set on the device, stream-ordered before the iterations, as alll_run's)
        HIP_TRY(launch_set_limits(*ctx_access(g->ctx).b, n_iters, g->stream));
        if ((rc = ctx_launch_iterations(g->ctx, n_iters))) return rc;
    }
    if (stats) {
        if ((rc = read_all(g))) return rc;
        fill_all(g, stats);
    }
    return ALLL_OK;
}

int alll_group_get_stats(alll_group* g, uint64_t item, alll_stats* stats) {
    if (!g || !stats) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    HIP_TRY(hipSetDevice(g->device));
    if (int rc = read_all(g)) return rc;
    to_stats(g, item, stats);
    return ALLL_OK;
}

int alll_group_get_assignment_words(alll_group* g, uint64_t item, uint32_t* out, uint64_t n_words) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    const GroupItem& it = g->items[item];
    if (!out && it.n_words) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < it.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", it.n_words);
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (it.n_words)
        HIP_TRY(hipMemcpy(out, ctx_access(g->ctx).b->A + it.word_base, it.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_group_set_assignment_words(alll_group* g, uint64_t item, const uint32_t* in, uint64_t n_words) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    const GroupItem& it = g->items[item];
    if (!in && it.n_words) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < it.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", it.n_words);
    HIP_TRY(hipSetDevice(g->device));
    if (int rc = read_all(g)) return rc;
    // a solved item is final (as a solved context, which no later call advances): the union's loop
    // would resample it again if its new assignment violated a clause
    if (g->h_items[item].end_iter)
        return fail(ALLL_ERR_INVALID_ARG, "item %llu is solved: its assignment is final", (unsigned long long)item);
    std::vector<uint32_t> w(in, in + it.n_words);
    if (!w.empty() && (it.n_vars & 31)) w.back() &= (1u << (it.n_vars & 31)) - 1u;
    if (it.n_words)
        HIP_TRY(hipMemcpy(ctx_access(g->ctx).b->A + it.word_base, w.data(), it.n_words * 4ull, hipMemcpyHostToDevice));
    ctx_assignment_changed(g->ctx);
    return ALLL_OK;
}

int alll_group_set_var_thresholds(alll_group* g, uint64_t item, const uint32_t* thr, uint64_t n) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    int rc;
    if ((rc = ctx_bias_supported(g->ctx))) return rc;
    const GroupItem& it = g->items[item];
    if (thr && n != it.n_vars)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for the %u variables of item %llu",
                    (unsigned long long)n, it.n_vars, (unsigned long long)item);
    HIP_TRY(hipSetDevice(g->device));
    if ((rc = read_all(g))) return rc;  // (drains the stream)
    const CtxAccess a = ctx_access(g->ctx);
    if (a.h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds are set before the group's first iteration (%llu made)",
                    (unsigned long long)a.h_state->n_iter);
    const uint32_t n_words = a.b->n_words;  // the union's
    const bool on = thr && it.n_words;
    if (on && !g->d_thr) {
        g->wbias.assign((n_words + 31) / 32, 0u);
        g->biased.assign(g->d.n_items, 0);
        if ((rc = upload<uint32_t>(g, &g->d_thr, nullptr, (size_t)n_words * 32)) ||
            (rc = upload<uint32_t>(g, &g->d_wbias, nullptr, g->wbias.size())))
            return rc;
    }
    if (g->d_thr) {
        if (on)
            HIP_TRY(hipMemcpy(const_cast<uint32_t*>(g->d_thr) + it.var_base, thr, (size_t)it.n_vars * 4,
                              hipMemcpyHostToDevice));
        for (uint32_t w = it.word_base; w < it.word_base + it.n_words; ++w) {
            if (on) g->wbias[w >> 5] |= 1u << (w & 31);
            else g->wbias[w >> 5] &= ~(1u << (w & 31));
        }
        g->biased[item] = on;
        HIP_TRY(hipMemcpy(const_cast<uint32_t*>(g->d_wbias), g->wbias.data(), g->wbias.size() * 4, hipMemcpyHostToDevice));
        const bool any = std::find(g->biased.begin(), g->biased.end(), 1) != g->biased.end();
        ctx_set_group_bias(g->ctx, any ? g->d_thr : nullptr, any ? g->d_wbias : nullptr);
    }
    // the item's words again: the biased fill, or its unbiased one
    if (launch_fill_words(a.b->A + it.word_base, it.n_words, it.n_vars, on ? g->d_thr + it.var_base : nullptr, it.seed,
                          g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess)
        return fail(ALLL_ERR_HIP, "fill kernel failed: %s", hipGetErrorString(hipGetLastError()));
    ctx_assignment_changed(g->ctx);
    return ALLL_OK;
}

// What the propagation, the scores and the residual hand to their drivers: the union's clauses and
// sizes and the group's tables (thr == nullptr: no item has thresholds).  The item of every word is
// built and uploaded at the first call.
static int group_prop_args(alll_group* g, const CtxAccess& a, PropArgs* p) {
    const uint32_t n = g->d.n_items;
    if (!g->d_word_item) {
        std::vector<uint32_t> word_item(a.b->n_words, 0u);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t w = 0; w < g->items[i].n_words; ++w) word_item[g->items[i].word_base + w] = i;
        if (int rc = upload(g, &g->d_word_item, word_item.data(), word_item.size())) return rc;
    }
    *p = PropArgs{};
    p->lits = a.cv->lits;
    p->offs = a.cv->offs;
    p->m = a.cv->m;
    p->k = a.cv->k;
    p->n_vars = a.b->n_vars;
    p->n_words = a.b->n_words;
    p->n_items = n;
    p->thr = const_cast<uint32_t*>(g->d_thr);
    p->words = g->d.words;
    p->wbias = g->d_wbias;
    p->word_item = g->d_word_item;
    p->clause_base = g->d.clause_base;
    return ALLL_OK;
}

// Unit propagation of every item's pins at once: the context's three kernels over the
// union, the items' records apart; a global round is every unfinished item's own round.
int alll_group_propagate_pins(alll_group* g, uint64_t max_rounds, alll_propagate_result* results) {
    if (!g || !results) return fail(ALLL_ERR_INVALID_ARG, "propagate pins: null argument");
    int rc;
    if ((rc = ctx_bias_supported(g->ctx))) return rc;
    HIP_TRY(hipSetDevice(g->device));
    if ((rc = read_all(g))) return rc;  // (drains the stream)
    const CtxAccess a = ctx_access(g->ctx);
    if (a.h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "propagate pins: allowed before the group's first iteration only (%llu made)",
                    (unsigned long long)a.h_state->n_iter);
    const uint32_t n = g->d.n_items;
    std::vector<uint8_t> on(n, 0);
    if (g->d_thr) on = g->biased;
    PropArgs p{};
    if ((rc = group_prop_args(g, a, &p))) return rc;
    if ((rc = prop_drive(p, on.data(), max_rounds, results, g->stream))) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const GroupItem& it = g->items[i];
        alll_propagate_result& r = results[i];
        // the item's own clause index; its words again, the biased fill of its propagated thresholds
        r.conflict_clause = r.status == ALLL_PROP_CONFLICT ? r.conflict_clause - it.clause_base : it.n_clauses;
        if (on[i] && launch_fill_words(a.b->A + it.word_base, it.n_words, it.n_vars, g->d_thr + it.var_base, it.seed,
                                       g->stream) != hipSuccess)
            return fail(ALLL_ERR_HIP, "fill kernel failed: %s", hipGetErrorString(hipGetLastError()));
    }
    HIP_TRY(hipStreamSynchronize(g->stream));
    ctx_assignment_changed(g->ctx);
    return ALLL_OK;
}

// Split scores of every item at once: one pass of the context's scoring kernels
// over the union; the items' scores are then cut out of the union's array, without its word padding.
int alll_group_var_scores(alll_group* g, alll_split_result* results, uint64_t* scores, uint64_t n_scores) {
    if (!g || !results) return fail(ALLL_ERR_INVALID_ARG, "var scores: null argument");
    int rc;
    if ((rc = ctx_bias_supported(g->ctx))) return rc;
    const uint32_t n = g->d.n_items;
    uint64_t want = 0;
    for (const GroupItem& it : g->items) want += 2ull * it.n_vars;
    if (scores && n_scores != want)
        return fail(ALLL_ERR_INVALID_ARG, "var scores: %llu entries for the %llu literals of the items",
                    (unsigned long long)n_scores, (unsigned long long)want);
    HIP_TRY(hipSetDevice(g->device));
    const CtxAccess a = ctx_access(g->ctx);
    PropArgs p{};
    if ((rc = group_prop_args(g, a, &p))) return rc;
    std::vector<uint32_t> item_vars(2ull * n);
    for (uint32_t i = 0; i < n; ++i) {
        item_vars[2 * i] = g->items[i].var_base;
        item_vars[2 * i + 1] = g->items[i].n_vars;
    }
    std::vector<uint64_t> S;
    if ((rc = score_drive(p, item_vars, results, scores ? &S : nullptr, g->stream))) return rc;
    if (scores)
        for (const GroupItem& it : g->items) {
            if (it.n_vars) memcpy(scores, S.data() + 2ull * it.var_base, 16ull * it.n_vars);
            scores += 2ull * it.n_vars;
        }
    return ALLL_OK;
}

// The residual formula of every item at once: one pass of the context's compaction
// kernels over the union; they write the items' arrays one after another, in local numbering.
int alll_group_residual(alll_group* g, alll_residual_result* results, uint64_t* offsets, uint32_t* literals,
                        uint32_t* var_map, uint64_t* clause_map, uint32_t* thr_out) {
    if (!g || !results) return fail(ALLL_ERR_INVALID_ARG, "residual: null argument");
    int rc;
    if ((rc = ctx_bias_supported(g->ctx))) return rc;
    const uint32_t n = g->d.n_items;
    HIP_TRY(hipSetDevice(g->device));
    const CtxAccess a = ctx_access(g->ctx);
    PropArgs p{};
    if ((rc = group_prop_args(g, a, &p))) return rc;
    std::vector<ResidItem> items(n);
    for (uint32_t i = 0; i < n; ++i) {
        const GroupItem& it = g->items[i];
        items[i] = ResidItem{it.var_base, it.n_vars, it.word_base, it.n_words, it.clause_base, it.n_clauses};
    }
    // the union's literal count: the capacity of the literal array
    uint64_t n_lits = p.m * p.k;
    if (!p.k && p.m) {
        uint32_t last = 0;
        HIP_TRY(hipStreamSynchronize(g->stream));
        HIP_TRY(hipMemcpy(&last, p.offs + p.m, 4, hipMemcpyDeviceToHost));
        n_lits = last;
    }
    return resid_drive(p, items, n_lits, results, ResidOut{offsets, literals, var_map, clause_map, thr_out}, g->stream);
}

// Failed-literal probing of every item at once: the call is validated and laid out on
// the host (plan_group_probes), then the probe kernels' group forms run over the union with scratch of
// their own on the drained stream; nothing of the group is written.
int alll_group_probe_literals(alll_group* g, const uint32_t* probes, const uint64_t* probe_offsets, uint64_t max_rounds,
                              alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, uint64_t n_row_words) {
    if (!g || !results || !probe_offsets) return fail(ALLL_ERR_INVALID_ARG, "group probes: null argument");
    int rc;
    if ((rc = ctx_bias_supported(g->ctx))) return rc;
    if (!pm_rows != !pv_rows) return fail(ALLL_ERR_INVALID_ARG, "group probes: the two row arrays go together");
    const CtxAccess a = ctx_access(g->ctx);
    GroupProbePlan plan;
    if ((rc = plan_group_probes(g->items.data(), g->items.size(), a.b->n_vars, probes, probe_offsets, pm_rows != nullptr,
                                n_row_words, probe_forced_chunk(), PROBE_BUDGET_BYTES, plan)))
        return fail(rc, "%s", plan.err.c_str());
    if (plan.n_probes == 0) return ALLL_OK;
    HIP_TRY(hipSetDevice(g->device));
    PropArgs p{};
    if ((rc = group_prop_args(g, a, &p))) return rc;
    return group_probe_drive(p, plan, g->items.data(), probes, max_rounds, results, pm_rows, pv_rows, g->stream);
}

int alll_group_get_var_thresholds(alll_group* g, uint64_t item, uint32_t* out, uint64_t n) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    const GroupItem& it = g->items[item];
    if (!g->d_thr || !g->biased[item])
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: item %llu has none", (unsigned long long)item);
    if (n != it.n_vars || (!out && n))
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for the %u variables of item %llu",
                    (unsigned long long)n, it.n_vars, (unsigned long long)item);
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (n) HIP_TRY(hipMemcpy(out, g->d_thr + it.var_base, (size_t)n * 4, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_group_track_best(alll_group* g, int on) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    int rc;
    if ((rc = ctx_track_supported(g->ctx))) return rc;
    HIP_TRY(hipSetDevice(g->device));
    if ((rc = read_all(g))) return rc;  // (drains the stream)
    const CtxAccess a = ctx_access(g->ctx);
    if (a.h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "best-assignment tracking is switched before the group's first iteration "
                                          "(%llu made)", (unsigned long long)a.h_state->n_iter);
    const uint32_t n = g->d.n_items;
    if (on && !g->best.rec) {
        std::vector<uint32_t> word_item(a.b->n_words, 0u);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t w = 0; w < g->items[i].n_words; ++w) word_item[g->items[i].word_base + w] = i;
        const unsigned long long* rec = nullptr;
        const uint32_t* improved = nullptr;
        if ((rc = upload<unsigned long long>(g, &rec, nullptr, (size_t)n * 2)) ||
            (rc = upload<uint32_t>(g, &improved, nullptr, (size_t)n)) ||
            (rc = upload(g, &g->best.word_item, word_item.data(), word_item.size())))
            return rc;
        g->best.rec = const_cast<unsigned long long*>(rec);
        g->best.improved = const_cast<uint32_t*>(improved);
    }
    if (on) {  // empty records: {~0, 0} per item, no flag
        std::vector<unsigned long long> rec((size_t)n * 2, 0ull);
        for (uint32_t i = 0; i < n; ++i) rec[2 * (size_t)i] = ~0ull;
        if (n) HIP_TRY(hipMemcpy(g->best.rec, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
        if (n) HIP_TRY(hipMemset(g->best.improved, 0, (size_t)n * 4));
    }
    if ((rc = ctx_set_group_best(g->ctx, on ? &g->best : nullptr))) return rc;
    g->tracking = on != 0;
    return ALLL_OK;
}

int alll_group_get_best(alll_group* g, uint64_t item, uint64_t* n_violated, uint64_t* iteration, uint32_t* words,
                        uint64_t n_words) {
    if (!g) return fail(ALLL_ERR_INVALID_ARG, "null group");
    if (item >= g->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, g->d.n_items);
    if (!g->tracking)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: the group does not track it (alll_group_track_best before "
                                          "the first iteration)");
    const GroupItem& it = g->items[item];
    if (words && n_words != it.n_words)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: %llu words for the %u of item %llu",
                    (unsigned long long)n_words, it.n_words, (unsigned long long)item);
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));
    unsigned long long rec[2];
    HIP_TRY(hipMemcpy(rec, g->best.rec + 2 * item, sizeof rec, hipMemcpyDeviceToHost));
    if (n_violated) *n_violated = rec[0];
    if (iteration) *iteration = rec[1];
    // (before any pass the words are left untouched)
    if (words && rec[1] && it.n_words)
        HIP_TRY(hipMemcpy(words, ctx_access(g->ctx).b->A_best + it.word_base, it.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_group_layout(alll_group* g) { return g ? alll_layout(g->ctx) : -1; }

const char* alll_group_eval_kernel(alll_group* g) { return g ? alll_eval_kernel(g->ctx) : ""; }

int alll_group_epoch_counters(alll_group* g, uint64_t out[4]) {
    if (!g || !out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    return alll_epoch_counters(g->ctx, out);
}

}  // extern "C"
