// alll_batch_runtime.cpp -- device set-up and host loop of the batch entry points (include/alll.h,
// alll_batch_*).  alll_batch.cpp plans and packs on the host; this file uploads the
// image and relaunches the LDS-resident kernel (alll_small.hip) slice by slice.  The host never
// waits inside a kernel: a launch runs at most `slice` iterations of every item.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "alll.h"
#include "alll_batch.h"
#include "alll_rt_util.h"
#include "alll_small.h"

using namespace alll;

namespace {

// Iterations per launch.  Measured on the MI355X (profiles/batch/summary.txt):
// items of 8192 clauses that never solve take 17.5 - 18.6 us per iteration (64 and 256 items, one
// workgroup per CU), so a launch of 256 iterations takes 4.6 - 4.8 ms; 1024 would take 18 ms.
constexpr uint32_t DEFAULT_SLICE = 256;

// Violated sets up to this size take the kernel's one-wave serial greedy instead of the claim rounds
// (ALLL_BATCH_SERIAL_MAX, 0 .. 64, overrides it: tuning, tests).  The results do not depend on it.
// Measured: equal at 4, up to 3x slower at 16 and 64, so the claim rounds serve all.
constexpr uint32_t DEFAULT_SERIAL_MAX = 0;

uint32_t serial_max_knob() {
    const char* e = getenv("ALLL_BATCH_SERIAL_MAX");
    if (!e || !*e) return DEFAULT_SERIAL_MAX;
    return (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), 64);
}

// ALLL_BATCH_THR_GLOBAL=1: a biased batch reads its thresholds from global memory also where they
// would fit the LDS (tuning, tests).  The results do not depend on it.
bool thr_global_knob() {
    const char* e = getenv("ALLL_BATCH_THR_GLOBAL");
    return e && *e && strtoull(e, nullptr, 10) != 0;
}

}  // namespace

struct alll_batch {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t max_iters = 0;
    uint32_t slice = DEFAULT_SLICE;
    std::vector<SmallItem> items;
    SmallBatch d{};
    SmallState* h_state = nullptr;  // pinned, n_items
    std::vector<void*> allocs;
    // per-variable thresholds: the pool is allocated at the first item that gets some
    uint32_t max_vars = 0, max_clauses = 0, max_lits = 0, a_words = 0;
    bool thr_global = false;      // ALLL_BATCH_THR_GLOBAL: never the LDS copy
    std::vector<uint8_t> biased;  // per item
    uint32_t* d_best = nullptr;   // best-assignment tracking: the records' words, d.best while it is on
};

namespace {

template <typename T>
int upload(alll_batch* b, const T** p, const T* src, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed", bytes);
    b->allocs.push_back(q);
    if (count) HIP_TRY(hipMemcpy(q, src, count * sizeof(T), hipMemcpyHostToDevice));
    *p = static_cast<const T*>(q);
    return ALLL_OK;
}

int read_states(alll_batch* b) {
    HIP_TRY(hipMemcpyAsync(b->h_state, b->d.states, sizeof(SmallState) * b->d.n_items, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return ALLL_OK;
}

void to_stats(const SmallState& s, alll_stats* st) {
    memset(st, 0, sizeof(*st));
    st->n_iterations = s.n_iter;
    st->n_resamples = s.n_resamples;
    st->sum_mis_size = s.sum_mis;
    st->avg_mis_size = s.n_iter ? s.sum_mis / s.n_iter : 0;
    st->n_violated = s.n_violated;
    st->solved = s.done == 1 ? 1 : 0;
    st->n_gpus = 1;
    st->lfmis_rounds_max = s.rounds_max;
    st->gpu_resamples[0] = s.n_resamples;
}

uint64_t count_active(const alll_batch* b, uint64_t* n_solved) {
    uint64_t active = 0, solved = 0;
    for (uint32_t i = 0; i < b->d.n_items; ++i) {
        const SmallState& s = b->h_state[i];
        active += s.done == 0 && s.n_iter < s.limit_eval;
        solved += s.done == 1;
    }
    *n_solved = solved;
    return active;
}

// slices until no item can advance (or, first_solved, until a slice solved one more item)
int run_slices(alll_batch* b, bool first_solved) {
    int rc;
    if ((rc = read_states(b))) return rc;
    uint64_t solved0, solved;
    uint64_t active = count_active(b, &solved0);
    while (active) {
        HIP_TRY(launch_small_slice(b->d, b->slice, b->stream));
        if ((rc = read_states(b))) return rc;
        active = count_active(b, &solved);
        if (first_solved && solved > solved0) break;
    }
    return ALLL_OK;
}

void fill_all(const alll_batch* b, alll_stats* stats) {
    if (stats)
        for (uint32_t i = 0; i < b->d.n_items; ++i) to_stats(b->h_state[i], &stats[i]);
}

bool is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace

extern "C" {

int alll_batch_fits(uint32_t n_vars, uint64_t n_clauses, uint64_t n_literals) {
    return batch_fits(n_vars, n_clauses, n_literals) ? 1 : 0;
}

int alll_batch_create(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options* opt_in,
                      alll_batch** out) {
    if (!out) return fail(ALLL_ERR_INVALID_ARG, "batch: null argument");
    *out = nullptr;
    alll_options opt;
    if (opt_in) opt = *opt_in; else alll_default_options(&opt);
    // ---- plan on the host: the batch is validated before a device is touched
    BatchPlan plan;
    int rc;
    if ((rc = plan_batch(probs, seeds, n_items, opt, plan))) return fail(rc, "%s", plan.err.c_str());

    const int ndev = alll_device_count();
    if (ndev <= 0) return fail(ALLL_ERR_NO_DEVICE, "no HIP device visible");
    int dev = opt.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) return fail(ALLL_ERR_NO_DEVICE, "device %d not visible (%d devices)", dev, ndev);
    if (!is_gfx950(dev)) return fail(ALLL_ERR_NO_DEVICE, "device %d is not gfx950 (MI355X)", dev);
    HIP_TRY(hipSetDevice(dev));

    alll_batch* b = new (std::nothrow) alll_batch();
    if (!b) return fail(ALLL_ERR_OOM, "host allocation failed");
    auto bail = [&](int code) { alll_batch_destroy(b); return code; };
    b->device = dev;
    b->max_iters = opt.max_iters;
    b->items = std::move(plan.items);
    b->d.n_items = (uint32_t)n_items;
    b->d.threads = plan.threads;
    b->d.lds = plan.lds;
    b->d.serial_max = serial_max_knob();
    b->thr_global = thr_global_knob();
    b->max_vars = plan.max_vars;
    b->max_clauses = plan.max_clauses;
    b->max_lits = plan.max_lits;
    b->a_words = plan.a_words;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "hipStreamCreate failed"));
    if (hipHostMalloc((void**)&b->h_state, sizeof(SmallState) * n_items, 0) != hipSuccess)
        return bail(fail(ALLL_ERR_OOM, "hipHostMalloc failed"));
    memset(b->h_state, 0, sizeof(SmallState) * n_items);
    for (uint64_t i = 0; i < n_items; ++i) {
        b->h_state[i].limit_eval = b->h_state[i].limit_nores = ~0ull;
        b->h_state[i].best_u = ~0u;  // (no record yet)
    }
    const SmallState* states = nullptr;
    const uint32_t* A = nullptr;
    const std::vector<uint32_t> zeros(plan.a_words, 0u);
    if ((rc = upload(b, &b->d.items, b->items.data(), b->items.size())) ||
        (rc = upload(b, &b->d.lits, plan.lits.data(), plan.lits.size())) ||
        (rc = upload(b, &b->d.offs, plan.offs.data(), plan.offs.size())) ||
        (rc = upload(b, &states, b->h_state, (size_t)n_items)) || (rc = upload(b, &A, zeros.data(), zeros.size())))
        return bail(rc);
    b->d.states = const_cast<SmallState*>(states);
    b->d.A = const_cast<uint32_t*>(A);
    hipError_t e = small_prepare();
    if (e != hipSuccess) return bail(fail(ALLL_ERR_HIP, "kernel attributes: %s", hipGetErrorString(e)));
    if (launch_small_init(b->d, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "init kernel failed: %s", hipGetErrorString(hipGetLastError())));
    *out = b;
    return ALLL_OK;
}

int alll_batch_destroy(alll_batch* b) {
    if (!b) return ALLL_OK;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (void* p : b->allocs) (void)hipFree(p);
    if (b->h_state) (void)hipHostFree(b->h_state);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    return ALLL_OK;
}

int alll_batch_solve(alll_batch* b, uint32_t flags, alll_stats* stats, int32_t* status) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (flags & ~ALLL_BATCH_FIRST_SOLVED) return fail(ALLL_ERR_INVALID_ARG, "batch solve: unknown flags 0x%x", flags);
    HIP_TRY(hipSetDevice(b->device));
    const uint64_t cap = b->max_iters ? b->max_iters : ~0ull;
    HIP_TRY(launch_small_limits(b->d, true, cap, b->stream));
    if (int rc = run_slices(b, (flags & ALLL_BATCH_FIRST_SOLVED) != 0)) return rc;
    fill_all(b, stats);
    if (status)
        for (uint32_t i = 0; i < b->d.n_items; ++i) status[i] = b->h_state[i].done == 1 ? ALLL_OK : ALLL_ERR_MAX_ITERS;
    return ALLL_OK;
}

int alll_batch_run(alll_batch* b, uint64_t n_iters, alll_stats* stats) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    if (n_iters) {
        HIP_TRY(launch_small_limits(b->d, false, n_iters, b->stream));
        if (int rc = run_slices(b, false)) return rc;
    } else if (stats) {
        if (int rc = read_states(b)) return rc;
    }
    fill_all(b, stats);
    return ALLL_OK;
}

int alll_batch_get_stats(alll_batch* b, uint64_t item, alll_stats* stats) {
    if (!b || !stats) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    HIP_TRY(hipSetDevice(b->device));
    SmallState s;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(&s, b->d.states + item, sizeof s, hipMemcpyDeviceToHost));
    to_stats(s, stats);
    return ALLL_OK;
}

int alll_batch_get_assignment_words(alll_batch* b, uint64_t item, uint32_t* out, uint64_t n_words) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    const SmallItem& it = b->items[item];
    if (!out && it.n_words) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < it.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", it.n_words);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (it.n_words) HIP_TRY(hipMemcpy(out, b->d.A + it.a_at, it.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_batch_set_assignment_words(alll_batch* b, uint64_t item, const uint32_t* in, uint64_t n_words) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    const SmallItem& it = b->items[item];
    if (!in && it.n_words) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < it.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", it.n_words);
    HIP_TRY(hipSetDevice(b->device));
    std::vector<uint32_t> w(in, in + it.n_words);
    if (!w.empty() && (it.n_vars & 31)) w.back() &= (1u << (it.n_vars & 31)) - 1u;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (it.n_words) HIP_TRY(hipMemcpy(b->d.A + it.a_at, w.data(), it.n_words * 4ull, hipMemcpyHostToDevice));
    return ALLL_OK;
}

int alll_batch_set_var_thresholds(alll_batch* b, uint64_t item, const uint32_t* thr, uint64_t n) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    SmallItem& it = b->items[item];
    if (thr && n != it.n_vars)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for the %u variables of item %llu",
                    (unsigned long long)n, it.n_vars, (unsigned long long)item);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    SmallState s;
    HIP_TRY(hipMemcpy(&s, b->d.states + item, sizeof s, hipMemcpyDeviceToHost));
    if (s.n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds are set before the item's first iteration (%llu made)",
                    (unsigned long long)s.n_iter);
    const bool on = thr && it.n_words;
    // ---- the thresholds into the pool (item i's at 32 * a_at, zeros up to its whole words), the item's flag
    if (on && !b->d.thr) {
        void* q = nullptr;
        const size_t bytes = std::max<size_t>((size_t)b->a_words * 128, 16);
        if (hipMalloc(&q, bytes) != hipSuccess) return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed", bytes);
        b->allocs.push_back(q);
        HIP_TRY(hipMemset(q, 0, bytes));
        b->d.thr = static_cast<const uint32_t*>(q);
        b->biased.assign(b->d.n_items, 0);
    }
    if (on)
        HIP_TRY(hipMemcpy(const_cast<uint32_t*>(b->d.thr) + 32ull * it.a_at, thr, (size_t)it.n_vars * 4, hipMemcpyHostToDevice));
    if (b->d.thr) {
        it.pad = on ? 1u : 0u;
        b->biased[item] = on;
        HIP_TRY(hipMemcpy(const_cast<SmallItem*>(b->d.items) + item, &it, sizeof it, hipMemcpyHostToDevice));
    }
    // ---- the item's words again: the biased fill, or its unbiased one
    if (it.n_words) {
        std::vector<uint8_t> bits(it.n_vars);
        if (int rc = on ? alll_biased_initial_assignment(it.seed, it.n_vars, thr, bits.data())
                        : alll_initial_assignment(it.seed, it.n_vars, bits.data()))
            return rc;
        std::vector<uint32_t> w(it.n_words, 0u);
        for (uint32_t v = 0; v < it.n_vars; ++v) w[v >> 5] |= (uint32_t)bits[v] << (v & 31);
        HIP_TRY(hipMemcpy(b->d.A + it.a_at, w.data(), it.n_words * 4ull, hipMemcpyHostToDevice));
    }
    // ---- the launch choice: the biased instantiation while any item has thresholds; they are
    // LDS-resident when the batch's layout with them fits the budget
    b->d.biased = std::find(b->biased.begin(), b->biased.end(), 1) != b->biased.end();
    uint32_t at = 0;
    const SmallLds with = small_lds_layout(b->max_vars, b->max_clauses, b->max_lits, &at);
    const bool in_lds = !b->thr_global && with.bytes <= SMALL_LDS_BUDGET;
    b->d.thr_lds = in_lds ? at : 0;
    b->d.lds_thr_bytes = with.bytes;
    return ALLL_OK;
}

// Unit propagation of every item's pins: one launch, a workgroup per item; then the
// propagated items' words again, as alll_batch_set_var_thresholds writes them.
int alll_batch_propagate_pins(alll_batch* b, uint64_t max_rounds, alll_propagate_result* results) {
    if (!b || !results) return fail(ALLL_ERR_INVALID_ARG, "propagate pins: null argument");
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = read_states(b)) return rc;  // (drains the stream)
    const uint32_t n = b->d.n_items;
    for (uint32_t i = 0; i < n; ++i)
        if (b->h_state[i].n_iter != 0)
            return fail(ALLL_ERR_INVALID_ARG, "propagate pins: allowed before the batch's first iteration only "
                                              "(item %u has made %llu)", i, (unsigned long long)b->h_state[i].n_iter);
    if (!b->d.thr) {  // no item has ever had thresholds
        for (uint32_t i = 0; i < n; ++i) results[i] = alll_propagate_result{b->items[i].m, 0, 0, ALLL_PROP_NONE};
        return ALLL_OK;
    }
    SmallProp* d_out = nullptr;
    if (hipMalloc((void**)&d_out, sizeof(SmallProp) * n) != hipSuccess)
        return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed", sizeof(SmallProp) * n);
    std::vector<SmallProp> out(n);
    // (more rounds than an item has variables never apply: such a cap is no cap)
    const uint32_t cap = max_rounds > ALLL_BATCH_MAX_VARS + 1u ? 0u : (uint32_t)max_rounds;
    hipError_t e = launch_small_propagate(b->d, const_cast<uint32_t*>(b->d.thr), cap, d_out, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) e = hipMemcpy(out.data(), d_out, sizeof(SmallProp) * n, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ALLL_ERR_HIP, "propagate kernel failed: %s", hipGetErrorString(e));
    std::vector<uint32_t> thr, w;
    std::vector<uint8_t> bits;
    for (uint32_t i = 0; i < n; ++i) {
        const SmallItem& it = b->items[i];
        results[i] = alll_propagate_result{out[i].conflict, out[i].n_forced, out[i].rounds, (int32_t)out[i].status};
        if (out[i].status == ALLL_PROP_NONE || !it.n_words) continue;
        thr.resize(it.n_vars);
        bits.resize(it.n_vars);
        HIP_TRY(hipMemcpy(thr.data(), b->d.thr + 32ull * it.a_at, (size_t)it.n_vars * 4, hipMemcpyDeviceToHost));
        if (int rc = alll_biased_initial_assignment(it.seed, it.n_vars, thr.data(), bits.data())) return rc;
        w.assign(it.n_words, 0u);
        for (uint32_t v = 0; v < it.n_vars; ++v) w[v >> 5] |= (uint32_t)bits[v] << (v & 31);
        HIP_TRY(hipMemcpy(b->d.A + it.a_at, w.data(), it.n_words * 4ull, hipMemcpyHostToDevice));
    }
    return ALLL_OK;
}

int alll_batch_get_var_thresholds(alll_batch* b, uint64_t item, uint32_t* out, uint64_t n) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    const SmallItem& it = b->items[item];
    if (!b->d.thr || !it.pad)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: item %llu has none", (unsigned long long)item);
    if (n != it.n_vars || (!out && n))
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for the %u variables of item %llu",
                    (unsigned long long)n, it.n_vars, (unsigned long long)item);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (n) HIP_TRY(hipMemcpy(out, b->d.thr + 32ull * it.a_at, (size_t)n * 4, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_batch_track_best(alll_batch* b, int on) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = read_states(b)) return rc;  // (drains the stream)
    for (uint32_t i = 0; i < b->d.n_items; ++i)
        if (b->h_state[i].n_iter != 0)
            return fail(ALLL_ERR_INVALID_ARG, "best-assignment tracking is switched before the batch's first iteration "
                                              "(item %u has made %llu)", i, (unsigned long long)b->h_state[i].n_iter);
    if (on && !b->d_best) {
        void* q = nullptr;
        const size_t bytes = std::max<size_t>((size_t)b->a_words * 4, 16);
        if (hipMalloc(&q, bytes) != hipSuccess) return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed", bytes);
        b->allocs.push_back(q);
        HIP_TRY(hipMemset(q, 0, bytes));
        b->d_best = static_cast<uint32_t*>(q);
    }
    b->d.best = on ? b->d_best : nullptr;  // (no item has made a pass: every record is still empty)
    return ALLL_OK;
}

int alll_batch_get_best(alll_batch* b, uint64_t item, uint64_t* n_violated, uint64_t* iteration, uint32_t* words,
                        uint64_t n_words) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (item >= b->d.n_items) return fail(ALLL_ERR_INVALID_ARG, "item %llu of %u", (unsigned long long)item, b->d.n_items);
    if (!b->d.best)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: the batch does not track it (alll_batch_track_best before "
                                          "the first iteration)");
    const SmallItem& it = b->items[item];
    if (words && n_words != it.n_words)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: %llu words for the %u of item %llu",
                    (unsigned long long)n_words, it.n_words, (unsigned long long)item);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    SmallState s;
    HIP_TRY(hipMemcpy(&s, b->d.states + item, sizeof s, hipMemcpyDeviceToHost));
    if (n_violated) *n_violated = s.best_iter ? s.best_u : ~0ull;
    if (iteration) *iteration = s.best_iter;
    // (before any pass the words are left untouched)
    if (words && s.best_iter && it.n_words)
        HIP_TRY(hipMemcpy(words, b->d.best + it.a_at, it.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_batch_set_slice(alll_batch* b, uint64_t iters_per_launch) {
    if (!b) return fail(ALLL_ERR_INVALID_ARG, "null batch");
    if (iters_per_launch > ALLL_BATCH_MAX_SLICE)
        return fail(ALLL_ERR_INVALID_ARG, "slice %llu > %u: a launch must stay bounded", (unsigned long long)iters_per_launch,
                    ALLL_BATCH_MAX_SLICE);
    b->slice = iters_per_launch ? (uint32_t)iters_per_launch : DEFAULT_SLICE;
    return ALLL_OK;
}

}  // extern "C"
