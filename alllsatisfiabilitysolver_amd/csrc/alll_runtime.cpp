// alll_runtime.cpp -- host side of the C-ABI (include/alll.h): device memory layout,
// the per-iteration launch sequence (captured once into a hipGraph), the RCCL exchange of
// the clause-sharded multi-GPU mode, statistics.
//
// Reference correspondence: alll_create ~ SATInstance(var_arr, n_threads) +
// VariablesArray(n_vars) (SATInstance.h:51-56, VariablesArray.h:23-34); alll_solve ~
// SATInstance::solve -> parallel_solve (SATInstance.h:60-66, 217-320); alll_verify ~
// verify_validity (SATInstance.h:156-173).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "alll.h"
#include "alll_group_dev.h"
#include "alll_internal.h"
#include "alll_layout.h"
#include "alll_probe.h"
#include "alll_propagate.h"
#include "alll_rt_util.h"
#include "alll_residual.h"
#include "alll_score.h"

using namespace alll;

namespace {

thread_local std::string g_err;

#define NCCL_TRY(expr)                                                                    \
    do {                                                                                  \
        ncclResult_t _r = (expr);                                                         \
        if (_r != ncclSuccess)                                                            \
            return fail(ALLL_ERR_RCCL, "%s failed: %s", #expr, ncclGetErrorString(_r));  \
    } while (0)

constexpr uint32_t DEFAULT_GRID_ROUNDS = 4;
// captured graphs of 1, 2, 4 and 8 iterations: a batch of n iterations replays n / 8 eight-
// iteration graphs and at most one of each smaller size (one launch gap per graph)
constexpr int GRAPH_SIZES = 4;
constexpr uint32_t GRAPH_UNROLL = 1u << (GRAPH_SIZES - 1);
constexpr uint32_t SKEWED_GRID_ROUNDS = 7;  // instances with hot variables

}  // namespace

struct alll_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    alll_options opt{};
    uint32_t n_vars = 0;
    uint64_t m = 0;
    uint64_t n_lits = 0;
    ClauseView cv{};
    LoopBuffers b{};
    uint32_t tiles_per_rank = 0, own_begin = 0, own_end = 0, n_tiles_padded = 0;
    uint32_t grid_rounds = DEFAULT_GRID_ROUNDS;
    // One GPU, bucketed round 0: the evaluation workgroups scatter their runs' claims themselves
    // (k_eval_scatter<K>, no k_bscatter launch; +2.6% iterations/s at M in round 4).  The
    // evaluation alone keeps its own kernel (k_eval_hybrid<K>: alll_bench_eval, verify, the
    // other variants) for its roofline.  env ALLL_FUSE_SCATTER=0: the separate k_bscatter
    bool fuse_scatter = true;
    int rank = 0, world = 1;
    bool allreduce = false;
    ncclComm_t comm = nullptr;
    // device allocations
    std::vector<void*> allocs;
    DevState* h_state = nullptr;  // pinned mirror
    // captured iterations per LFMIS variant (0: atomic round 0, 1: bucketed round 0, 2: one grid
    // round + tail for few violated clauses): [v][j]
    // holds 2^j iterations
    hipGraph_t graph[3][GRAPH_SIZES] = {};
    hipGraphExec_t graph_exec[3][GRAPH_SIZES] = {};
    bool use_graph = true;
    std::string graph_note;      // why the loop launches eagerly (empty: graphs replay)
    // Hint for the LFMIS variant of the next launch batch (round0_variant): the violated count
    // and pass count of the last pass the host knows of.  read_state refreshes it; every
    // launch batch ends with an asynchronous copy of the device state into h_async, adopted
    // by the next batch once its event has completed (so a run(sync=False) loop follows the
    // device a batch behind instead of freezing at the last read); an assignment set by the
    // caller makes it unknown (treated as large).
    uint64_t hint_u = ~0ull, hint_iter = 0;
    // Round robin with the fixpoint passes: every iteration is a graph of the evaluation, the
    // set-up and rr_p passes, then (host-driven, after reading the pass state) single-pass
    // graphs until the passes settle (at most fp_max), then the finishing graph (k_rr_mw when
    // they did not, resample).  rr_p = the passes the last iteration needed.
    uint32_t rr_p = 8;
    std::vector<hipGraph_t> rr_graph;         // every captured round-robin graph (destroyed at the end)
    std::vector<hipGraphExec_t> rr_pre;       // [P]: evaluation .. set-up + P passes
    hipGraphExec_t rr_more = nullptr, rr_full = nullptr, rr_post = nullptr;
    uint32_t* h_fp = nullptr;                 // pinned copy of RRFpCtl's first words {state, nu, fp_iter, .., inc}
    DevState* h_async = nullptr;  // pinned
    hipEvent_t ev_async = nullptr;
    bool async_pending = false;
    uint64_t small_u = 0;       // one grid round (then the tail) when the last pass found at most
                                // this many violated clauses (variant 2)
    uint64_t bucket_min_u = 0;  // bucketed round 0 when the last pass found at least this many
    hipEvent_t ev[8] = {};
    int n_cu = 256;
    bool hybrid = false;
    alll_exchange_fn xfn = nullptr;  // host-staged exchange (instead of RCCL)
    void* xuser = nullptr;
    std::vector<uint8_t> xbuf;
    std::vector<uint32_t> perm;  // evaluation position -> clause id (fixed-k layout)
    std::string eval_name;
    int wall_khz = 100000;       // s_memrealtime rate (ALLL_FLAG_KERNEL_TIMING)
    // Streaming solve with T > 1 threads (b.srr_T > 0): the reference's
    // ClauseGenerator states (ClauseGenerator.h:104-113) between iterations, the plan of the next
    // one (pinned, uploaded per iteration) and the device lists, grown on demand
    struct SGen { uint64_t base = 0, n = 0, c = 0, ny = 0; bool fin = false; };
    std::vector<SGen> sgen;
    bool srr_started = false;   // an iteration ran: the next one starts where its check stopped
    uint64_t srr_batch = 1;
    SrrGen* h_srr = nullptr;
    SrrPlan* h_plan = nullptr;
    unsigned long long* h_first = nullptr;
    size_t srr_cap_blk = 0, srr_cap_ent = 0, srr_cap_step = 0;
    int rw_occupancy = 0;       // resident k_fp_repair workgroups per CU found at create (-1: query failed)
    // block-diagonal group (alll_group_runtime.cpp): the iteration ends with the
    // group's per-item accounting and keyed resample instead of k_resample_vars; nullptr otherwise
    const GroupDev* grp = nullptr;
    // per-variable probabilities: the context's own copy of the thresholds (b.thr
    // points to it while they are set), and a group's per-word bits
    uint32_t* d_thr = nullptr;
    const uint32_t* grp_wbias = nullptr;
    // best-assignment tracking: the record's words (b.A_best points to them while
    // tracking is on), and a group's tables
    uint32_t* d_best = nullptr;
    const GroupBest* grp_best = nullptr;
};

namespace {

template <typename T>
int dalloc(alll_ctx* c, T** p, size_t count, int fill = 0) {
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess)
        return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    c->allocs.push_back(q);
    e = hipMemsetAsync(q, fill, bytes, c->stream);
    if (e != hipSuccess) return fail(ALLL_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    *p = static_cast<T*>(q);
    return ALLL_OK;
}

// dalloc, then v's contents once the zero-fill has drained (`what` names it in the failure text)
template <typename T, typename P>
int upload(alll_ctx* c, P** p, const std::vector<T>& v, const char* what) {
    T* d = nullptr;
    if (int rc = dalloc(c, &d, v.size())) return rc;
    if (hipStreamSynchronize(c->stream) != hipSuccess ||
        (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess))
        return fail(ALLL_ERR_HIP, "%s upload failed", what);
    *p = d;
    return ALLL_OK;
}

int read_state(alll_ctx* c) {
    HIP_TRY(hipMemcpyAsync(c->h_state, c->b.state, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hint_u = c->h_state->u_total;
    c->hint_iter = c->h_state->n_iter;
    c->async_pending = false;  // (the stream is drained: this read is newer)
    if (c->h_state->error == 4)
        return fail(ALLL_ERR_HIP, "round-robin MIS: a grid barrier of k_rr_mw timed out (its %u workgroups "
                                  "were not all resident)", c->b.rr_mw);
    if (c->h_state->error == 5)
        return fail(ALLL_ERR_HIP, "round-robin MIS: an incremental-pass kernel ran without its buffers (DESIGN.md §10)");
    if (c->h_state->error == 7)
        return fail(ALLL_ERR_HIP, "reference-RNG mode: a resample round needed more draws than its buffer holds");
    if (c->h_state->error == 6)
        return fail(ALLL_ERR_HIP, "streaming round robin: k_srr_mis made no progress (DESIGN.md §4.2.1)");
    if (c->h_state->error)
        return fail(ALLL_ERR_UNSUPPORTED, c->b.rr_T ? "round-robin MIS exceeded its batch cap in one iteration"
                                                    : "LFMIS needed more than %u rounds in one iteration",
                    MAX_TAIL_ROUNDS);
    return ALLL_OK;
}

int write_limits(alll_ctx* c, uint64_t limit_eval, uint64_t limit_nores) {
    // called only with the stream drained (after read_state)
    c->h_state->limit_eval = limit_eval;
    c->h_state->limit_nores = limit_nores;
    if (c->h_state->done == 2) c->h_state->done = 0;
    HIP_TRY(hipMemcpyAsync(c->b.state, c->h_state, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALLL_OK;
}

hipError_t eval_launch(alll_ctx* c, uint32_t tb, uint32_t te, bool gated, bool scatter = false, bool flags = false) {
    if (c->cv.rg_off) return launch_eval_ragged(c->cv, c->b, tb, te, gated, c->n_cu, c->stream);
    if (c->hybrid) return launch_eval_hybrid(c->cv, c->b, tb, te, gated, c->n_cu, scatter, c->stream, flags);
    return launch_eval(c->cv, c->b, tb, te, gated, c->stream);
}

// Host-staged collective: drain the stream, move the device buffer through host memory and
// the user's exchange function.  Allgather: `bytes` per rank, own piece at `own_off`.
int host_exchange(alll_ctx* c, int op, void* dev, size_t bytes, size_t own_off) {
    if (!c->xfn) return fail(ALLL_ERR_INVALID_ARG, "world > 1 without RCCL needs alll_set_host_exchange");
    const size_t total = op == ALLL_XCHG_ALLGATHER ? bytes * c->world : bytes;
    c->xbuf.resize(total);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (op == ALLL_XCHG_ALLGATHER)
        HIP_TRY(hipMemcpy(c->xbuf.data() + own_off, (uint8_t*)dev + own_off, bytes, hipMemcpyDeviceToHost));
    else
        HIP_TRY(hipMemcpy(c->xbuf.data(), dev, bytes, hipMemcpyDeviceToHost));
    if (c->xfn(c->xuser, op, c->xbuf.data(), bytes) != 0)
        return fail(ALLL_ERR_RCCL, "host exchange callback failed");
    HIP_TRY(hipMemcpy(dev, c->xbuf.data(), total, hipMemcpyHostToDevice));
    return ALLL_OK;
}

// Clause-sharded exchange after the evaluation: the violated bitmask pieces are all-gathered
// (clause order: cmask, marked from the own lists, when the evaluation order is not clause
// order; else the evaluation's own bitmask), then the other shards' lists are collected.
int enqueue_exchange(alll_ctx* c, hipStream_t s) {
    const size_t words = (size_t)c->tiles_per_rank * TILE_WORDS;
    uint64_t* mask = c->b.cmask ? c->b.cmask : c->b.vmask;
    if (c->b.cmask) HIP_TRY(launch_cmark(c->cv, c->b, words, c->rank, true, s));
    if (c->comm) {
        NCCL_TRY(ncclAllGather(mask + (size_t)c->rank * words, mask, words, ncclUint64, c->comm, s));
    } else {
        int rc = host_exchange(c, ALLL_XCHG_ALLGATHER, mask, words * 8, (size_t)c->rank * words * 8);
        if (rc) return rc;
    }
    HIP_TRY(launch_collect(c->cv, c->b, c->own_begin, c->own_end, s));
    return ALLL_OK;
}

// The launch sequence of one iteration (SATInstance.h:260-311).  Every kernel is gated on
// the device state, so replaying it after convergence is a no-op.
// Round-0 variant for the next iterations, from the last state read: the bucketed kernels
// have a fixed cost that only pays off on large violated sets (and they are not built for
// skewed instances, see create).
int round0_variant(const alll_ctx* c) {
    const uint64_t u = c->hint_u;
    if (c->b.rr_T) return 0;  // (round robin: launch_rr_iteration)
    if (c->b.pairs && (c->hint_iter == 0 || u >= c->bucket_min_u)) return 1;
    // few violated clauses (the end of a converging solve): round 0 on the grid, the rest in
    // the one-workgroup tail -- 6 launches per iteration instead of 12, each ~4.5 us even
    // when it has almost nothing to do
    if (c->hint_iter > 0 && u <= c->small_u && !c->b.rr_T) return 2;
    return 0;
}

// Adopt the asynchronous state copy of the last launch batch once it has landed.
// Ranks of a sharded run keep the hint of the synchronous state reads only (which they make at
// the same points of the loop), so that they pick the same graph variants at the same batches
// and capture their collectives in lockstep.
void refresh_hint(alll_ctx* c) {
    if (!c->async_pending) return;
    const hipError_t q = hipEventQuery(c->ev_async);
    if (q != hipSuccess) {
        // (hipErrorNotReady would stay the thread's last error and fail the next launch check)
        if (q == hipErrorNotReady) (void)hipGetLastError();
        return;
    }
    c->hint_u = c->h_async->u_total;
    c->hint_iter = c->h_async->n_iter;
    c->async_pending = false;
}

int post_state_copy(alll_ctx* c) {
    if (c->world > 1 || c->comm) return ALLL_OK;  // (sharded: synchronous hints only, refresh_hint)
    HIP_TRY(hipMemcpyAsync(c->h_async, c->b.state, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->ev_async, c->stream));
    c->async_pending = true;
    return ALLL_OK;
}

int enqueue_iteration(alll_ctx* c, hipEvent_t* marks, int variant) {
    hipStream_t s = c->stream;
    if (marks) HIP_TRY(hipEventRecord(marks[0], s));
    // one GPU, bucketed round 0: the evaluation workgroups scatter their runs' claims
    // themselves (no k_bscatter), before the reduce (pre-reduce epoch)
    const bool xchg = c->world > 1 || c->comm;  // the clause-sharded exchange path
    const bool scatter = variant == 1 && !xchg && c->hybrid && c->fuse_scatter && !c->b.rr_T;
    HIP_TRY(eval_launch(c, c->own_begin, c->own_end, true, scatter));
    if (marks) HIP_TRY(hipEventRecord(marks[1], s));
    if (xchg) {
        int rc = enqueue_exchange(c, s);
        if (rc) return rc;
    }
    if (marks) HIP_TRY(hipEventRecord(marks[2], s));
    // the bucketed round 0 runs the reduce in an extra k_bscatter workgroup (one GPU, no hot
    // variables, not the round robin): one launch less
    const bool fused = variant == 1 && !xchg && !c->b.rr_T;
    if (!fused) HIP_TRY(launch_reduce(c->b, 0, s));
    if (c->b.rr_T) {  // (without the fixpoint passes: k_rr_mw decides every iteration)
        HIP_TRY(launch_rr_prep(c->cv, c->b, false, s));
        HIP_TRY(launch_rr_finish(c->cv, c->b, s));
    } else {
        const uint32_t rounds = variant == 2 ? 1u : c->grid_rounds;
        for (uint32_t r = 0; r < rounds; ++r) {
            if (r == 0 && variant == 1)
                HIP_TRY(launch_round0_buckets(c->cv, c->b, rounds == 1, fused, scatter, s));
            else HIP_TRY(launch_round(c->cv, c->b, r, r + 1 == rounds, s));
        }
        HIP_TRY(launch_tail(c->cv, c->b, rounds, s));
    }
    if (marks) HIP_TRY(hipEventRecord(marks[3], s));
    if (c->allreduce && xchg) {
        HIP_TRY(launch_resample(c->cv, c->b, c->own_begin, c->own_end, true, s));
        if (c->comm) {
            NCCL_TRY(ncclAllReduce(c->b.delta, c->b.delta, c->b.n_words, ncclUint32, ncclSum, c->comm, s));
        } else {
            int rc = host_exchange(c, ALLL_XCHG_ALLREDUCE_SUM_U32, c->b.delta, (size_t)c->b.n_words * 4, 0);
            if (rc) return rc;
        }
        HIP_TRY(launch_apply_delta(c->b, s));
    } else if (c->grp) {
        HIP_TRY(launch_group_account(c->cv, c->b, *c->grp, s));
        HIP_TRY(launch_group_resample(c->b, *c->grp, c->grp_wbias, c->grp_best, s));
    } else {
        HIP_TRY(launch_resample(c->cv, c->b, c->own_begin, c->own_end, false, s));
    }
    if (marks) HIP_TRY(hipEventRecord(marks[4], s));
    return ALLL_OK;
}

// Round robin with the fixpoint passes: the pieces of one iteration.
//   pre(P):  evaluation [+ exchange] + reduce + scan entries + set-up + P passes
//   more:    one pass
//   post:    k_rr_mw (only if the passes did not settle) + resample
int enqueue_rr_piece(alll_ctx* c, hipEvent_t* marks, int piece, uint32_t passes) {
    hipStream_t s = c->stream;
    const bool xchg = c->world > 1 || c->comm;
    // one GPU, hybrid evaluation: the evaluation writes the clause-order violated flags itself
    const bool flags = !xchg && c->hybrid && c->b.rr_flag;
    if (piece == 0) {
        if (marks) HIP_TRY(hipEventRecord(marks[0], s));
        HIP_TRY(eval_launch(c, c->own_begin, c->own_end, true, false, flags));
        if (marks) HIP_TRY(hipEventRecord(marks[1], s));
        if (xchg) {
            int rc = enqueue_exchange(c, s);
            if (rc) return rc;
        }
        if (marks) HIP_TRY(hipEventRecord(marks[2], s));
        HIP_TRY(launch_reduce(c->b, 0, s));
        HIP_TRY(launch_rr_prep(c->cv, c->b, flags, s));
        HIP_TRY(launch_rr_passes(c->cv, c->b, passes, true, s));
    } else if (piece == 1 || piece == 3) {  // one incremental (1) or full (3) pass
        HIP_TRY(launch_rr_passes(c->cv, c->b, passes, piece == 3, s));
    } else {
        HIP_TRY(launch_rr_finish(c->cv, c->b, s));
        if (marks) HIP_TRY(hipEventRecord(marks[3], s));
        if (c->allreduce && xchg) {
            HIP_TRY(launch_resample(c->cv, c->b, c->own_begin, c->own_end, true, s));
            if (c->comm) {
                NCCL_TRY(ncclAllReduce(c->b.delta, c->b.delta, c->b.n_words, ncclUint32, ncclSum, c->comm, s));
            } else {
                int rc = host_exchange(c, ALLL_XCHG_ALLREDUCE_SUM_U32, c->b.delta, (size_t)c->b.n_words * 4, 0);
                if (rc) return rc;
            }
            HIP_TRY(launch_apply_delta(c->b, s));
        } else {
            HIP_TRY(launch_resample(c->cv, c->b, c->own_begin, c->own_end, false, s));
        }
        if (marks) HIP_TRY(hipEventRecord(marks[4], s));
    }
    return ALLL_OK;
}

// captured once per (piece, passes); nullptr when the loop launches eagerly
int rr_graph_of(alll_ctx* c, int piece, uint32_t passes, hipGraphExec_t* out) {
    *out = nullptr;
    hipGraphExec_t* slot = piece == 0 ? &c->rr_pre[passes] : piece == 1 ? &c->rr_more : piece == 3 ? &c->rr_full
                                                                                               : &c->rr_post;
    if (!c->use_graph) return ALLL_OK;
    if (*slot) { *out = *slot; return ALLL_OK; }
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        c->use_graph = false;
        c->graph_note = std::string("hipStreamBeginCapture: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return ALLL_OK;
    }
    const int rc = enqueue_rr_piece(c, nullptr, piece, passes);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(c->stream, &g);
    if (rc != ALLL_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        c->graph_note = rc != ALLL_OK ? "capture of the iteration failed: " + g_err
                                      : std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        c->use_graph = false;
        return ALLL_OK;
    }
    c->rr_graph.push_back(g);
    e = hipGraphInstantiate(slot, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        *slot = nullptr;
        c->use_graph = false;
        c->graph_note = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return ALLL_OK;
    }
    (void)hipGraphUpload(*slot, c->stream);
    *out = *slot;
    return ALLL_OK;
}

int launch_rr_piece(alll_ctx* c, hipEvent_t* marks, int piece, uint32_t passes) {
    hipGraphExec_t g = nullptr;
    int rc;
    if (!marks && (rc = rr_graph_of(c, piece, passes, &g))) return rc;
    if (g) {
        HIP_TRY(hipGraphLaunch(g, c->stream));
        return ALLL_OK;
    }
    return enqueue_rr_piece(c, marks, piece, passes);
}

// One round-robin iteration with host-driven passes: pre(rr_p) (a full pass, then incremental
// ones), then one pass at a time while the pass state (read back) is still running -- an
// incremental one, or a full one after an incremental pass gave up -- at most fp_max in all, then
// post.  The host reads the pass state per decision instead of the GPU running passes after
// convergence.
int launch_rr_iteration(alll_ctx* c, hipEvent_t* marks) {
    const uint32_t cap = c->b.fp_max;
    uint32_t done = std::min(c->rr_p, cap);
    int rc;
    if ((rc = launch_rr_piece(c, marks, 0, done))) return rc;
    constexpr size_t ctl_words = offsetof(RRFpCtl, inc) / 4 + 1;  // {state, nu, fp_iter, ..., inc}
    for (;;) {
        HIP_TRY(hipMemcpyAsync(c->h_fp, c->b.fp_ctl, ctl_words * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->h_fp[0] != FP_RUN || done >= cap) break;
        const bool inc = c->h_fp[offsetof(RRFpCtl, inc) / 4] != 0;
        if ((rc = launch_rr_piece(c, marks, inc ? 1 : 3, 1))) return rc;
        ++done;
    }
    // next iteration: the passes this one needed (fp_iter = passes that changed the picks)
    // (two or four passes fewer, with more host-driven passes after them: within noise at M
    // and C5)
    if (c->h_fp[0] == FP_FINAL || c->h_fp[0] == FP_DONE) c->rr_p = std::max<uint32_t>(1, std::min(cap, c->h_fp[2] + 1));
    return launch_rr_piece(c, marks, 2, 0);
}

// ---- streaming solve with T > 1 threads ------------------------------------
// Device lists grown on demand (the stream is drained: the caller has just read the state).
int srr_grow(alll_ctx* c, uint32_t** p, size_t& cap, size_t need) {
    if (need <= cap) return ALLL_OK;
    need = std::max<size_t>(need + need / 4, 1024);
    if (*p) { (void)hipFree(*p); *p = nullptr; cap = 0; }
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need * 4);
    if (e != hipSuccess) return fail(ALLL_ERR_OOM, "hipMalloc(%zu bytes) failed: %s", need * 4, hipGetErrorString(e));
    *p = static_cast<uint32_t*>(q);
    cap = need;
    return ALLL_OK;
}

// smallest s >= 1 with s = b_t (mod p_t) for every generator: the batch step at which all of them
// finish together (1 <= b_t <= p_t); false when there is none, or it lies beyond 2^62
bool srr_common_finish(const std::vector<uint64_t>& bs, const std::vector<uint64_t>& ps, uint64_t* S) {
    __int128 a = 0, mod = 1;  // s = a (mod mod)
    for (size_t t = 0; t < bs.size(); ++t) {
        const __int128 n2 = ps[t], a2 = bs[t] % ps[t];
        // a + mod k = a2 (mod n2)
        __int128 r0 = mod, r1 = n2, x0 = 1, x1 = 0;  // extended Euclid: x0 mod = r0 (mod n2)
        while (r1) {
            const __int128 q = r0 / r1, r = r0 - q * r1, x = x0 - q * x1;
            r0 = r1; r1 = r; x0 = x1; x1 = x;
        }
        const __int128 g = r0, d = a2 - a;
        if (d % g != 0) return false;
        const __int128 n2g = n2 / g;
        __int128 k = ((d / g) % n2g) * (x0 % n2g) % n2g;
        if (k < 0) k += n2g;
        a = a + mod * k;
        mod = mod * n2g;
        if (mod > ((__int128)1 << 62)) return false;
        a %= mod;
    }
    *S = a == 0 ? (uint64_t)mod : (uint64_t)a;
    return true;
}

// One iteration: evaluation + reduce (the previous iteration's check) + the check's stop offsets;
// then, while the loop is active, the plan from the generators' states, the lists, the round robins
// and the resample.  Host-synchronous (one state read per iteration).
int launch_srr_iteration(alll_ctx* c, hipEvent_t* marks) {
    hipStream_t s = c->stream;
    LoopBuffers& b = c->b;
    const uint32_t T = b.srr_T;
    if (marks) HIP_TRY(hipEventRecord(marks[0], s));
    HIP_TRY(eval_launch(c, c->own_begin, c->own_end, true));
    if (marks) { HIP_TRY(hipEventRecord(marks[1], s)); HIP_TRY(hipEventRecord(marks[2], s)); }
    HIP_TRY(launch_reduce(b, 0, s));
    HIP_TRY(launch_srr_first(b, s));
    HIP_TRY(hipMemcpyAsync(c->h_first, b.srr_first, T * 8ull, hipMemcpyDeviceToHost, s));
    int rc = read_state(c);
    if (rc) return rc;
    if (!c->h_state->active) {
        if (marks) { HIP_TRY(hipEventRecord(marks[3], s)); HIP_TRY(hipEventRecord(marks[4], s)); }
        return ALLL_OK;
    }
    std::vector<alll_ctx::SGen>& gens = c->sgen;
    if (c->srr_started) {
        // the lock-step check stopped after its first step that found a violated clause: every
        // generator has yielded min(n_t, f + 1) clauses (oracle/alll_oracle.c orc_solve_stream_rr)
        unsigned long long f = ~0ull;
        for (uint32_t t = 0; t < T; ++t) f = std::min(f, c->h_first[t]);
        for (auto& g : gens) {
            g.ny = std::min<uint64_t>(g.n, f + 1);
            g.fin = g.ny == g.n;
        }
    }
    // ---- plan: every generator's first window (r steps, finished at batch step b) and walks (p
    // steps each); the step S at which all finish together; the lists stop at the step by which
    // every generator has walked its whole range (later steps re-yield seen clauses only)
    const uint64_t B = c->srr_batch;
    std::vector<uint64_t> bs(T), ps(T), zs(T);
    for (uint32_t t = 0; t < T; ++t) {
        const auto& g = gens[t];
        SrrGen& d = c->h_srr[t];
        d.base = g.base;
        d.n = g.n;
        d.pt = g.n ? 9223372036854775783ull % g.n : 0;
        d.c0 = g.c;
        if (g.n == 0) { d.r = 0; d.b = 1; d.p = 1; zs[t] = 1; }
        else {
            d.r = g.fin ? g.n : g.n - g.ny;
            d.b = (d.r + B - 1) / B;
            d.p = (g.n + B - 1) / B;
            zs[t] = d.r == g.n ? d.b : d.b + d.p;
        }
        bs[t] = d.b;
        ps[t] = d.p;
    }
    uint64_t S = 0;
    if (!srr_common_finish(bs, ps, &S))
        return fail(ALLL_ERR_UNSUPPORTED, "streaming solve, %u threads: the generators never finish at the same "
                                          "batch step (the reference's loop, SATInstance.h:98-125, would not end)", T);
    const uint64_t steps = std::min<uint64_t>(S, *std::max_element(zs.begin(), zs.end()));
    uint64_t nblk = 0, total = 0;
    for (uint32_t t = 0; t < T; ++t) {
        SrrGen& d = c->h_srr[t];
        uint64_t y = 0;
        if (d.n) {
            if (steps <= d.b) y = std::min<uint64_t>(d.r, steps * B);
            else {
                const uint64_t q = steps - d.b;
                y = d.r + (q / d.p) * d.n + std::min<uint64_t>(d.n, (q % d.p) * B);
            }
        }
        d.yields = y;
        d.vblk = nblk;
        d.e0 = 0;
        nblk += (y + SRR_BLK - 1) / SRR_BLK;
        total += y;
    }
    c->h_srr[T] = SrrGen{};
    c->h_srr[T].vblk = nblk;
    if (total >= 0xFFFFFFFFull || nblk >= (1ull << 31) || (steps + 1) * T >= (1ull << 40))
        return fail(ALLL_ERR_UNSUPPORTED, "streaming solve: %llu walk steps in one iteration (limit 2^32)",
                    (unsigned long long)total);
    *c->h_plan = SrrPlan{T, (uint32_t)nblk, B, steps, S - steps};
    if ((rc = srr_grow(c, &b.srr_bcnt, c->srr_cap_blk, 2 * nblk + 1)) ||
        (rc = srr_grow(c, &b.srr_ent, c->srr_cap_ent, std::max<uint64_t>(total, 1) * SRR_ENT_WORDS)) ||
        (rc = srr_grow(c, &b.srr_step, c->srr_cap_step, (steps + 1) * T)))
        return rc;
    HIP_TRY(hipMemcpyAsync(b.srr_gen, c->h_srr, (T + 1) * sizeof(SrrGen), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.srr_plan, c->h_plan, sizeof(SrrPlan), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_srr_lists(c->cv, b, (uint32_t)nblk, s));
    HIP_TRY(launch_srr_mis(c->cv, b, s));
    if (marks) HIP_TRY(hipEventRecord(marks[3], s));
    HIP_TRY(launch_resample(c->cv, b, c->own_begin, c->own_end, false, s));
    if (marks) HIP_TRY(hipEventRecord(marks[4], s));
    // after the batch loop every generator has finished (n_yielded = n_t) at walk position
    // c0 + (its walk steps in all S batch steps) P: r + whole walks, i.e. c0 + r P (mod n_t)
    for (uint32_t t = 0; t < T; ++t) {
        auto& g = gens[t];
        const SrrGen& d = c->h_srr[t];
        if (g.n) g.c = (uint64_t)(((unsigned __int128)(d.r % g.n) * d.pt + g.c) % g.n);
        g.ny = g.n;
        g.fin = true;
    }
    c->srr_started = true;
    // (the pinned plan is read by the copies above; the next iteration drains the stream in its
    // state read before it rewrites the plan)
    return ALLL_OK;
}

int ensure_graph(alll_ctx* c, int variant, int j) {
    if (!c->use_graph || c->graph_exec[variant][j]) return ALLL_OK;
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        c->use_graph = false;
        c->graph_note = std::string("hipStreamBeginCapture: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return ALLL_OK;
    }
    int rc = ALLL_OK;
    for (uint32_t i = 0; i < (1u << j) && rc == ALLL_OK; ++i) rc = enqueue_iteration(c, nullptr, variant);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(c->stream, &g);
    if (rc != ALLL_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        c->graph_note = rc != ALLL_OK ? "capture of the iteration failed: " + g_err
                                      : std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        c->use_graph = false;  // fall back to eager launches (alll_uses_graphs reports it)
        return ALLL_OK;
    }
    e = hipGraphInstantiate(&c->graph_exec[variant][j], g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        c->graph_exec[variant][j] = nullptr;
        c->use_graph = false;
        c->graph_note = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return ALLL_OK;
    }
    c->graph[variant][j] = g;
    (void)hipGraphUpload(c->graph_exec[variant][j], c->stream);
    return ALLL_OK;
}

// n iterations: n / 8 replays of the 8-iteration graph, then one replay per set bit of n % 8
int launch_srr_iteration(alll_ctx* c, hipEvent_t* marks);

int launch_iterations(alll_ctx* c, uint64_t n) {
    if (c->b.srr_T) {
        int rc;
        for (uint64_t i = 0; i < n; ++i)
            if ((rc = launch_srr_iteration(c, nullptr))) return rc;
        return ALLL_OK;
    }
    if (c->b.rr_T && c->b.fp_ctl) {
        int rc;
        for (uint64_t i = 0; i < n; ++i)
            if ((rc = launch_rr_iteration(c, nullptr))) return rc;
        return ALLL_OK;
    }
    refresh_hint(c);
    const int variant = round0_variant(c);
    int rc;
    // every size is captured, instantiated and uploaded at the variant's first launch, so a
    // later batch never pays a capture
    for (int j = 0; j < GRAPH_SIZES; ++j)
        if ((rc = ensure_graph(c, variant, j))) return rc;
    if (!c->use_graph) {
        for (uint64_t i = 0; i < n; ++i)
            if ((rc = enqueue_iteration(c, nullptr, variant))) return rc;
        return post_state_copy(c);
    }
    for (; n >= GRAPH_UNROLL; n -= GRAPH_UNROLL)
        HIP_TRY(hipGraphLaunch(c->graph_exec[variant][GRAPH_SIZES - 1], c->stream));
    for (int j = GRAPH_SIZES - 2; j >= 0; --j)
        if ((n >> j) & 1u) HIP_TRY(hipGraphLaunch(c->graph_exec[variant][j], c->stream));
    return post_state_copy(c);
}

int fill_stats(alll_ctx* c, alll_stats* st) {
    int rc = read_state(c);
    if (rc) return rc;
    std::vector<unsigned long long> ts(2 * (size_t)c->b.n_tiles);
    if (!ts.empty())
        HIP_TRY(hipMemcpy(ts.data(), c->b.tile_stats, ts.size() * 8, hipMemcpyDeviceToHost));
    memset(st, 0, sizeof(*st));
    st->n_iterations = c->h_state->n_iter;
    for (uint32_t t = 0; t < c->b.n_tiles; ++t) {
        st->sum_mis_size += ts[2 * t];
        st->n_resamples += ts[2 * t + 1];
        const uint32_t r = c->tiles_per_rank ? t / c->tiles_per_rank : 0;
        if (r < ALLL_MAX_GPU_STATS) st->gpu_resamples[r] += ts[2 * t + 1];
    }
    if (c->opt.stream_batch && st->n_iterations) {
        // a stream iteration is evaluation + MIS + resample + the full check (SATInstance.h:
        // 91-147); the check is the next evaluation pass, so the stream iterations are the
        // resample rounds: every pass but a final non-resampling one (solved or capped), and
        // at least one (a start that is already satisfied)
        const uint64_t rounds = st->n_iterations - (c->h_state->done ? 1 : 0);
        st->n_iterations = rounds ? rounds : 1;
    }
    st->avg_mis_size = st->n_iterations ? st->sum_mis_size / st->n_iterations : 0;
    st->n_violated = c->h_state->u_total;
    st->solved = (c->h_state->done == 1) ? 1 : 0;
    st->n_gpus = c->world;
    st->lfmis_rounds_max = c->h_state->max_rounds;
    st->lfmis_tail_rounds = c->h_state->tail_rounds;
    return ALLL_OK;
}

// Captured iterations hold LoopBuffers (and the group's pointers) by value: after a change of
// either they are dropped, and the next launch batch captures them again.  Stream drained.
void drop_graphs(alll_ctx* c) {
    for (int v = 0; v < 3; ++v)
        for (int u = 0; u < GRAPH_SIZES; ++u) {
            if (c->graph_exec[v][u]) (void)hipGraphExecDestroy(c->graph_exec[v][u]);
            if (c->graph[v][u]) (void)hipGraphDestroy(c->graph[v][u]);
            c->graph_exec[v][u] = nullptr;
            c->graph[v][u] = nullptr;
        }
    for (auto& g : c->rr_pre) {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
    }
    for (hipGraphExec_t* g : {&c->rr_more, &c->rr_full, &c->rr_post}) {
        if (*g) (void)hipGraphExecDestroy(*g);
        *g = nullptr;
    }
    for (auto g : c->rr_graph) (void)hipGraphDestroy(g);
    c->rr_graph.clear();
}

// Per-variable probabilities and best-assignment tracking (§4.9) hook into the
// resample kernels of the one-GPU loop only (resample_body): `what` names the feature in the message.
int resample_hook_supported(const alll_ctx* c, const char* what) {
    if ((c->opt.flags & ALLL_FLAG_REFERENCE_RNG) || c->b.rrng_mask)
        return fail(ALLL_ERR_UNSUPPORTED, "%s: ALLL_FLAG_REFERENCE_RNG draws the reference's own fair-coin stream "
                                          "(its own resample kernels)", what);
    if ((c->opt.flags & ALLL_FLAG_EXCHANGE_ALLREDUCE) || c->allreduce)
        return fail(ALLL_ERR_UNSUPPORTED, "%s: ALLL_FLAG_EXCHANGE_ALLREDUCE resamples through the delta exchange, "
                                          "which draws fair coins only", what);
    bool zero_id = true;
    for (int i = 0; i < 128; ++i) zero_id &= c->opt.comm_id[i] == 0;
    if (c->world != 1 || c->comm || !zero_id)
        return fail(ALLL_ERR_UNSUPPORTED, "%s: one GPU only (world %d%s)", what, c->world,
                    zero_id ? "" : ", a communicator id");
    if (c->opt.stream_batch != 0)
        return fail(ALLL_ERR_UNSUPPORTED, "%s: the streaming solve (stream_batch %llu) is not covered", what,
                    (unsigned long long)c->opt.stream_batch);
    return ALLL_OK;
}
int bias_supported(const alll_ctx* c) { return resample_hook_supported(c, "variable thresholds"); }
int track_supported(const alll_ctx* c) { return resample_hook_supported(c, "best-assignment tracking"); }

// Switches the tracking of the best assignment: gb = a group's tables.  Before the
// first iteration only: captured iterations hold LoopBuffers by value.
int set_track_best(alll_ctx* c, bool on, const GroupBest* gb) {
    int rc;
    if ((rc = read_state(c))) return rc;  // (drains the stream)
    if (c->h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "best-assignment tracking is switched before the first iteration (%llu made)",
                    (unsigned long long)c->h_state->n_iter);
    if (on && !c->d_best) {
        if ((rc = dalloc(c, &c->d_best, (size_t)c->b.n_words))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->b.A_best = on ? c->d_best : nullptr;
    c->grp_best = on ? gb : nullptr;
    c->h_state->best_u = ~0ull;
    c->h_state->best_iter = 0;
    c->h_state->improved = 0;
    HIP_TRY(hipMemcpy(c->b.state, c->h_state, sizeof(DevState), hipMemcpyHostToDevice));
    drop_graphs(c);  // (none is captured before the first iteration; one would hold the old pointer)
    return ALLL_OK;
}

bool is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace

// ---- the context as the group's runtime drives it (alll_group_dev.h)
namespace alll {

CtxAccess ctx_access(alll_ctx* c) {
    return CtxAccess{c->device, c->stream, &c->b, &c->cv, c->h_state, c->perm.data(), c->perm.size()};
}
void ctx_attach_group(alll_ctx* c, const GroupDev* g) { c->grp = g; }
int ctx_read_state(alll_ctx* c) { return read_state(c); }
int ctx_write_limits(alll_ctx* c, uint64_t limit_eval, uint64_t limit_nores) { return write_limits(c, limit_eval, limit_nores); }
int ctx_launch_iterations(alll_ctx* c, uint64_t n) { return launch_iterations(c, n); }
void ctx_assignment_changed(alll_ctx* c) {
    c->hint_u = ~0ull;
    c->async_pending = false;
}
int ctx_bias_supported(alll_ctx* c) { return bias_supported(c); }
void ctx_set_group_bias(alll_ctx* c, const uint32_t* thr, const uint32_t* wbias) {
    c->b.thr = thr;
    c->grp_wbias = wbias;
    drop_graphs(c);
}
int ctx_track_supported(alll_ctx* c) { return track_supported(c); }
int ctx_set_group_best(alll_ctx* c, const GroupBest* gb) { return set_track_best(c, gb != nullptr, gb); }

}  // namespace alll

extern "C" {

const char* alll_version(void) { return "alll-mi355x 0.1.0 (abi 1, gfx950)"; }
const char* alll_last_error(void) { return g_err.c_str(); }
void alll_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }

void alll_default_options(alll_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->seed = 1;
    o->max_iters = 0;
    o->device = -1;
    o->n_threads = 1;
    o->rank = 0;
    o->world = 1;
    o->flags = 0;
    o->grid_rounds = 0;
}

int alll_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int alll_comm_unique_id(uint8_t out[128]) {
    if (!out) return fail(ALLL_ERR_INVALID_ARG, "null output");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(out, &id, 128);
    return ALLL_OK;
}

namespace {

// ---- alll_create's steps: alll_layout.cpp plans what the buffers hold; the functions below
// allocate and upload it (the order of the allocations is kept: device addresses follow from it)

int open_device(const alll_options& opt, alll_ctx** pc) {
    int ndev = alll_device_count();
    if (ndev <= 0) return fail(ALLL_ERR_NO_DEVICE, "no HIP device visible");
    int dev = opt.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) return fail(ALLL_ERR_NO_DEVICE, "device %d not visible (%d devices)", dev, ndev);
    if (!is_gfx950(dev)) return fail(ALLL_ERR_NO_DEVICE, "device %d is not gfx950 (MI355X)", dev);
    HIP_TRY(hipSetDevice(dev));

    alll_ctx* c = new (std::nothrow) alll_ctx();
    if (!c) return fail(ALLL_ERR_OOM, "host allocation failed");
    c->device = dev;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        c->n_cu = prop.multiProcessorCount;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
        c->wall_khz = khz;
    auto bail = [&](int rc) { alll_destroy(c); return rc; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "hipStreamCreate failed"));
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(fail(ALLL_ERR_HIP, "hipEventCreate failed"));
    if (hipHostMalloc((void**)&c->h_state, sizeof(DevState), 0) != hipSuccess ||
        hipHostMalloc((void**)&c->h_async, sizeof(DevState), 0) != hipSuccess)
        return bail(fail(ALLL_ERR_OOM, "hipHostMalloc failed"));
    if (hipEventCreateWithFlags(&c->ev_async, hipEventDisableTiming) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "hipEventCreate failed"));
    *pc = c;
    return ALLL_OK;
}

// the context's scalar fields; the loop buffers and the clause view start from the planned ones
void set_shape(alll_ctx* c, const alll_options& opt, const Knobs& kn, const Layout& l) {
    c->opt = opt;
    c->n_vars = l.n_vars;
    c->m = l.m;
    c->n_lits = l.n_lits;
    c->rank = opt.rank;
    c->world = opt.world;
    c->allreduce = (opt.flags & ALLL_FLAG_EXCHANGE_ALLREDUCE) != 0;
    c->use_graph = (opt.flags & ALLL_FLAG_NO_GRAPH) == 0;
    if (!c->use_graph) c->graph_note = "ALLL_FLAG_NO_GRAPH";
    // skewed instances need more rounds before the leftovers are few enough for the
    // single-workgroup tail (power-law 3-SAT at 10M clauses: 10 rounds)
    // (at most GRID_ROUNDS_MAX: the margin of the owner epochs' restart, EP_RESTART_AT, counts on it)
    c->grid_rounds = opt.grid_rounds ? std::min(opt.grid_rounds, GRID_ROUNDS_MAX) : (l.cv.n_hot ? SKEWED_GRID_ROUNDS : DEFAULT_GRID_ROUNDS);
    c->small_u = kn.small_u;
    c->fuse_scatter = kn.fuse_scatter;
    c->tiles_per_rank = l.tiles_per_rank;
    c->n_tiles_padded = l.n_tiles_padded;
    c->own_begin = l.b.own_begin;
    c->own_end = l.b.own_end;
    c->b = l.b;  // (the planned scalars; every pointer still null)
    c->cv = l.cv;
}

// the round robin of T > 1 chunks: scan entries, the batch kernel (fallback of the fixpoint),
// the fixpoint passes and the incremental passes (§4.3.3)
int alloc_round_robin(alll_ctx* c, const Layout& l) {
    if (!l.b.rr_T) return ALLL_OK;
    LoopBuffers& b = c->b;
    const uint64_t m = l.m, L = l.n_lits;
    const size_t nv = l.n_vars;
    const uint32_t T = l.b.rr_T;
    int rc;
    if ((rc = dalloc(c, &b.rr_u, 12 * (size_t)m))) return rc;  // scan entries (k_rr_entries)
    if (l.fixed_k > 0) {  // the hybrid evaluation's lists -> clause-order flags (k_rr_mark)
        if ((rc = dalloc(c, &b.rr_flag, (size_t)l.b.n_tiles * TILE)) || (rc = dalloc(c, &b.rr_tcnt, l.b.n_tiles))) return rc;
    }
    if ((rc = upload(c, &b.rr_sets, l.rr_sets, "chunk"))) return rc;
    if ((rc = dalloc(c, &b.rr_ctl, RR_MW_CTL_WORDS)) || (rc = dalloc(c, &b.rr_gkey, RR_MW_GH)) ||
        (rc = dalloc(c, &b.rr_gmin, RR_MW_GH, 0xFF)) || (rc = dalloc(c, &b.rr_ptr, T)) || (rc = dalloc(c, &b.rr_end, T)))
        return rc;
    if (!l.fp) return ALLL_OK;
    const size_t nblk = m / FP_B + 2;
    if ((rc = dalloc(c, &b.fp_ctl, 1)) || (rc = dalloc(c, &b.fp_in, m + FP_B)) || (rc = dalloc(c, &b.fp_turn, m + 1)) ||
        (rc = dalloc(c, &b.fp_v4, l.fp_slots == 4 ? m + 1 : 1)) ||
        (rc = dalloc(c, &b.fp_sole, (size_t)m * l.fp_slots + 16)) || (rc = dalloc(c, &b.fp_list, 2 * (size_t)m + 2)) ||
        (rc = dalloc(c, &b.fp_tcnt, 2 * FP_G_MAX * ((size_t)m / 256 + 2))) ||  // (round tiles of 256)
        (rc = dalloc(c, &b.fp_owner, nv + 1, 0xFF)) || (rc = dalloc(c, &b.fp_cov, nv + 16)) ||
        (rc = dalloc(c, &b.fp_own0, nv + 1)) || (rc = dalloc(c, &b.fp_vlist, (size_t)L + 1)) ||
        (rc = dalloc(c, &b.fp_heavy, 4 * ((size_t)L / 64 + 2))) ||  // (segments of lists > 64 claims)
        (rc = dalloc(c, &b.fp_pairs, (size_t)L + 1)) ||
        (rc = dalloc(c, &b.fp_blk, 2 * nblk + 2048)) ||  // sums, offsets, changes, earliest changes
        (rc = dalloc(c, &b.fp_sf, T + 1)) || (rc = dalloc(c, &b.fp_bnd, T + 1)) || (rc = dalloc(c, &b.fp_pf, T + 1)) ||
        (rc = dalloc(c, &b.fp_nseg, T)) || (rc = dalloc(c, &b.fp_seg, (size_t)T * T)) || (rc = dalloc(c, &b.fp_erase, T)))
        return rc;
    c->rr_p = std::min<uint32_t>(c->rr_p, b.fp_max);
    c->rr_pre.assign(b.fp_max + 1, nullptr);
    if (hipHostMalloc((void**)&c->h_fp, sizeof(RRFpCtl), 0) != hipSuccess) return fail(ALLL_ERR_OOM, "hipHostMalloc failed");
    if (!l.b.fp_inc) return ALLL_OK;
    if ((rc = dalloc(c, &b.fp_blocker, m + 1, 0xFF)) || (rc = dalloc(c, &b.fp_covby, nv + 1)) ||
        (rc = dalloc(c, &b.fp_sc, nv + 1)) || (rc = dalloc(c, &b.fp_dl, 3 * (size_t)m + 16 * std::min<size_t>(m, 1u << 16) + 64)) ||
        (rc = dalloc(c, &b.fp_dmark, m + 1)) || (rc = dalloc(c, &b.fp_pbits, 2 * ((size_t)m / 8 + 80))) ||
        (rc = dalloc(c, &b.fp_log, FP_LOG_WORDS)) || (rc = dalloc(c, &b.fp_lst, 2 * (size_t)m * l.fp_slots + 16)))
        return rc;
    return ALLL_OK;
}

// the streaming solve with T > 1 threads: generator plans, and the generators of
// SATInstance.h:74-86 (T t_n_clauses = n_clauses / n_threads, the last one takes the remainder), fresh
int alloc_streaming(alll_ctx* c, const alll_options& opt, const Layout& l) {
    const uint32_t T = l.b.srr_T;
    if (!T) return ALLL_OK;
    LoopBuffers& b = c->b;
    int rc;
    if ((rc = dalloc(c, &b.srr_gen, T + 1)) || (rc = dalloc(c, &b.srr_plan, 1)) || (rc = dalloc(c, &b.srr_first, T)))
        return rc;
    if (hipHostMalloc((void**)&c->h_srr, (T + 1) * sizeof(SrrGen), 0) != hipSuccess ||
        hipHostMalloc((void**)&c->h_plan, sizeof(SrrPlan), 0) != hipSuccess ||
        hipHostMalloc((void**)&c->h_first, T * 8ull, 0) != hipSuccess)
        return fail(ALLL_ERR_OOM, "hipHostMalloc failed");
    c->srr_batch = opt.stream_batch;
    c->sgen.resize(T);
    const uint64_t tn = l.m / T;
    for (uint32_t t = 0; t < T; ++t) {
        c->sgen[t].base = (uint64_t)t * tn;
        c->sgen[t].n = t == T - 1 ? l.m - c->sgen[t].base : tn;
    }
    c->use_graph = false;
    c->graph_note = "streaming solve with n_threads > 1: host-planned iterations (eager launches)";
    return ALLL_OK;
}

// the loop's buffers: assignment, violated mask, staging lists, MIS lists
int alloc_loop(alll_ctx* c, const Layout& l) {
    LoopBuffers& b = c->b;
    const size_t slots = (size_t)l.b.n_tiles * TILE;
    const size_t ent_words = (l.fixed_k > 0 ? (size_t)l.fixed_k + 1 : 1);
    int rc;
    if ((rc = dalloc(c, &b.A, b.n_words + 4)) ||  // +4: 16-byte tail loads
        (rc = dalloc(c, &b.vmask, (size_t)l.n_tiles_padded * TILE_WORDS)) ||
        (rc = dalloc(c, &b.tile_cnt, l.b.n_tiles)) || (rc = dalloc(c, &b.mis_cnt, l.b.n_tiles)) ||
        (rc = dalloc(c, &b.stage[0], slots * ent_words)) || (rc = dalloc(c, &b.stage[1], slots * ent_words)) ||
        (rc = dalloc(c, &b.mis, slots)) || (rc = dalloc(c, &b.left, slots * ent_words)) || (rc = dalloc(c, &b.tmis, slots)))
        return rc;
    return ALLL_OK;
}

// reference-RNG mode (alll_refrng.hip): the round's mask, offsets and draws
int alloc_refrng(alll_ctx* c, const alll_options& opt, const Knobs& kn, const Layout& l) {
    if (!l.refrng) return ALLL_OK;
    LoopBuffers& b = c->b;
    // (no clauses: the initial fill still draws; the mask pointer marks the mode)
    if (!l.m) return dalloc(c, &b.rrng_mask, 1);
    const uint64_t nmw = (l.m + 63) / 64, nblk = (nmw + 1023) / 1024;
    int rc;
    if ((rc = dalloc(c, &b.rrng_mask, (size_t)nmw)) || (rc = dalloc(c, &b.rrng_woff, (size_t)nmw)) ||
        (rc = dalloc(c, &b.rrng_bsum, (size_t)nblk + 1)))
        return rc;
    b.rrng_cap = l.n_lits / 63 + 2;  // a round draws ceil(bits / 63), bits <= every literal
    if ((rc = dalloc(c, &b.rrng_stream, (size_t)b.rrng_cap))) return rc;
    // the parallel draws (alll_refrng.hip): engine positions for RRNG_POS_PER_DRAW per draw,
    // jump levels until 2^levels exceeds the most draws a round can take
    const uint64_t nmax = std::min(std::min<uint64_t>(b.rrng_cap * RRNG_POS_PER_DRAW + 64, 0xFFFFFFF0ull), kn.rrng_nmax);
    b.rrng_nmax = (uint32_t)nmax;
    b.rrng_levels = 1;
    while ((1ull << b.rrng_levels) <= b.rrng_cap) ++b.rrng_levels;
    if ((rc = dalloc(c, &b.rrng_jump, (size_t)b.rrng_levels * (nmax + 2))) || (rc = dalloc(c, &b.rrng_val, (size_t)nmax + 2)))
        return rc;
    if (opt.stream_batch && (rc = dalloc(c, &b.rrng_map, (size_t)l.m))) return rc;
    return ALLL_OK;
}

// owner keys, the round robin's claimant bucket tables, cover stamps, statistics, loop state
int alloc_owner_state(alll_ctx* c, const alll_options& opt, const Layout& l) {
    LoopBuffers& b = c->b;
    int rc;
    if ((rc = dalloc(c, &b.owner, (size_t)l.vrange, 0xFF))) return rc;
    if (l.fp) {
        if ((rc = upload(c, &b.fp_soff, l.fp_soff, "claimant bucket")) || (rc = upload(c, &b.fp_breg, l.fp_breg, "claimant bucket")) ||
            (rc = dalloc(c, &b.fp_bfill, l.b.n_bkt)) || (rc = dalloc(c, &b.fp_sv, (size_t)l.b.n_bkt * l.b.bkt_width)) ||
            (rc = dalloc(c, &b.fp_sbcnt, l.b.n_bkt)))
            return rc;
    }
    if ((rc = dalloc(c, &b.cover, (size_t)b.n_words * 32)) ||  // whole words, zero-padded
        (rc = dalloc(c, &b.tile_stats, 2 * (size_t)l.b.n_tiles)) || (rc = dalloc(c, &b.delta, b.n_words)) ||
        (rc = dalloc(c, &b.state, 1)))
        return rc;
    if (opt.flags & ALLL_FLAG_KERNEL_TIMING) {
        std::vector<unsigned long long> init((size_t)TIME_SLOTS * TIME_FIELDS, 0ull);
        for (uint32_t i = 0; i < TIME_SLOTS; ++i) init[(size_t)i * TIME_FIELDS] = ~0ull;
        if ((rc = upload(c, &b.ktime, init, "timing buffer"))) return rc;
    }
    return ALLL_OK;
}

// bucketed LFMIS round 0: the run table and the pair areas
int alloc_round0(alll_ctx* c, const Layout& l) {
    if (!l.bucketed) return ALLL_OK;
    LoopBuffers& b = c->b;
    int rc;
    if ((rc = upload(c, &b.run_t0, l.run_t0, "run table"))) return rc;
    const size_t run_cap = (size_t)b.run_tiles * TILE * l.fixed_k;
    if ((rc = dalloc(c, &b.pairs, (size_t)b.n_runs * run_cap)) || (rc = dalloc(c, &b.runtab, (size_t)b.n_bkt * b.n_runs)) ||
        (rc = dalloc(c, &b.run_rec, (size_t)b.n_runs * RUN_REC_WORDS)))  // (line-aligned: records are one line)
        return rc;
    c->bucket_min_u = l.bucket_min_u;
    return ALLL_OK;
}

// Clause storage: AoS literals (hot variables flagged in bit 31) + offsets, or, for fixed width
// k, a chunk-transposed copy in the planner's locality order; ragged widths add theirs.  The
// big host arrays are planned one at a time and freed once they are on the device.
int upload_clauses(alll_ctx* c, const alll_problem& prob, const Knobs& kn, Layout& l) {
    LoopBuffers& b = c->b;
    ClauseView& cv = c->cv;
    const uint64_t m = l.m, L = l.n_lits;
    const int K = l.fixed_k;
    uint32_t *d_lits = nullptr, *d_t = nullptr;
    int rc;
    if ((rc = dalloc(c, &d_lits, L))) return rc;
    if (K > 0) {
        if ((rc = dalloc(c, &d_t, (m + CHUNK - 1) / CHUNK * CHUNK * K))) return rc;
    } else if ((rc = upload(c, &cv.offs, offsets32(prob), "offset"))) {
        return rc;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(ALLL_ERR_HIP, "memset drain failed");
    flag_hot(prob, l);
    if (l.cv.n_hot && b.fp_ctl && (rc = dalloc(c, &b.fp_hv, (size_t)l.n_vars + 16))) return rc;
    const uint32_t* src = l.flagged.empty() ? prob.literals : l.flagged.data();
    if (L && hipMemcpy(d_lits, src, L * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(ALLL_ERR_HIP, "literal upload failed");
    cv.lits = d_lits;
    if (K > 0) {
        order_fixed(prob, kn, l);
        cv.lit_mask = l.cv.lit_mask;
        cv.id_shift = l.cv.id_shift;
        cv.id_bits = l.cv.id_bits;
        cv.lits_nt = l.cv.lits_nt;
        transpose_fixed(prob, l);
        if (!l.lits_t.empty() && hipMemcpy(d_t + l.t_chunk0 * CHUNK * K, l.lits_t.data(), l.lits_t.size() * 4,
                                           hipMemcpyHostToDevice) != hipSuccess)
            return fail(ALLL_ERR_HIP, "transposed literal upload failed");
        std::vector<uint32_t>().swap(l.lits_t);
        cv.lits_t = d_t;
        if (!cv.id_bits && (rc = upload(c, &cv.perm, l.perm, "permutation"))) return rc;
        window_bases(prob, l);
        if (!l.win_base.empty() && (rc = upload(c, &b.win_base, l.win_base, "window"))) return rc;
    } else if (l.ragged) {
        if ((rc = order_ragged(prob, kn, l))) return fail(rc, "%s", l.err.c_str());
        if ((rc = upload(c, &cv.rg_off, l.rg_off, "ragged layout")) || (rc = upload(c, &cv.rg_lits, l.lits_t, "ragged layout")) ||
            (rc = upload(c, &cv.perm, l.perm, "ragged layout")) ||
            (!l.win_base.empty() && (rc = upload(c, &b.win_base, l.win_base, "ragged layout"))))
            return rc;
        std::vector<uint32_t>().swap(l.lits_t);
    }
    c->perm = std::move(l.perm);
    return ALLL_OK;
}

// RCCL communicator (clause-sharded mode; world 1 with a comm id: a one-rank communicator that
// runs the multi-GPU exchange path on one GPU) and the exchange's buffers
int open_exchange(alll_ctx* c, const alll_options& opt, const Layout& l) {
    LoopBuffers& b = c->b;
    const bool zero_id = l.zero_id;
    int rc;
    if ((c->world > 1 || !zero_id) && (c->cv.k > 0 || c->cv.rg_off)) {
        // the exchange's clause-order mask (this rank laid out its own shard only)
        if ((rc = dalloc(c, &b.cmask, (size_t)c->n_tiles_padded * TILE_WORDS))) return rc;
        if ((rc = dalloc(c, &b.cflag, (size_t)c->tiles_per_rank * TILE + 64))) return rc;
    }
    if (c->world > 1 && (rc = dalloc(c, &b.xcount, 4))) return rc;
    if (c->world > 1 || !zero_id) {
        if (!zero_id) {
            ncclUniqueId id;
            memcpy(&id, opt.comm_id, 128);
            ncclResult_t r = ncclCommInitRank(&c->comm, c->world, id, c->rank);
            if (r != ncclSuccess) return fail(ALLL_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
        } else {
            c->use_graph = false;  // host-staged exchange: eager launches
            c->graph_note = "host-staged exchange (eager launches)";
        }
    }
    return ALLL_OK;
}

}  // namespace

int alll_create(const alll_problem* prob, const alll_options* opt_in, alll_ctx** out) {
    if (!prob || !out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    alll_options opt;
    if (opt_in) opt = *opt_in; else alll_default_options(&opt);
    if (opt.world < 1 || opt.rank < 0 || opt.rank >= opt.world)
        return fail(ALLL_ERR_INVALID_ARG, "bad rank %d / world %d", opt.rank, opt.world);
    if (opt.world > ALLL_MAX_GPU_STATS) return fail(ALLL_ERR_UNSUPPORTED, "world > %d", ALLL_MAX_GPU_STATS);
    // ---- plan on the host: the instance is validated before a device is touched
    const Knobs kn = read_knobs();
    Layout lay;
    int rc;
    if ((rc = plan_instance(*prob, opt, kn, lay))) return fail(rc, "%s", lay.err.c_str());

    alll_ctx* c = nullptr;
    if ((rc = open_device(opt, &c))) return rc;
    auto bail = [&](int rc) { alll_destroy(c); return rc; };
    if (kn.plan_cus) c->n_cu = std::min(c->n_cu, (int)std::min<uint32_t>(kn.plan_cus, 1u << 20));  // (ALLL_PLAN_CUS: tests)
    if ((rc = plan_buckets(*prob, opt, kn, (uint32_t)c->n_cu, lay))) return bail(fail(rc, "%s", lay.err.c_str()));
    set_shape(c, opt, kn, lay);
    if ((rc = alloc_round_robin(c, lay)) || (rc = alloc_streaming(c, opt, lay)) || (rc = alloc_loop(c, lay)) ||
        (rc = alloc_refrng(c, opt, kn, lay)) || (rc = alloc_owner_state(c, opt, lay)) || (rc = alloc_round0(c, lay)) ||
        (rc = upload_clauses(c, *prob, kn, lay)))
        return bail(rc);
    ClauseView& cv = c->cv;
    LoopBuffers& b = c->b;

    // ---- state + initial assignment
    memset(c->h_state, 0, sizeof(DevState));
    c->h_state->limit_eval = ~0ull;
    c->h_state->limit_nores = ~0ull;
    c->h_state->round_next = std::max<uint32_t>(1, lay.epoch0);
    if (c->h_state->round_next >= EP_RESTART_AT) {  // (ALLL_EPOCH0 past the restart point: the tail's rule, on fresh keys)
        c->h_state->round_next = 1;
        c->h_state->ep_restarts = 1;
    }
    c->h_state->best_u = ~0ull;
    if (lay.refrng) c->h_state->rd_state = opt.seed;  // (the random_device stand-in's state)
    if (hipMemcpyAsync(b.state, c->h_state, sizeof(DevState), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "state upload failed"));
    if (launch_init_assignment(b, c->stream) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "init kernel launch failed"));
    {  // kernel attributes (dynamic LDS), outside every stream capture
        const hipError_t e = prepare_kernels(cv, b);
        if (e != hipSuccess) return bail(fail(ALLL_ERR_HIP, "kernel attributes: %s", hipGetErrorString(e)));
    }
    if (b.fp_inc) {
        // the wide repair rounds synchronise their workgroups by a grid barrier: all of them must be
        // resident at once, else every incremental pass would wait for the barrier's timeout and
        // give up; without that guarantee the repair keeps to its one-workgroup rounds
        // (a failed query, or one that reports no resident workgroup at all -- seen in processes that
        // had imported torch, whose bundled HIP runtime answers it differently -- keeps the wide
        // rounds: their barriers time out safely, and are counted)
        int per_cu = 0;
        const uint32_t gw = std::min<uint32_t>(FP_RW_GRID, std::max(1, c->n_cu));
        (void)hipGetLastError();
        const hipError_t e = fp_repair_occupancy(cv, b, &per_cu);
        if (e == hipSuccess && per_cu > 0 && (uint64_t)per_cu * (uint64_t)c->n_cu < gw) b.fp_rw_min = ~0u;
        if (e != hipSuccess) (void)hipGetLastError();
        c->rw_occupancy = e == hipSuccess ? per_cu : -1;
        if (kn.debug_occupancy)  // (diagnostics)
            fprintf(stderr, "alll: k_fp_repair occupancy query %s, %d per CU, %d CUs, wide rounds %s\n",
                    hipGetErrorString(e), per_cu, c->n_cu, b.fp_rw_min == ~0u ? "off" : "on");
    }
    if ((rc = open_exchange(c, opt, lay))) return bail(rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess)
        return bail(fail(ALLL_ERR_HIP, "create: stream sync failed: %s", hipGetErrorString(hipGetLastError())));
    c->hybrid = cv.k > 0 && !(opt.flags & ALLL_FLAG_NO_RANGED);
    char nm[64];
    if (cv.rg_off) snprintf(nm, sizeof nm, "k_eval_ragged");
    else if (c->hybrid) snprintf(nm, sizeof nm, "k_eval_hybrid<%u>", cv.k);
    else if (cv.k) snprintf(nm, sizeof nm, "k_eval_fixed<%u>", cv.k);
    else snprintf(nm, sizeof nm, "k_eval_csr");
    c->eval_name = nm;
    *out = c;
    return ALLL_OK;
}

int alll_destroy(alll_ctx* c) {
    if (!c) return ALLL_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_graphs(c);
    if (c->h_fp) (void)hipHostFree(c->h_fp);
    if (c->h_srr) (void)hipHostFree(c->h_srr);
    if (c->h_plan) (void)hipHostFree(c->h_plan);
    if (c->h_first) (void)hipHostFree(c->h_first);
    for (uint32_t* p : {c->b.srr_bcnt, c->b.srr_ent, c->b.srr_step})
        if (p) (void)hipFree(p);
    if (c->comm) ncclCommDestroy(c->comm);
    for (void* p : c->allocs) (void)hipFree(p);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->h_async) (void)hipHostFree(c->h_async);
    if (c->ev_async) (void)hipEventDestroy(c->ev_async);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return ALLL_OK;
}

int alll_set_host_exchange(alll_ctx* c, alll_exchange_fn fn, void* user) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    c->xfn = fn;
    c->xuser = user;
    c->use_graph = false;
    c->graph_note = "host-staged exchange (eager launches)";
    return ALLL_OK;
}

int alll_solve(alll_ctx* c, alll_stats* st) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = read_state(c);
    if (rc) return rc;
    // (streaming solve: max_iters counts stream iterations; the last one's check is one more
    // evaluation pass, which does not resample)
    const uint64_t cap = c->opt.max_iters ? c->opt.max_iters + (c->opt.stream_batch ? 1 : 0) : ~0ull;
    if (c->h_state->done != 1) {
        if ((rc = write_limits(c, cap, cap))) return rc;
        uint64_t batch = 1;
        for (;;) {
            if ((rc = launch_iterations(c, batch))) return rc;
            if ((rc = read_state(c))) return rc;
            if (c->h_state->done || c->h_state->n_iter >= cap) break;
            batch = std::min<uint64_t>(batch * 2, 64);
        }
    }
    alll_stats tmp;
    if ((rc = fill_stats(c, st ? st : &tmp))) return rc;
    if (c->h_state->done != 1)
        return fail(ALLL_ERR_MAX_ITERS, "not solved after %llu eval passes (%llu clauses violated)",
                    (unsigned long long)c->h_state->n_iter, (unsigned long long)c->h_state->u_total);
    return ALLL_OK;
}

int alll_run(alll_ctx* c, uint64_t n_iters, alll_stats* st) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (n_iters) {
        // no host round trip: the limit is set on the device (n_iter + n_iters), stream-ordered
        // before the iterations; after convergence every kernel is gated off
        HIP_TRY(launch_set_limits(c->b, n_iters, c->stream));
        if ((rc = launch_iterations(c, n_iters))) return rc;
    }
    if (st) return fill_stats(c, st);
    return ALLL_OK;
}

int alll_get_stats(alll_ctx* c, alll_stats* st) {
    if (!c || !st) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    return fill_stats(c, st);
}

int alll_synchronize(alll_ctx* c) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALLL_OK;
}

int alll_verify(alll_ctx* c, int* valid, uint64_t* n_violated) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    // every rank evaluates its own shard (the only one laid out for its evaluation); the
    // counts are summed over the ranks
    HIP_TRY(eval_launch(c, c->own_begin, c->own_end, false));
    HIP_TRY(launch_reduce(c->b, 1, c->stream));
    uint64_t count = 0;
    if (c->world > 1) {
        // the mask alll_get_violated_mask returns on sharded runs (clause order: cmask, or the
        // CSR evaluation's own bitmask) refreshed from this evaluation: the own shard's piece,
        // then the other shards' pieces all-gathered
        const size_t words = (size_t)c->tiles_per_rank * TILE_WORDS;
        uint64_t* mask = c->b.cmask ? c->b.cmask : c->b.vmask;
        if (c->b.cmask) HIP_TRY(launch_cmark(c->cv, c->b, words, c->rank, false, c->stream));
        if (c->comm) {
            NCCL_TRY(ncclAllGather(mask + (size_t)c->rank * words, mask, words, ncclUint64, c->comm, c->stream));
        } else {
            int rc = host_exchange(c, ALLL_XCHG_ALLGATHER, mask, words * 8, (size_t)c->rank * words * 8);
            if (rc) return rc;
        }
    }
    if (c->world > 1) {
        if (c->comm) {
            NCCL_TRY(ncclAllReduce(c->b.xcount, c->b.xcount, 1, ncclUint32, ncclSum, c->comm, c->stream));
        } else {
            int rc = host_exchange(c, ALLL_XCHG_ALLREDUCE_SUM_U32, c->b.xcount, 4, 0);
            if (rc) return rc;
        }
        uint32_t x = 0;
        HIP_TRY(hipMemcpyAsync(&x, c->b.xcount, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        count = x;
    }
    int rc = read_state(c);
    if (rc) return rc;
    if (c->world == 1) count = c->h_state->count_out;
    if (valid) *valid = count == 0;
    if (n_violated) *n_violated = count;
    return ALLL_OK;
}

int alll_get_assignment_words(alll_ctx* c, uint32_t* out, uint64_t n_words) {
    if (!c || (!out && c->b.n_words)) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < c->b.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", c->b.n_words);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->b.n_words) HIP_TRY(hipMemcpy(out, c->b.A, c->b.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_set_assignment_words(alll_ctx* c, const uint32_t* in, uint64_t n_words) {
    if (!c || (!in && c->b.n_words)) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n_words < c->b.n_words) return fail(ALLL_ERR_INVALID_ARG, "need %u words", c->b.n_words);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint32_t> w(in, in + c->b.n_words);
    if (!w.empty() && (c->n_vars & 31)) w.back() &= (1u << (c->n_vars & 31)) - 1u;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->b.n_words) HIP_TRY(hipMemcpy(c->b.A, w.data(), c->b.n_words * 4ull, hipMemcpyHostToDevice));
    c->hint_u = ~0ull;  // the next pass's violated count is unknown: no small-set variant
    c->async_pending = false;
    return ALLL_OK;
}

int alll_get_assignment(alll_ctx* c, uint8_t* out, uint64_t n) {
    if (!c || (!out && c->n_vars)) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n < c->n_vars) return fail(ALLL_ERR_INVALID_ARG, "need %u bytes", c->n_vars);
    std::vector<uint32_t> w(c->b.n_words);
    int rc = alll_get_assignment_words(c, w.data(), w.size());
    if (rc) return rc;
    for (uint32_t v = 0; v < c->n_vars; ++v) out[v] = (w[v >> 5] >> (v & 31)) & 1u;
    return ALLL_OK;
}

int alll_set_assignment(alll_ctx* c, const uint8_t* in, uint64_t n) {
    if (!c || (!in && c->n_vars)) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    if (n < c->n_vars) return fail(ALLL_ERR_INVALID_ARG, "need %u bytes", c->n_vars);
    std::vector<uint32_t> w(c->b.n_words, 0u);
    for (uint32_t v = 0; v < c->n_vars; ++v)
        if (in[v]) w[v >> 5] |= 1u << (v & 31);
    return alll_set_assignment_words(c, w.data(), w.size());
}

int alll_set_var_thresholds(alll_ctx* c, const uint32_t* thr, uint64_t n) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: the context belongs to a group "
                                                  "(alll_group_set_var_thresholds)");
    int rc;
    if ((rc = bias_supported(c))) return rc;
    if (thr && n != c->n_vars)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for %u variables", (unsigned long long)n,
                    c->n_vars);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = read_state(c))) return rc;  // (drains the stream)
    if (c->h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds are set before the first iteration (%llu made)",
                    (unsigned long long)c->h_state->n_iter);
    LoopBuffers& b = c->b;
    if (thr && b.n_words) {
        // the context's own copy, padded with zeros to whole words (k_resample_biased loads 16 per lane)
        if (!c->d_thr && (rc = dalloc(c, &c->d_thr, (size_t)b.n_words * 32))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(c->d_thr, thr, (size_t)c->n_vars * 4, hipMemcpyHostToDevice));
        b.thr = c->d_thr;
    } else {
        b.thr = nullptr;
    }
    drop_graphs(c);  // (none is captured before the first iteration; one would hold the old pointer)
    HIP_TRY(launch_fill_words(b.A, b.n_words, b.n_vars, b.thr, b.seed, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ctx_assignment_changed(c);
    return ALLL_OK;
}

// Unit propagation of the pins: the rounds run on the context's own thresholds,
// then the assignment is the biased fill of the propagated thresholds, as after alll_set_var_thresholds.
int alll_propagate_pins(alll_ctx* c, uint64_t max_rounds, alll_propagate_result* res) {
    if (!c || !res) return fail(ALLL_ERR_INVALID_ARG, "propagate pins: null argument");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "propagate pins: the context belongs to a group "
                                                  "(alll_group_propagate_pins)");
    int rc;
    if ((rc = bias_supported(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = read_state(c))) return rc;  // (drains the stream)
    if (c->h_state->n_iter != 0)
        return fail(ALLL_ERR_INVALID_ARG, "propagate pins: allowed before the first iteration only (%llu made)",
                    (unsigned long long)c->h_state->n_iter);
    LoopBuffers& b = c->b;
    if (!b.thr || !c->d_thr)
        return fail(ALLL_ERR_INVALID_ARG, "propagate pins: the context has no thresholds (alll_set_var_thresholds first)");
    PropArgs a{};
    a.lits = c->cv.lits;
    a.offs = c->cv.offs;
    a.m = c->cv.m;
    a.k = c->cv.k;
    a.n_vars = b.n_vars;
    a.n_words = b.n_words;
    a.n_items = 1;
    a.thr = c->d_thr;
    const uint8_t on = 1;
    if ((rc = prop_drive(a, &on, max_rounds, res, c->stream))) return rc;
    HIP_TRY(launch_fill_words(b.A, b.n_words, b.n_vars, b.thr, b.seed, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ctx_assignment_changed(c);
    return ALLL_OK;
}

int alll_get_var_thresholds(alll_ctx* c, uint32_t* out, uint64_t n) {
    if (!c || (!out && n)) return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: null argument");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: the context belongs to a group "
                                                  "(alll_group_get_var_thresholds)");
    if (!c->b.thr || !c->d_thr) return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: the context has none");
    if (n != c->n_vars)
        return fail(ALLL_ERR_INVALID_ARG, "variable thresholds: %llu entries for %u variables", (unsigned long long)n,
                    c->n_vars);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(out, c->d_thr, (size_t)n * 4, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

// Split scores under the context's thresholds: a pass of its own kernels and
// scratch on the drained stream; nothing of the context is written.
int alll_var_scores(alll_ctx* c, uint64_t* scores, uint64_t n_scores, alll_split_result* res) {
    if (!c || !res) return fail(ALLL_ERR_INVALID_ARG, "var scores: null argument");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "var scores: the context belongs to a group (alll_group_var_scores)");
    int rc;
    if ((rc = bias_supported(c))) return rc;
    if (scores && n_scores != 2ull * c->n_vars)
        return fail(ALLL_ERR_INVALID_ARG, "var scores: %llu entries for the %llu literals of %u variables",
                    (unsigned long long)n_scores, 2ull * c->n_vars, c->n_vars);
    HIP_TRY(hipSetDevice(c->device));
    const LoopBuffers& b = c->b;
    PropArgs a{};
    a.lits = c->cv.lits;
    a.offs = c->cv.offs;
    a.m = c->cv.m;
    a.k = c->cv.k;
    a.n_vars = b.n_vars;
    a.n_words = b.n_words;
    a.n_items = 1;
    a.thr = (b.thr && c->d_thr) ? c->d_thr : nullptr;
    std::vector<uint64_t> S;
    if ((rc = score_drive(a, {0u, c->n_vars}, res, scores ? &S : nullptr, c->stream))) return rc;
    if (scores && c->n_vars) memcpy(scores, S.data(), 16ull * c->n_vars);
    return ALLL_OK;
}

// Failed-literal probing under the context's thresholds: rounds of its own kernels
// and scratch on the drained stream; nothing of the context is written.
int alll_probe_literals(alll_ctx* c, const uint32_t* probes, uint64_t n_probes, uint64_t max_rounds,
                        alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, uint64_t n_words) {
    if (!c || !results || (!probes && n_probes)) return fail(ALLL_ERR_INVALID_ARG, "probe literals: null argument");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "probe literals: the context belongs to a group (no group form)");
    int rc;
    if ((rc = bias_supported(c))) return rc;
    const LoopBuffers& b = c->b;
    if ((pm_rows || pv_rows) && n_words != b.n_words)
        return fail(ALLL_ERR_INVALID_ARG, "probe literals: rows of %llu words for the %u of the assignment",
                    (unsigned long long)n_words, b.n_words);
    for (uint64_t p = 0; p < n_probes; ++p)
        if (probes[p] >= 2ull * c->n_vars)
            return fail(ALLL_ERR_INVALID_ARG, "probe literals: probe %llu is literal %u of %u variables",
                        (unsigned long long)p, probes[p], c->n_vars);
    if (n_probes == 0) return ALLL_OK;
    HIP_TRY(hipSetDevice(c->device));
    PropArgs a{};
    a.lits = c->cv.lits;
    a.offs = c->cv.offs;
    a.m = c->cv.m;
    a.k = c->cv.k;
    a.n_vars = b.n_vars;
    a.n_words = b.n_words;
    a.n_items = 1;
    a.thr = (b.thr && c->d_thr) ? c->d_thr : nullptr;
    return probe_drive(a, probes, n_probes, max_rounds, results, pm_rows, pv_rows, c->stream);
}

// The residual formula under the context's thresholds: a pass of its own kernels
// and scratch on the drained stream; nothing of the context is written.
int alll_residual(alll_ctx* c, alll_residual_result* res, uint64_t* offsets, uint32_t* literals, uint32_t* var_map,
                  uint64_t* clause_map, uint32_t* thr_out) {
    if (!c || !res) return fail(ALLL_ERR_INVALID_ARG, "residual: null argument");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "residual: the context belongs to a group (alll_group_residual)");
    int rc;
    if ((rc = bias_supported(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const LoopBuffers& b = c->b;
    PropArgs a{};
    a.lits = c->cv.lits;
    a.offs = c->cv.offs;
    a.m = c->cv.m;
    a.k = c->cv.k;
    a.n_vars = b.n_vars;
    a.n_words = b.n_words;
    a.n_items = 1;
    a.thr = (b.thr && c->d_thr) ? c->d_thr : nullptr;
    const std::vector<ResidItem> items{ResidItem{0u, c->n_vars, 0u, b.n_words, 0u, (uint32_t)c->cv.m}};
    return resid_drive(a, items, c->n_lits, res, ResidOut{offsets, literals, var_map, clause_map, thr_out}, c->stream);
}

int alll_track_best(alll_ctx* c, int on) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "best-assignment tracking: the context belongs to a group "
                                                  "(alll_group_track_best)");
    int rc;
    if ((rc = track_supported(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return set_track_best(c, on != 0, nullptr);
}

int alll_get_best(alll_ctx* c, uint64_t* n_violated, uint64_t* iteration, uint32_t* words, uint64_t n_words) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    if (c->grp) return fail(ALLL_ERR_INVALID_ARG, "best assignment: the context belongs to a group (alll_group_get_best)");
    if (!c->b.A_best)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: the context does not track it (alll_track_best before the "
                                          "first iteration)");
    if (words && n_words != c->b.n_words)
        return fail(ALLL_ERR_INVALID_ARG, "best assignment: %llu words for the %u of the assignment",
                    (unsigned long long)n_words, c->b.n_words);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = read_state(c)) return rc;  // (drains the stream)
    if (n_violated) *n_violated = c->h_state->best_u;
    if (iteration) *iteration = c->h_state->best_iter;
    // (before any pass the words are left untouched)
    if (words && c->h_state->best_iter && c->b.n_words)
        HIP_TRY(hipMemcpy(words, c->b.A_best, c->b.n_words * 4ull, hipMemcpyDeviceToHost));
    return ALLL_OK;
}

int alll_get_violated_mask(alll_ctx* c, uint64_t* out, uint64_t n_words) {
    if (!c) return fail(ALLL_ERR_INVALID_ARG, "null context");
    const uint64_t need = (c->m + 63) / 64;
    if (n_words < need || (!out && need)) return fail(ALLL_ERR_INVALID_ARG, "need %llu words", (unsigned long long)need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->b.cmask && c->world > 1) {  // clause-sharded: the last all-gathered clause-order mask
        if (need) HIP_TRY(hipMemcpy(out, c->b.cmask, need * 8, hipMemcpyDeviceToHost));
        if (c->m & 63) out[need - 1] &= (1ull << (c->m & 63)) - 1ull;
    } else if (!c->perm.empty()) {  // fixed width: device bits are chunk ballots in evaluation order
        std::vector<uint64_t> ev((c->m + CHUNK - 1) / CHUNK * 4);
        HIP_TRY(hipMemcpy(ev.data(), c->b.vmask, ev.size() * 8, hipMemcpyDeviceToHost));
        std::fill(out, out + need, 0ull);
        for (uint64_t p = 0; p < c->m; ++p) {
            const uint64_t w = (p / CHUNK) * 4 + (p & 3), bit = (p % CHUNK) >> 2;
            if ((ev[w] >> bit) & 1ull) out[c->perm[p] >> 6] |= 1ull << (c->perm[p] & 63);
        }
    } else {
        if (need) HIP_TRY(hipMemcpy(out, c->b.vmask, need * 8, hipMemcpyDeviceToHost));
        if (c->m & 63) out[need - 1] &= (1ull << (c->m & 63)) - 1ull;
    }
    return ALLL_OK;
}

int alll_get_mis(alll_ctx* c, uint32_t* out, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = read_state(c);
    if (rc) return rc;
    const uint32_t nt = c->b.n_tiles;
    std::vector<uint32_t> cnt(nt);
    if (nt) HIP_TRY(hipMemcpy(cnt.data(), c->b.mis_cnt, nt * 4ull, hipMemcpyDeviceToHost));
    std::vector<uint32_t> all;
    std::vector<uint32_t> buf;
    for (uint32_t t = 0; t < nt; ++t) {
        if (!cnt[t]) continue;
        buf.resize(cnt[t]);
        HIP_TRY(hipMemcpy(buf.data(), c->b.mis + (size_t)t * TILE, cnt[t] * 4ull, hipMemcpyDeviceToHost));
        all.insert(all.end(), buf.begin(), buf.end());
    }
    if (c->h_state->tmis_cnt) {
        buf.resize(c->h_state->tmis_cnt);
        HIP_TRY(hipMemcpy(buf.data(), c->b.tmis, buf.size() * 4ull, hipMemcpyDeviceToHost));
        all.insert(all.end(), buf.begin(), buf.end());
    }
    std::sort(all.begin(), all.end());
    *n_out = all.size();
    if (out) {
        if (cap < all.size()) return fail(ALLL_ERR_INVALID_ARG, "need capacity %zu", all.size());
        std::copy(all.begin(), all.end(), out);
    }
    return ALLL_OK;
}

int alll_bench_eval(alll_ctx* c, int reps, double* avg_ms, uint64_t* n_violated) {
    if (!c || reps < 1) return fail(ALLL_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(eval_launch(c, c->own_begin, c->own_end, false));  // warm
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    for (int i = 0; i < reps; ++i) HIP_TRY(eval_launch(c, c->own_begin, c->own_end, false));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipEventSynchronize(c->ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (avg_ms) *avg_ms = ms / reps;
    if (n_violated) {
        int valid = 0;
        int rc = alll_verify(c, &valid, n_violated);
        if (rc) return rc;
    }
    return ALLL_OK;
}

int alll_profile(alll_ctx* c, uint64_t n_iters, alll_phase_times* out) {
    if (!c || !out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    memset(out, 0, sizeof(*out));
    int rc = read_state(c);
    if (rc) return rc;
    if (c->h_state->done == 1) return ALLL_OK;
    if ((rc = write_limits(c, c->h_state->n_iter + n_iters, ~0ull))) return rc;
    double acc[4] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < n_iters; ++i) {
        if (c->b.srr_T) rc = launch_srr_iteration(c, c->ev);
        else if (c->b.rr_T && c->b.fp_ctl) rc = launch_rr_iteration(c, c->ev);
        else rc = enqueue_iteration(c, c->ev, round0_variant(c));
        if (rc) return rc;
        HIP_TRY(hipEventSynchronize(c->ev[4]));
        float t;
        for (int p = 0; p < 4; ++p) {
            HIP_TRY(hipEventElapsedTime(&t, c->ev[p], c->ev[p + 1]));
            acc[p] += t;
        }
    }
    out->iterations = n_iters;
    out->eval_ms = acc[0] / n_iters;
    out->exchange_ms = acc[1] / n_iters;
    out->mis_ms = acc[2] / n_iters;
    out->resample_ms = acc[3] / n_iters;
    out->total_ms = (acc[0] + acc[1] + acc[2] + acc[3]) / n_iters;
    return ALLL_OK;
}

int alll_loop_times(alll_ctx* c, uint64_t first_iter, uint64_t n_iters, alll_phase_times* out) {
    if (!c || !out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    if (!c->b.ktime) return fail(ALLL_ERR_INVALID_ARG, "created without ALLL_FLAG_KERNEL_TIMING");
    HIP_TRY(hipSetDevice(c->device));
    int rc = read_state(c);
    if (rc) return rc;
    const uint64_t done = c->h_state->n_iter;  // slots of iterations < done are complete
    if (first_iter + n_iters > done) n_iters = done > first_iter ? done - first_iter : 0;
    if (done > TIME_SLOTS && first_iter < done - TIME_SLOTS) {
        const uint64_t lo = done - TIME_SLOTS;
        n_iters = first_iter + n_iters > lo ? first_iter + n_iters - lo : 0;
        first_iter = lo;
    }
    if (n_iters == 0) return ALLL_OK;
    std::vector<unsigned long long> t((size_t)TIME_SLOTS * TIME_FIELDS);
    HIP_TRY(hipMemcpy(t.data(), c->b.ktime, t.size() * 8, hipMemcpyDeviceToHost));
    const double tick_ms = 1.0 / c->wall_khz;
    auto slot = [&](uint64_t i) { return &t[(size_t)(i % TIME_SLOTS) * TIME_FIELDS]; };
    double se = 0, sx = 0, sm = 0, sr = 0, st = 0;
    uint64_t ne = 0, nm = 0, nt = 0;
    for (uint64_t i = first_iter; i < first_iter + n_iters; ++i) {
        const unsigned long long* a = slot(i);
        if (a[0] == ~0ull || a[1] < a[0]) continue;  // not evaluated (converged / gated)
        se += (a[1] - a[0]) * tick_ms; ++ne;
        if (a[2] >= a[1]) sx += (a[2] - a[1]) * tick_ms;
        if (a[3] && a[3] >= a[2]) {
            sm += (a[3] - a[2]) * tick_ms; ++nm;
            // resample + launch gaps: LFMIS end to the next iteration's evaluation start
            const unsigned long long* z = slot(i + 1);
            if (i + 1 < done && z[0] != ~0ull && z[0] >= a[3]) {
                sr += (z[0] - a[3]) * tick_ms;
                st += (z[0] - a[0]) * tick_ms;
                ++nt;
            }
        }
    }
    out->iterations = ne;
    if (ne) { out->eval_ms = se / ne; out->exchange_ms = sx / ne; }
    if (nm) out->mis_ms = sm / nm;
    if (nt) { out->resample_ms = sr / nt; out->total_ms = st / nt; }
    return ALLL_OK;
}

int alll_shard_plan(uint64_t n_clauses, int world, int rank, uint64_t* clause_begin,
                    uint64_t* clause_end, uint64_t* mask_words_per_rank) {
    if (world < 1 || rank < 0 || rank >= world) return fail(ALLL_ERR_INVALID_ARG, "bad rank/world");
    const uint64_t n_tiles = (n_clauses + TILE - 1) / TILE;
    uint64_t tpr = (n_tiles + world - 1) / world;
    if (tpr == 0) tpr = 1;
    const uint64_t tb = std::min<uint64_t>(n_tiles, (uint64_t)rank * tpr);
    const uint64_t te = std::min<uint64_t>(n_tiles, tb + tpr);
    if (clause_begin) *clause_begin = std::min<uint64_t>(n_clauses, tb * TILE);
    if (clause_end) *clause_end = std::min<uint64_t>(n_clauses, te * TILE);
    if (mask_words_per_rank) *mask_words_per_rank = tpr * TILE_WORDS;
    return ALLL_OK;
}

int alll_plan_multi_gpu(uint64_t n_clauses, uint64_t n_literals, uint32_t n_vars, int world,
                        alll_multi_plan* out) {
    if (!out || world < 1) return fail(ALLL_ERR_INVALID_ARG, "bad arguments");
    memset(out, 0, sizeof(*out));
    const double m = (double)n_clauses, G = (double)world;
    const double k_avg = n_clauses ? (double)n_literals / m : 0.0;
    // evaluation: the literal stream + assignment + bitmask bytes (alll_eval_bytes) at the rate
    // the evaluation kernel reaches on one MI355X: 4.3 TB/s while the stream fits the 256 MB
    // Infinity Cache (M: 121.6 MB in 28 us), 3.3 TB/s beyond it (C4: 1,556 MB in 467 us)
    const double bytes = 4.0 * (double)n_literals + (double)n_vars / 8.0 + m / 8.0;
    const double eval_us = bytes / (bytes <= 200e6 ? 4.3e6 : 3.3e6);
    // violated clauses: a uniform assignment violates a k-clause with probability 2^-k
    const double u = m * std::pow(2.0, -k_avg);
    out->eval_us_1gpu = eval_us;
    out->eval_saved_us = eval_us * (1.0 - 1.0 / G);
    out->violated_est = u;
    if (world > 1) {
        // own shard's marking (k_cmark: 14.4 us for 0.75M violated clauses; k_cpack: 7.4 us per
        // 10M clauses), the in-graph all-gather (15 us latency + m/8 bytes at ~300 GB/s), the
        // other shards' violated clauses collected (4.5 us + a 64-byte line each at ~6 TB/s),
        // the round-0 scatter and reduce the exchange path runs unfused (2.6 + 4.6 us)
        const double mark = 14.4 * (u / G) / 0.75e6 + 7.4 * (m / G) / 10e6;
        const double gather = 15.0 + (m / 8.0) / 300e3;
        const double collect = 4.5 + u * (G - 1.0) / G * 64.0 / 6e6;
        out->exchange_us = mark + gather + collect + 2.6 + 4.6;
    }
    out->plan = world > 1 && out->eval_saved_us > out->exchange_us ? ALLL_PLAN_SHARD : ALLL_PLAN_REPLICATE;
    return ALLL_OK;
}

uint64_t alll_eval_bytes(alll_ctx* c) {
    // B_eval = 4 L + 4 (m+1) [CSR offsets only] + ceil(n/8) + ceil(m/8),
    // for this rank's clause shard.
    if (!c) return 0;
    const uint64_t cb = (uint64_t)c->own_begin * TILE;
    const uint64_t ce = std::min<uint64_t>(c->m, (uint64_t)c->own_end * TILE);
    const uint64_t ms = ce > cb ? ce - cb : 0;
    const uint64_t lits = c->cv.k ? ms * c->cv.k : (c->m ? (c->n_lits * ms) / c->m : 0);
    return 4 * lits + (c->cv.k ? 0 : 4 * (ms + 1)) + (c->n_vars + 7) / 8 + (ms + 7) / 8;
}

int alll_layout(alll_ctx* c) { return c ? (int)c->cv.k : -1; }

int alll_rr_pass_log(alll_ctx* c, uint32_t* out, uint32_t n_words) {
    if (!c || (!out && n_words)) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t have = c->b.fp_log ? FP_LOG_WORDS : 0;
    const uint32_t nw = std::min(n_words, have);
    if (nw) HIP_TRY(hipMemcpy(out, c->b.fp_log, nw * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t i = nw; i < n_words; ++i) out[i] = 0;
    return (int)nw;
}

int64_t alll_rr_barrier_timeouts(alll_ctx* c) {
    if (!c) return -1;
    if (!c->b.fp_ctl) return 0;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    RRFpCtl ctl;
    if (hipMemcpy(&ctl, c->b.fp_ctl, sizeof ctl, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return ctl.rw_timeouts;
}

int alll_epoch_counters(alll_ctx* c, uint64_t out[4]) {
    if (!c || !out) return fail(ALLL_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    DevState st;
    HIP_TRY(hipMemcpy(&st, c->b.state, sizeof st, hipMemcpyDeviceToHost));
    out[0] = out[1] = 0;
    if (c->b.fp_ctl) {
        RRFpCtl ctl;
        HIP_TRY(hipMemcpy(&ctl, c->b.fp_ctl, sizeof ctl, hipMemcpyDeviceToHost));
        out[0] = ctl.ep_restarts;
        out[1] = ctl.ep_fails;
    }
    out[2] = st.ep_restarts;
    out[3] = st.round_next;
    return ALLL_OK;
}

int alll_comm_size(alll_ctx* c) {
    if (!c) return -1;
    if (!c->comm) return c->world;
    int n = 0;
    if (ncclCommCount(c->comm, &n) != ncclSuccess) return -1;
    return n;
}

const char* alll_eval_kernel(alll_ctx* c) { return c ? c->eval_name.c_str() : ""; }

int alll_uses_graphs(alll_ctx* c, const char** why) {
    if (!c) return -1;
    if (why) *why = c->graph_note.c_str();
    return c->use_graph ? 1 : 0;
}

}  // extern "C"
