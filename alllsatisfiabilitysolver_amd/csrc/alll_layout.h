// alll_layout.h -- host-only planning of what alll_create puts on the device: validation, the
// hot-variable set, the bucket plans and the evaluation orders, from the CSR instance alone.
// No HIP, RCCL or alll_ctx access: the unit builds with a plain host compiler (tests/cpp/
// layout_dump.cpp runs it under the sanitizers).  alll_runtime.cpp allocates and uploads.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "alll.h"
#include "alll_internal.h"

namespace alll {

// Every environment knob of alll_create (tuning, tests), read at every create.
struct Knobs {
    uint64_t small_u = 8192;            // ALLL_SMALL_U
    bool fuse_scatter = true;           // ALLL_FUSE_SCATTER
    uint32_t win_words = LDS_WORDS;     // ALLL_WIN_WORDS: [16, LDS_WORDS], a multiple of 8
    bool rr_fp = true;                  // ALLL_RR_FP
    uint32_t rr_fp_max = FP_MAX_DEFAULT;  // ALLL_RR_FP_MAX: [1, 250]
    bool rr_inc = true;                 // ALLL_RR_INC
    uint32_t rr_rep_cap = FP_REP_CAP;   // ALLL_RR_REP_CAP: >= 1
    uint32_t rr_rw_min = FP_RW_MIN;     // ALLL_RR_RW_MIN: >= 0
    unsigned long long rr_rw_timeout = FP_RW_TIMEOUT;  // ALLL_RR_RW_TIMEOUT
    uint32_t rr_inc_after = 1;          // ALLL_RR_INC_AFTER: >= 1
    uint32_t rr_ep_budget = 0;          // ALLL_RR_EP_BUDGET: >= FP_EP_CAP_MIN, 0 unset (no cap)
    uint32_t epoch0 = 1;                // ALLL_EPOCH0: the first owner epoch of the one-set loop (32-bit)
    uint64_t rrng_nmax = ~0ull;         // ALLL_RRNG_NMAX: >= 8 (unset or empty: no cap)
    bool has_bucket_min_u = false;      // ALLL_BUCKET_MIN_U
    uint64_t bucket_min_u = 0;
    int eval_windows = -1;              // ALLL_EVAL_WINDOWS: 0 / 1, -1 unset
    bool packed_ids = true;             // ALLL_PACKED_IDS
    int eval_nt = -1;                   // ALLL_EVAL_NT: 0 / 1, -1 unset
    bool debug_occupancy = false;       // ALLL_DEBUG_OCCUPANCY
    uint32_t plan_cus = 0;              // ALLL_PLAN_CUS: >= 1, 0 unset (the device's compute units)
};
Knobs read_knobs();

// Host threads for the layout work: the process's CPU affinity, at most 16 (the CPU share of
// one GPU on the MI355X boxes) or OMP_NUM_THREADS when set.
unsigned host_threads();

// What the stages below decide.  A failing stage returns its ALLL_ERR_* code and leaves the
// message in err.
struct Layout {
    std::string err;
    // The scalar fields of the loop buffers and the clause view that the plan decides (shape,
    // tiles, own shard, vmix, buckets, runs, round-robin limits, packed ids); pointers stay null.
    LoopBuffers b{};
    ClauseView cv{};
    // ---- plan_instance
    uint64_t m = 0, n_lits = 0;
    uint32_t n_vars = 0;
    int width = -1;       // common clause width (-1: no clauses, 0: ragged)
    int fixed_k = 0;      // width of the fixed-width (chunk-transposed) layout, 0: CSR
    bool refrng = false, zero_id = true;  // reference-RNG mode; opt.comm_id is all zero
    bool ragged = false;  // ragged widths evaluated from the chunk-transposed copy (order_ragged)
    uint32_t tiles_per_rank = 0, n_tiles_padded = 0;  // shards: contiguous tile ranges
    uint64_t own_c0 = 0, own_c1 = 0;      // the own shard's clauses
    std::vector<uint32_t> rr_sets;        // b.rr_T + 1 chunk starts
    std::vector<uint8_t> is_hot;          // per variable (empty: no hot variable)
    bool fp = false;                      // round robin by fixpoint
    uint32_t fp_slots = 8;                // variable slots per scan entry: 4 when every width <= 4
    uint32_t epoch0 = 1;                  // DevState::round_next at create (before the restart rule, EP_RESTART_AT)
    // ---- plan_buckets
    uint64_t vrange = 0;                  // owner slots / bucketed variable keys
    std::vector<uint32_t> fp_soff, fp_breg;  // round robin: claimant list starts, bucket regions
    bool skewed = false;                  // bucketed round 0 refused: one bucket would hold most pairs
    bool bucketed = false;                // bucketed round 0 (b.run_tiles, b.n_runs, run_t0, bucket_min_u)
    std::vector<uint32_t> run_t0;         // first tile of every run (+ end)
    uint64_t bucket_min_u = 0;
    // ---- flag_hot / order_fixed / transpose_fixed / window_bases / order_ragged
    std::vector<uint32_t> flagged;        // the literals with bit 31 on the hot ones (empty: none)
    std::vector<uint32_t> perm;           // evaluation position -> clause id
    bool windows = false;
    uint64_t t_chunk0 = 0;                // fixed width: first chunk of lits_t
    std::vector<uint32_t> lits_t;         // own chunks, transposed (fixed width) / rg_lits (ragged)
    std::vector<uint32_t> win_base;       // per tile (empty: no windows)
    std::vector<uint32_t> rg_off;         // ragged: chunk offsets (units of CHUNK words)
};

// Validation (before any device is touched), shape, shards, chunk starts, streaming inverse,
// hot variables, the round robin's fixpoint decision.
int plan_instance(const alll_problem& prob, const alll_options& opt, const Knobs& kn, Layout& l);
// vmix, the round robin's claimant buckets and the plan of the bucketed LFMIS round 0.
int plan_buckets(const alll_problem& prob, const alll_options& opt, const Knobs& kn, uint32_t n_cu, Layout& l);
void flag_hot(const alll_problem& prob, Layout& l);
std::vector<uint32_t> offsets32(const alll_problem& prob);
// Fixed width: perm and the packed-id decision; the own shard's transposed literals; the windows.
void order_fixed(const alll_problem& prob, const Knobs& kn, Layout& l);
void transpose_fixed(const alll_problem& prob, Layout& l);
void window_bases(const alll_problem& prob, Layout& l);
// Ragged widths: perm, rg_off, the padded literals and the windows.
int order_ragged(const alll_problem& prob, const Knobs& kn, Layout& l);

}  // namespace alll
