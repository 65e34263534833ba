// alll_batch.h -- batches of LDS-resident instances (include/alll.h): the records
// the kernel (alll_small.hip) and the device set-up (alll_batch_runtime.cpp) share, and the
// host-only planner (alll_batch.cpp) that validates a batch, stores every distinct problem once
// and packs the device image.  No HIP here: the planner builds with a plain host compiler.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "alll.h"

namespace alll {

// One item of the batch.  Literals and offsets are 16-bit (variables < 8192, literals < 16384,
// offsets <= 24576); every problem's arrays start at a multiple of 8 elements of their pool,
// so they load as 16-byte vectors.
struct SmallItem {
    uint64_t seed;
    uint32_t n_vars, n_words;   // assignment: n_words = ceil(n_vars / 32)
    uint32_t m, n_lits;
    uint32_t lits_at, offs_at;  // first element of the problem in the literal / offset pool
    uint32_t a_at;              // first word of the item's assignment in the assignment pool
    uint32_t pad;               // the planner's 0; the runtime sets 1 while the item has thresholds (§4.8)
};
static_assert(sizeof(SmallItem) == 40, "SmallItem");

// Loop state of one item (device resident, read and written back by its workgroup every slice):
// the scalar part of DevState (alll_internal.h) with the statistics.
struct SmallState {
    uint64_t n_iter;       // eval passes executed
    uint64_t limit_eval;   // eval passes allowed
    uint64_t limit_nores;  // a pass with n_iter == limit_nores does not resample
    uint64_t n_resamples;
    uint64_t sum_mis;
    uint32_t n_violated;   // violated clauses of the last eval pass
    uint32_t done;         // 0 running, 1 solved, 2 stopped at limit_nores
    uint32_t rounds_max;   // most LFMIS rounds one iteration needed
    // best-assignment tracking (maintained by the tracked instantiations only)
    uint32_t best_u;       // fewest violated clauses a pass found (~0: no pass yet)
    uint64_t best_iter;    // n_iter of the first pass that found them (0: no pass yet)
};
static_assert(sizeof(SmallState) == 64, "SmallState");

// Dynamic LDS of the kernel: byte offsets of its arrays, sized from the largest item of the batch.
struct SmallLds {
    uint32_t lits;    // u16[max literals, rounded up to 8]
    uint32_t offs;    // u16[max clauses + 1, rounded up to 8]
    uint32_t vmask;   // u64[ceil(max clauses / 64)]: violated ballots of the eval pass
    uint32_t claim;   // u32[max variables]: LFMIS claim keys, 0 = covered by an MIS clause
    uint32_t A;       // u32[max words]
    uint32_t prefix;  // u32[ceil(max clauses / 64) + 1]: violated clauses before every ballot
    uint32_t ctl;     // u32[8]: live counts of the two lists, the iteration's |MIS| and resamples
    uint32_t list;    // u16[2][max clauses]: undecided violated clauses, double buffered
    uint32_t list_stride;  // elements between the two lists
    uint32_t bytes;
};

// What plan_batch decides.  A failing plan returns its ALLL_ERR_* code and leaves the message in err.
struct BatchPlan {
    std::string err;
    std::vector<SmallItem> items;
    std::vector<uint16_t> lits, offs;   // the pools (every distinct problem once)
    uint32_t a_words = 0;               // assignment pool size
    uint32_t n_problems = 0;            // distinct problems stored
    uint32_t max_vars = 0, max_clauses = 0, max_lits = 0;
    SmallLds lds{};
    uint32_t threads = 64;              // workgroup size, a multiple of 64
};

bool batch_fits(uint32_t n_vars, uint64_t n_clauses, uint64_t n_literals);
SmallLds small_lds_layout(uint32_t max_vars, uint32_t max_clauses, uint32_t max_lits);
// Per-variable thresholds of a batch with a biased item: the same layout followed
// by u32[max variables, rounded up to 4] at *thr_at; bytes includes it.  The thresholds are
// LDS-resident when this layout is within SMALL_LDS_BUDGET, else the kernel reads them from global
// memory and keeps the layout above.
constexpr uint32_t SMALL_LDS_BUDGET = 160u * 1024u;
SmallLds small_lds_layout(uint32_t max_vars, uint32_t max_clauses, uint32_t max_lits, uint32_t* thr_at);
inline bool small_thr_fits_lds(uint32_t max_vars, uint32_t max_clauses, uint32_t max_lits) {
    uint32_t at;
    return small_lds_layout(max_vars, max_clauses, max_lits, &at).bytes <= SMALL_LDS_BUDGET;
}
// Validation (options, then every item: the message names the item's index), deduplication by
// pointer and size, 16-bit packing, LDS layout and workgroup size.
int plan_batch(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options& opt,
               BatchPlan& p);

}  // namespace alll
