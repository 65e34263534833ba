// alll_residual.h -- the residual formula under the pins on the device (include/alll.h, alll_residual
// and its group form): the kernels' own argument struct and the host driver both
// runtimes call (alll_residual.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "alll.h"
#include "alll_propagate.h"

namespace alll {

// The tile of every pass: clauses (assignment words) per workgroup of the classify, count and emit
// kernels -- and the lanes of the workgroup that scans the tile sums, RESID_TILE of them per trip.
constexpr int RESID_TILE = 256;

// Where an item lies in the union (a context is one item at 0).
struct ResidItem {
    uint32_t var_base, n_vars;
    uint32_t word_base, n_words;
    uint32_t clause_base, n_clauses;
};
static_assert(sizeof(ResidItem) == 24, "ResidItem");

// Arguments of the k_resid_* kernels (neither the loop's structs nor PropArgs nor ScoreArgs grow).
struct ResidArgs {
    // the clauses in clause order: ClauseView::lits (bit 31: hot flag) and offs, or the fixed width k
    const uint32_t* lits;
    const uint32_t* offs;
    uint64_t m;
    uint32_t k;
    uint32_t n_vars;             // the union's in a group
    uint32_t n_words;
    uint32_t n_items;
    uint32_t n_tiles_c;          // ceil(m / RESID_TILE)
    uint32_t n_tiles_w;          // ceil(n_words / RESID_TILE)
    const uint32_t* thr;         // 32 * n_words thresholds; nullptr: none
    const uint32_t* PM;          // per word: pinned variables (k_prop_pack; all zero without thresholds)
    const uint32_t* PV;          // per word: their values
    uint32_t* KM;                // per word: kept variables (only grows: atomicOr)
    uint32_t* keptlen;           // per clause: 0 dropped, else 1 + its free occurrences
    uint32_t* ts_c;              // per clause tile: kept clauses
    uint32_t* ts_l;              // per clause tile: residual literals
    uint32_t* ts_v;              // per word tile: kept variables
    unsigned long long* tp_c;    // n_tiles_c + 1: exclusive scan of ts_c, the total last
    unsigned long long* tp_l;    // n_tiles_c + 1
    unsigned long long* tp_v;    // n_tiles_w + 1
    uint32_t* WP;                // per word: kept variables of the union before it
    unsigned long long* n_fals;  // per item
    unsigned long long* first_fals;  // per item: the union's index; ~0: none
    unsigned long long* base_c;  // n_items + 1: kept clauses of the union before the item (the total last)
    unsigned long long* base_l;  // n_items + 1: residual literals
    unsigned long long* base_v;  // n_items + 1: kept variables
    const ResidItem* items;
    alll_residual_result* res;   // per item
    // the residual, the items one after another (all nullptr: the records alone)
    unsigned long long* out_offsets;     // item i's at base_c[i] + i, n_clauses_i + 1 entries
    uint32_t* out_lits;
    uint32_t* out_var_map;
    unsigned long long* out_clause_map;
    uint32_t* out_thr;
    // group only (nullptr in a context): whose word it is, the words of items with thresholds,
    // the item of every word and the items' clause bases
    const GroupWord* words;
    const uint32_t* wbias;
    const uint32_t* word_item;
    const uint32_t* clause_base;
};

// Host arrays that receive the residual (any may be nullptr), laid as alll_group_residual lays them.
struct ResidOut {
    uint64_t* offsets;
    uint32_t* literals;
    uint32_t* var_map;
    uint64_t* clause_map;
    uint32_t* thr_out;
};

// One compaction pass for the items that `p` describes (the fields a propagation call fills in:
// clauses, sizes, the group's tables; p.thr == nullptr: every variable free, else k_prop_pack builds
// PM / PV from it).  n_literals: the union's literal count (the capacity of the literal array).
// results: one record per item in the item's local numbering.  The scratch is one allocation made
// here and freed before the return; `s` is drained on entry and at the return.
int resid_drive(const PropArgs& p, const std::vector<ResidItem>& items, uint64_t n_literals,
                alll_residual_result* results, const ResidOut& out, hipStream_t s);

}  // namespace alll
