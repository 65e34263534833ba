// alll_score.h -- split scores of the free variables on the device (include/alll.h, alll_var_scores
// and its group form): the kernels' own argument struct and the host driver both
// runtimes call (alll_score.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "alll.h"
#include "alll_propagate.h"

namespace alll {

// Arguments of k_score_scan / k_score_pick_* (neither the loop's structs nor PropArgs grow).
struct ScoreArgs {
    // the clauses in clause order: ClauseView::lits (bit 31: hot flag) and offs, or the fixed width k
    const uint32_t* lits;
    const uint32_t* offs;
    uint64_t m;
    uint32_t k;
    uint32_t n_vars;             // the union's in a group
    uint32_t n_words;
    uint32_t n_items;
    const uint32_t* PM;          // per word: pinned variables (k_prop_pack; all zero without thresholds)
    const uint32_t* PV;          // per word: their values
    unsigned long long* S;       // 64 per word: S[l] of every literal of the union, padding included
    unsigned long long* word_T;  // per word: the largest T among its variables (0: none)
    uint32_t* word_v;            // per word: the lowest variable that has it
    unsigned long long* n_open;  // per item
    unsigned long long* best_T;  // per item: max of word_T
    uint32_t* best_v;            // per item: the lowest variable (the union's index) that has it; ~0u: none
    const uint32_t* item_vars;   // per item: var_base, n_vars
    alll_split_result* res;      // per item
    // group only (nullptr in a context): whose word it is, the item of every word, the items' clause bases
    const GroupWord* words;
    const uint32_t* word_item;
    const uint32_t* clause_base;
};

// One scoring pass for the n_items items that `p` describes (the fields a propagation call fills in:
// clauses, sizes, the group's tables; p.thr == nullptr: every variable free, else k_prop_pack builds
// PM / PV from it).  item_vars: per item var_base, n_vars.  results: n_items records in the items'
// local numbering.  S_host: nullptr, or it receives the union's score array (64 entries per word).
// The scratch is allocated here and freed before the return; `s` is drained on entry and at the return.
int score_drive(const PropArgs& p, const std::vector<uint32_t>& item_vars, alll_split_result* results,
                std::vector<uint64_t>* S_host, hipStream_t s);

}  // namespace alll
