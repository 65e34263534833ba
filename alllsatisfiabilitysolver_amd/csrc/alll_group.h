// alll_group.h -- block-diagonal groups (include/alll.h, alll_group_*): many
// instances of any size laid side by side as one instance with disjoint variable and clause ranges,
// advanced together by the one-instance loop.  The records the kernels (alll_kernels.hip, k_group_*)
// and the device set-up (alll_group_runtime.cpp) share, and the host-only planner (alll_group.cpp)
// that validates the items, lays them out and writes the union's CSR.  No HIP here: the planner
// builds with a plain host compiler.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "alll.h"

namespace alll {

// One item of the group inside the union.  Its variables are [var_base, var_base + n_vars) with
// var_base = 32 * word_base (every item starts a new assignment word, so its Philox words are its
// own; the padding variables up to the next multiple of 32 occur in no clause), its clauses
// [clause_base, clause_base + n_clauses) in their own order, literals shifted by 2 * var_base.
struct GroupItem {
    uint64_t seed;
    uint64_t lit_base;          // first literal of the item in the union's literal array
    uint32_t n_vars, n_words;   // n_words = ceil(n_vars / 32)
    uint32_t var_base, word_base;
    uint32_t clause_base, n_clauses;
};
static_assert(sizeof(GroupItem) == 40, "GroupItem");

// Per assignment word of the union: whose word it is (the keyed init and resample kernels draw
// Philox(key = seed, counter word = local_word) from one 16-byte load).
struct GroupWord {
    uint32_t seed_lo, seed_hi;
    uint32_t local_word;
    uint32_t tail_mask;         // bits of the word that are variables of the item (~0u but for its last word)
};
static_assert(sizeof(GroupWord) == 16, "GroupWord");

// What plan_group decides.  A failing plan returns its ALLL_ERR_* code and leaves the message in err.
struct GroupPlan {
    std::string err;
    std::vector<GroupItem> items;
    std::vector<uint32_t> clause_base;  // n_items + 1: clause_base of every item, then the union's clause count
    std::vector<GroupWord> words;       // one per assignment word of the union
    // the union as one CSR instance
    uint32_t n_vars = 0;                // last item's var_base + n_vars
    uint64_t n_clauses = 0;
    std::vector<uint64_t> offsets;      // n_clauses + 1
    std::vector<uint32_t> literals;
};

// Validation (options first, then every item: the message names the item's index; the codes are
// alll_create's), the layout of the items in the union and its CSR.  Items may share arrays: every
// item gets its own shifted copy of its clauses.
int plan_group(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items, const alll_options& opt,
               GroupPlan& p);

}  // namespace alll
