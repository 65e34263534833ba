// alll_propagate.h -- unit propagation of the pinned variables on the device (include/alll.h,
// alll_propagate_pins and its group form): the kernels' own argument struct, their
// launchers (alll_propagate.hip) and the host driver both runtimes call.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "alll.h"
#include "alll_group.h"
#include "alll_internal.h"

namespace alll {

constexpr unsigned long long PROP_NO_CONFLICT = ~0ull;

// Per item (a context is one item): what a round found, read by the host after every round.
struct PropItem {
    unsigned long long conflict;  // smallest falsified clause (the union's index), PROP_NO_CONFLICT: none
    uint32_t forced;              // variables the round's units pin (counted by k_prop_apply)
    uint32_t active;              // the item still propagates (the host clears it when the item ends)
};
static_assert(sizeof(PropItem) == 16, "PropItem");

// Arguments of k_prop_pack / k_prop_scan / k_prop_apply (none of the loop's structs grows).
struct PropArgs {
    // the clauses in clause order: ClauseView::lits (bit 31: hot flag) and offs, or the fixed width k
    const uint32_t* lits;
    const uint32_t* offs;
    uint64_t m;
    uint32_t k;
    uint32_t n_vars;           // the union's in a group
    uint32_t n_words;
    uint32_t n_items;
    uint32_t* thr;             // 32 * n_words thresholds
    uint32_t* PM;              // per word: pinned variables
    uint32_t* PV;              // per word: their values
    uint32_t* F1;              // per word: variables a unit of this round forces to 1
    uint32_t* F0;              // ... to 0
    PropItem* items;
    // group only (nullptr in a context): whose word it is, the words of items with thresholds,
    // the item of every word and the items' clause bases
    const GroupWord* words;
    const uint32_t* wbias;
    const uint32_t* word_item;
    const uint32_t* clause_base;
};

// the item of clause c: the last clause base <= c (n_items + 1 ascending bases; empty items share one)
__device__ __forceinline__ uint32_t prop_clause_item(const uint32_t* clause_base, uint32_t n_items, uint32_t c) {
    uint32_t lo = 0, hi = n_items;  // clause_base[lo] <= c < clause_base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (clause_base[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Launchers (alll_propagate.hip).  All asynchronous on `s`.
hipError_t launch_prop_pack(const PropArgs& a, hipStream_t s);
hipError_t launch_prop_scan(const PropArgs& a, hipStream_t s);
// dry: the round that would exceed max_rounds -- the forced variables are counted, nothing is applied
hipError_t launch_prop_apply(const PropArgs& a, bool dry, hipStream_t s);

// The rounds (pack, then scan + apply and a read of the items' records per round) for the n_items
// items of `a`; on[i] == 0: the item has no thresholds (ALLL_PROP_NONE).  a.PM .. a.items are
// allocated here and freed before the return; results[i].conflict_clause is the union's index
// (a.m when there is none).  Stream drained at the return.
int prop_drive(PropArgs a, const uint8_t* on, uint64_t max_rounds, alll_propagate_result* results, hipStream_t s);

}  // namespace alll
