// alll_probe.h -- failed-literal probing on the device (include/alll.h, alll_probe_literals; DESIGN.md
// §4.13): the kernels' own argument struct and the host driver the runtime calls (alll_probe.hip).
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alll.h"
#include "alll_group_probe.h"
#include "alll_propagate.h"

namespace alll {

constexpr uint32_t PROBE_SLAB = 64;                 // probes per slab: bit p of a delta word is probe p
constexpr size_t PROBE_BUDGET_BYTES = 1ull << 30;   // the scratch of one chunk of slabs
constexpr uint32_t PROBE_MAX_CHUNK = 4096;          // slabs per chunk at the most (the grid's second dimension)
static_assert(PROBE_SLAB == GROUP_PROBE_SLAB && PROBE_MAX_CHUNK == GROUP_PROBE_MAX_LAYERS, "the planner's constants");

// Per probe: what its rounds found so far (the host reads the records once, when the chunk has ended).
struct ProbeRec {
    unsigned long long conflict;  // smallest falsified clause of the round, PROP_NO_CONFLICT: none
    uint32_t forced;              // variables this round's units pin (k_probe_apply; cleared by k_probe_settle)
    uint32_t rounds;              // rounds that applied something
    uint32_t n_forced;            // variables pinned so far, the probe's own not counted
    int32_t status;               // ALLL_PROP_*, final once the probe's bit has left act
};
static_assert(sizeof(ProbeRec) == GROUP_PROBE_REC_BYTES, "ProbeRec");

// Arguments of the k_probe_* kernels (PropArgs, ScoreArgs and the loop's structs do not grow).  The
// per-slab arrays hold n_slabs entries; slab s owns the delta words [s * nv_pad, (s + 1) * nv_pad).
struct ProbeArgs {
    // the clauses in clause order: ClauseView::lits (bit 31: hot flag) and offs, or the fixed width k
    const uint32_t* lits;
    const uint32_t* offs;
    uint64_t m;
    uint32_t k;
    uint32_t n_vars;
    uint32_t n_words;
    uint32_t nv_pad;              // n_vars rounded up to whole waves of 64
    uint32_t n_slabs;             // of this chunk
    uint32_t n_probes;            // of this chunk (the last slab may be ragged)
    uint32_t max_rounds;          // 0: no cap
    const uint32_t* probes;       // the chunk's literals
    const uint32_t* PM;           // per word: the base's pinned variables (k_prop_pack)
    const uint32_t* PV;           // per word: their values
    unsigned long long* DM;       // per slab and variable: pinned by the probe's own propagation
    unsigned long long* DV;       // ... its value
    unsigned long long* F1;       // ... forced to 1 by a unit of this round
    unsigned long long* F0;       // ... to 0
    ProbeRec* rec;                // per slab 64 records
    unsigned long long* act;      // per slab: probes still running
    unsigned long long* cnt;      // per slab: probes whose new variables this round are counted
    unsigned long long* app;      // per slab: probes whose units this round are applied
    uint32_t* any_active;         // one word: a probe of the chunk still runs (the host reads it per round)
    uint32_t* pm_rows;            // n_probes x n_words: the probes' pinned bits, the base's included
    uint32_t* pv_rows;            // ... value bits
};

// Arguments of the group instantiations.  What changes its meaning: the sizes and the
// base bitmaps are the union's; the delta words are per layer of the chunk (layer y owns [y * nv_pad,
// (y + 1) * nv_pad)); n_slabs is the chunk's slot count and rec / act / cnt / app are per slot; probes
// holds the whole call's literals, in the items' local numbering; pm_rows / pv_rows are the chunk's
// rows, slot after slot.
struct GroupProbeArgs : ProbeArgs {
    const GroupProbeItem* items;         // per item: its words and its probes
    const uint32_t* slot_base;           // n_items + 1: slot(item, layer y) = slot_base[item] + y while below the next base
    const uint32_t* slot_item;           // per slot: its item
    const unsigned long long* slot_row;  // per slot: where its rows start in pm_rows / pv_rows, in words
    const uint32_t* word_item;           // per assignment word of the union: its item
    const uint32_t* clause_base;         // n_items + 1 ascending clause bases
    uint32_t n_items;
    uint32_t layer0;                     // the chunk's first layer
};

// The probes of include/alll.h for one context: `p` carries what a propagation call fills in (the
// clauses, the sizes; p.thr == nullptr: every variable free, else k_prop_pack builds the base bitmaps
// from it; thr is only read).  results: n_probes records; pm_rows / pv_rows: nullptr, or n_probes x
// n_words words each.  Works in chunks of slabs under PROBE_BUDGET_BYTES (env ALLL_PROBE_SLABS forces
// the chunk, whatever the budget says); the scratch is allocated here and freed before the return;
// `s` is drained on entry and at the return.
int probe_drive(const PropArgs& p, const uint32_t* probes, uint64_t n_probes, uint64_t max_rounds,
                alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, hipStream_t s);

// The group form, alll_group_probe_literals: `p` is what the group hands its drivers (the union's
// clauses and sizes, the group's tables; p.thr == nullptr: no item has thresholds), `plan` what
// plan_group_probes decided for this call, items the group's (clause bases and counts), probes the
// call's.  results, pm_rows and pv_rows are the caller's arrays (rows: both or neither).  The scratch
// is allocated here and freed before the return; `s` is drained on entry and at the return.
int group_probe_drive(const PropArgs& p, const GroupProbePlan& plan, const GroupItem* items, const uint32_t* probes,
                      uint64_t max_rounds, alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows,
                      hipStream_t s);

// ALLL_PROBE_SLABS: slabs (a group: layers) per chunk whatever the budget says; 0: not set
uint32_t probe_forced_chunk();

}  // namespace alll
