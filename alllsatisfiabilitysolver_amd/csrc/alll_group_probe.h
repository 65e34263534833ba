// alll_group_probe.h -- failed-literal probing of a whole group (include/alll.h,
// alll_group_probe_literals): the host-only planner that validates the call and lays
// out its layers, slots, chunks and rows (alll_group_probe.cpp), and the records it shares with the
// kernels and their driver (alll_probe.hip).  No HIP here: the planner builds with a plain host compiler.
//
// The items of a group have disjoint variables and clauses, so bit p of a delta word is probe p of
// whichever item owns the variable: layer L holds probes 64 L .. 64 L + 63 of every item that has that
// many, and one pass over the union's clauses advances 64 probes of every item.  A slot is a (layer,
// item) pair that has probes; masks and records exist per slot only (an item without probes costs
// nothing but its entry in the slot bases).  Within a chunk of layers the slots are laid item after
// item: slot(item i, chunk layer y) = slot_base[i] + y, valid while y < slot_base[i + 1] - slot_base[i].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "alll.h"
#include "alll_group.h"

namespace alll {

constexpr uint32_t GROUP_PROBE_SLAB = 64;        // probes per slot (alll_probe.h: PROBE_SLAB)
constexpr uint32_t GROUP_PROBE_REC_BYTES = 24;   // sizeof(ProbeRec)
constexpr uint32_t GROUP_PROBE_MAX_LAYERS = 4096;  // layers per chunk at the most (alll_probe.h: PROBE_MAX_CHUNK)

// Per item, as the kernels read it (one 16-byte load).
struct GroupProbeItem {
    uint32_t word_base, n_words;   // the item's assignment words in the union
    uint32_t probe_base, n_probes; // its probes in the call's probe array
};
static_assert(sizeof(GroupProbeItem) == 16, "GroupProbeItem");

// A chunk of layers that goes through the launches together.
struct GroupProbeChunk {
    uint32_t layer0, n_layers;
    uint32_t n_slots;      // (layer, item) pairs of the chunk that have probes
    uint64_t row_words;    // words of one of the two row arrays of the chunk (0 without rows)
    uint64_t bytes;        // the chunk's scratch as accounted against the budget
};

struct GroupProbePlan {
    std::string err;
    uint64_t n_probes = 0;         // of the call
    uint32_t n_layers = 0;         // of the item with the most probes
    uint32_t max_item_vars = 0;    // the round bound without a cap is this + 1
    uint32_t nv_pad = 0;           // the union's variables rounded up to whole waves of 64
    uint64_t n_row_words = 0;      // the sum of the items' row blocks
    std::vector<GroupProbeItem> items;
    std::vector<uint64_t> row_base;  // n_items + 1: the items' blocks in the caller's row arrays, in words
    std::vector<GroupProbeChunk> chunks;
};

// Validation (ALLL_ERR_INVALID_ARG and a message in p.err: null offsets, null probes with a non-zero
// total, offsets that do not start at 0 or descend, more than 2^32 - 1 probes, a probe >= 2 n_vars of
// its own item, rows of n_row_words words when the blocks sum to something else) and the layout.
// forced_layers (env ALLL_PROBE_SLABS): layers per chunk whatever the budget says, 0: as many as fit
// `budget` bytes (at least one), GROUP_PROBE_MAX_LAYERS at the most.  Accounted per chunk: 32 bytes per
// layer and variable of the union (nv_pad), per slot the 64 records, the three masks, the slot's item
// and row base, and with rows 2 x its probes x the item's words x 4 bytes.
int plan_group_probes(const GroupItem* items, uint64_t n_items, uint32_t union_vars, const uint32_t* probes,
                      const uint64_t* probe_offsets, bool rows, uint64_t n_row_words, uint32_t forced_layers, size_t budget,
                      GroupProbePlan& p);

// The slots of chunk c: slot_base (n_items + 1), the item of every slot, and the slots' bases in the
// chunk's row arrays in words (n_slots + 1; all 0 without rows).
void group_probe_chunk_slots(const GroupProbePlan& p, const GroupProbeChunk& c, bool rows, std::vector<uint32_t>& slot_base,
                             std::vector<uint32_t>& slot_item, std::vector<uint64_t>& slot_row);

}  // namespace alll
