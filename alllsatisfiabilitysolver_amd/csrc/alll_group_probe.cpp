// alll_group_probe.cpp -- the host-only planner of alll_group_probe_literals (alll_group_probe.h;
// DESIGN.md §4.14): validation, then layers, slots, chunks and row bases.  No HIP.
#include "alll_group_probe.h"

#include <algorithm>
#include <cstdio>

namespace alll {

namespace {

int refuse(GroupProbePlan& p, const char* fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    p.err = buf;
    return ALLL_ERR_INVALID_ARG;
}

// the layers item `it` has among the chunk's [layer0, layer0 + n_layers)
inline uint32_t layers_in(const GroupProbeItem& it, uint32_t layer0, uint32_t n_layers) {
    const uint32_t own = (it.n_probes + GROUP_PROBE_SLAB - 1) / GROUP_PROBE_SLAB;
    return own <= layer0 ? 0u : std::min(own - layer0, n_layers);
}

// the probes of item `it` in layer `layer` (which it has)
inline uint32_t probes_in(const GroupProbeItem& it, uint32_t layer) {
    return std::min(GROUP_PROBE_SLAB, it.n_probes - layer * GROUP_PROBE_SLAB);
}

}  // namespace

int plan_group_probes(const GroupItem* items, uint64_t n_items, uint32_t union_vars, const uint32_t* probes,
                      const uint64_t* probe_offsets, bool rows, uint64_t n_row_words, uint32_t forced_layers, size_t budget,
                      GroupProbePlan& p) {
    p = GroupProbePlan{};
    if (!probe_offsets || (!items && n_items)) return refuse(p, "group probes: null argument");
    if (probe_offsets[0] != 0)
        return refuse(p, "group probes: the offsets start at %llu, not at 0", probe_offsets[0]);
    for (uint64_t i = 0; i < n_items; ++i)
        if (probe_offsets[i + 1] < probe_offsets[i])
            return refuse(p, "group probes: the offsets descend at item %llu (%llu after %llu)", i, probe_offsets[i + 1],
                          probe_offsets[i]);
    const uint64_t total = probe_offsets[n_items];
    if (total > 0xFFFFFFFFull) return refuse(p, "group probes: %llu probes are more than 2^32 - 1", total);
    if (total && !probes) return refuse(p, "group probes: null probes for a total of %llu", total);
    uint64_t want = 0;
    for (uint64_t i = 0; i < n_items; ++i) {
        const uint64_t np = probe_offsets[i + 1] - probe_offsets[i];
        // (a literal past its item can be a valid literal of the union: this is the check that matters)
        for (uint64_t j = 0; j < np; ++j)
            if (probes[probe_offsets[i] + j] >= 2ull * items[i].n_vars)
                return refuse(p, "group probes: probe %llu of item %llu is literal %llu past the item's variables", j, i,
                              probes[probe_offsets[i] + j]);
        want += np * items[i].n_words;
    }
    if (rows && n_row_words != want)
        return refuse(p, "group probes: rows of %llu words for the %llu of the items' blocks", n_row_words, want);

    p.n_probes = total;
    p.n_row_words = want;
    p.nv_pad = (uint32_t)(((uint64_t)union_vars + 63u) & ~63ull);
    p.items.resize(n_items);
    p.row_base.assign(n_items + 1, 0);
    for (uint64_t i = 0; i < n_items; ++i) {
        const uint32_t np = (uint32_t)(probe_offsets[i + 1] - probe_offsets[i]);
        p.items[i] = GroupProbeItem{items[i].word_base, items[i].n_words, (uint32_t)probe_offsets[i], np};
        p.row_base[i + 1] = p.row_base[i] + (uint64_t)np * items[i].n_words;
        p.n_layers = std::max(p.n_layers, (np + GROUP_PROBE_SLAB - 1) / GROUP_PROBE_SLAB);
        if (np) p.max_item_vars = std::max(p.max_item_vars, items[i].n_vars);
    }
    if (!total) return ALLL_OK;

    // what a layer costs: the delta tables over the union and the layer's slots
    const uint64_t delta = 32ull * p.nv_pad;
    const uint64_t per_slot = (uint64_t)GROUP_PROBE_SLAB * GROUP_PROBE_REC_BYTES + 3 * 8 + 4 + 8;
    std::vector<uint64_t> layer_bytes(p.n_layers, delta), layer_rows(p.n_layers, 0);
    std::vector<uint32_t> layer_slots(p.n_layers, 0);
    for (const GroupProbeItem& it : p.items) {
        const uint32_t own = layers_in(it, 0, p.n_layers);
        for (uint32_t l = 0; l < own; ++l) {
            layer_slots[l] += 1;
            if (rows) layer_rows[l] += (uint64_t)probes_in(it, l) * it.n_words;
        }
    }
    for (uint32_t l = 0; l < p.n_layers; ++l) layer_bytes[l] += layer_slots[l] * per_slot + 8 * layer_rows[l];
    const uint32_t cap = forced_layers ? std::min(forced_layers, GROUP_PROBE_MAX_LAYERS) : GROUP_PROBE_MAX_LAYERS;
    for (uint32_t l = 0; l < p.n_layers;) {
        GroupProbeChunk c{l, 0, 0, 0, 0};
        while (l < p.n_layers && c.n_layers < cap &&
               (forced_layers || c.n_layers == 0 || c.bytes + layer_bytes[l] <= (uint64_t)budget)) {
            c.n_layers += 1;
            c.n_slots += layer_slots[l];
            c.row_words += layer_rows[l];
            c.bytes += layer_bytes[l];
            ++l;
        }
        p.chunks.push_back(c);
    }
    return ALLL_OK;
}

void group_probe_chunk_slots(const GroupProbePlan& p, const GroupProbeChunk& c, bool rows, std::vector<uint32_t>& slot_base,
                             std::vector<uint32_t>& slot_item, std::vector<uint64_t>& slot_row) {
    const size_t n = p.items.size();
    slot_base.assign(n + 1, 0);
    slot_item.clear();
    slot_row.assign(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const GroupProbeItem& it = p.items[i];
        const uint32_t own = layers_in(it, c.layer0, c.n_layers);
        slot_base[i + 1] = slot_base[i] + own;
        for (uint32_t y = 0; y < own; ++y) {
            slot_item.push_back((uint32_t)i);
            slot_row.push_back(slot_row.back() + (rows ? (uint64_t)probes_in(it, c.layer0 + y) * it.n_words : 0));
        }
    }
}

}  // namespace alll
