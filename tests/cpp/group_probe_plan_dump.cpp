// group_probe_plan_dump.cpp -- TEST INFRASTRUCTURE: runs the host-only planner of
// alll_group_probe_literals (alll_group_probe.cpp, plan_group_probes) on a call read from a file and
// prints what it decided, one "key values" line each.  tests/test_group_probe_plan.py builds it with a
// plain host compiler under the address and undefined-behaviour sanitizers (no HIP, no GPU, nothing
// loaded into Python).
//
// input (little endian): u32 n_items; u32 n_vars[n_items] (the items are laid out as plan_group lays
// them: every item starts a new assignment word); u32 null_offsets; u64 offsets[n_items + 1];
// u32 null_probes; u32 n_probes; u32 probes[n_probes]; u32 rows; u64 n_row_words; u32 forced_layers;
// u64 budget.
// usage: group_probe_plan_dump <input file>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "alll_group_probe.h"

namespace {

struct Reader {
    FILE* f;
    template <typename T>
    T get() {
        T x{};
        if (fread(&x, sizeof x, 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); }
        return x;
    }
    template <typename T>
    std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
        return v;
    }
};

template <typename T>
void line(const char* key, const std::vector<T>& v) {
    printf("%s", key);
    for (const T& x : v) printf(" %llu", (unsigned long long)x);
    printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader r{fopen(argv[1], "rb")};
    if (!r.f) return 2;
    const uint32_t n_items = r.get<uint32_t>();
    const std::vector<uint32_t> n_vars = r.many<uint32_t>(n_items);
    const bool null_offsets = r.get<uint32_t>() != 0;
    const std::vector<uint64_t> offsets = r.many<uint64_t>((size_t)n_items + 1);
    const bool null_probes = r.get<uint32_t>() != 0;
    const std::vector<uint32_t> probes = r.many<uint32_t>(r.get<uint32_t>());
    const bool rows = r.get<uint32_t>() != 0;
    const uint64_t n_row_words = r.get<uint64_t>();
    const uint32_t forced = r.get<uint32_t>();
    const uint64_t budget = r.get<uint64_t>();
    fclose(r.f);

    std::vector<alll::GroupItem> items(n_items);
    uint32_t word = 0, clause = 0, union_vars = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        alll::GroupItem& g = items[i];
        g = alll::GroupItem{};
        g.n_vars = n_vars[i];
        g.n_words = (n_vars[i] + 31u) / 32u;
        g.word_base = word;
        g.var_base = 32u * word;
        g.clause_base = clause;
        g.n_clauses = 3;
        word += g.n_words;
        clause += g.n_clauses;
        union_vars = g.var_base + g.n_vars;
    }
    alll::GroupProbePlan plan;
    const int rc = alll::plan_group_probes(items.data(), n_items, union_vars, null_probes ? nullptr : probes.data(),
                                           null_offsets ? nullptr : offsets.data(), rows, n_row_words, forced, (size_t)budget,
                                           plan);
    printf("rc %d\n", rc);
    printf("err %s\n", plan.err.c_str());
    if (rc) return 0;
    printf("shape %llu %u %u %u %llu\n", (unsigned long long)plan.n_probes, plan.n_layers, plan.max_item_vars, plan.nv_pad,
           (unsigned long long)plan.n_row_words);
    for (const alll::GroupProbeItem& it : plan.items) printf("item %u %u %u %u\n", it.word_base, it.n_words, it.probe_base, it.n_probes);
    line("row_base", plan.row_base);
    std::vector<uint32_t> slot_base, slot_item;
    std::vector<uint64_t> slot_row;
    for (const alll::GroupProbeChunk& c : plan.chunks) {
        printf("chunk %u %u %u %llu %llu\n", c.layer0, c.n_layers, c.n_slots, (unsigned long long)c.row_words,
               (unsigned long long)c.bytes);
        alll::group_probe_chunk_slots(plan, c, rows, slot_base, slot_item, slot_row);
        line("slot_base", slot_base);
        line("slot_item", slot_item);
        line("slot_row", slot_row);
    }
    return 0;
}
