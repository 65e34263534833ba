// group_plan_dump.cpp -- TEST INFRASTRUCTURE: runs the host-only group planner (alll_group.cpp,
// plan_group) on a group read from a file and prints what it decided, one "key values" line
// each.  tests/test_group_plan.py builds it with a plain host compiler under the address and
// undefined-behaviour sanitizers (no HIP, no GPU, nothing loaded into Python).
//
// input (little endian): u32 n_problems; per problem {u32 n_vars, u32 m, u64 offsets[m + 1],
// u32 n_literals, u32 literals[n_literals]}; u32 n_items; per item {u32 problem, u64 seed}; then the options
// {i32 n_threads, i32 world, u64 stream_batch, u32 flags, u32 comm_byte} (comm_byte != 0: comm_id[5] = comm_byte).
// A problem index of 0xFFFFFFFF hands plan_group null item arrays, an item count of 0xFFFFFFFF a null seed array.
// usage: group_plan_dump <input file>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alll_group.h"

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
    struct Prob { uint32_t n_vars, m; std::vector<uint64_t> offs; std::vector<uint32_t> lits; };
    std::vector<Prob> probs(r.get<uint32_t>());
    for (Prob& p : probs) {
        p.n_vars = r.get<uint32_t>();
        p.m = r.get<uint32_t>();
        p.offs = r.many<uint64_t>((size_t)p.m + 1);
        // (the literal count is the file's, not offsets[m]: a test may hand in bad offsets)
        p.lits = r.many<uint32_t>(r.get<uint32_t>());
    }
    uint32_t n_items = r.get<uint32_t>();
    const bool null_seeds = n_items == 0xFFFFFFFFu;
    if (null_seeds) n_items = 1;
    std::vector<alll_problem> items(n_items);
    std::vector<uint64_t> seeds(n_items);
    bool null_probs = false;
    for (uint32_t i = 0; i < n_items && !null_seeds; ++i) {
        const uint32_t pi = r.get<uint32_t>();
        seeds[i] = r.get<uint64_t>();
        if (pi == 0xFFFFFFFFu) { null_probs = true; continue; }
        const Prob& p = probs.at(pi);
        items[i] = alll_problem{p.n_vars, 0, p.m, p.offs.data(), p.lits.data()};
    }
    alll_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_threads = r.get<int32_t>();
    opt.world = r.get<int32_t>();
    opt.stream_batch = r.get<uint64_t>();
    opt.flags = r.get<uint32_t>();
    opt.comm_id[5] = (uint8_t)r.get<uint32_t>();
    fclose(r.f);

    alll::GroupPlan plan;
    const int rc = alll::plan_group(null_probs ? nullptr : items.data(), null_seeds ? nullptr : seeds.data(), n_items,
                                    opt, plan);
    printf("rc %d\n", rc);
    printf("err %s\n", plan.err.c_str());
    if (rc) return 0;
    printf("shape %u %llu %zu\n", plan.n_vars, (unsigned long long)plan.n_clauses, plan.words.size());
    for (const alll::GroupItem& g : plan.items)
        printf("item %llu %llu %u %u %u %u %u %u\n", (unsigned long long)g.seed, (unsigned long long)g.lit_base, g.n_vars,
               g.n_words, g.var_base, g.word_base, g.clause_base, g.n_clauses);
    line("clause_base", plan.clause_base);
    printf("words");
    for (const alll::GroupWord& w : plan.words) printf(" %u %u %u %u", w.seed_lo, w.seed_hi, w.local_word, w.tail_mask);
    printf("\n");
    line("offsets", plan.offsets);
    line("literals", plan.literals);
    return 0;
}
