// batch_plan_dump.cpp -- TEST INFRASTRUCTURE: runs the host-only batch planner (alll_batch.cpp,
// plan_batch) on a batch read from a file and prints what it decided, one "key values" line
// each.  tests/test_batch_plan.py builds it with a plain host compiler under the address and
// undefined-behaviour sanitizers (no HIP, no GPU, nothing loaded into Python).
//
// input (little endian): u32 n_problems; per problem {u32 n_vars, u32 m, u64 offsets[m + 1],
// u32 n_literals, u32 literals[n_literals]}; u32 n_items; per item {u32 problem, u64 seed}; then the options
// {i32 n_threads, i32 world, u64 stream_batch, u32 flags}.
// usage: batch_plan_dump <input file>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alll_batch.h"

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
    const uint32_t n_items = r.get<uint32_t>();
    std::vector<alll_problem> items(n_items);
    std::vector<uint64_t> seeds(n_items);
    for (uint32_t i = 0; i < n_items; ++i) {
        const Prob& p = probs.at(r.get<uint32_t>());
        items[i] = alll_problem{p.n_vars, 0, p.m, p.offs.data(), p.lits.data()};
        seeds[i] = r.get<uint64_t>();
    }
    alll_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_threads = r.get<int32_t>();
    opt.world = r.get<int32_t>();
    opt.stream_batch = r.get<uint64_t>();
    opt.flags = r.get<uint32_t>();
    fclose(r.f);

    alll::BatchPlan plan;
    const int rc = alll::plan_batch(items.data(), seeds.data(), n_items, opt, plan);
    printf("rc %d\n", rc);
    printf("err %s\n", plan.err.c_str());
    if (rc) return 0;
    printf("shape %u %u %u %u %u %u\n", plan.n_problems, plan.a_words, plan.max_vars, plan.max_clauses, plan.max_lits,
           plan.threads);
    const alll::SmallLds& l = plan.lds;
    printf("lds %u %u %u %u %u %u %u %u %u %u\n", l.lits, l.offs, l.vmask, l.claim, l.A, l.prefix, l.ctl, l.list,
           l.list_stride, l.bytes);
    for (const alll::SmallItem& s : plan.items)
        printf("item %llu %u %u %u %u %u %u %u\n", (unsigned long long)s.seed, s.n_vars, s.n_words, s.m, s.n_lits,
               s.lits_at, s.offs_at, s.a_at);
    line("lits", plan.lits);
    line("offs", plan.offs);
    return 0;
}
