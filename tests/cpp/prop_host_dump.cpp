// prop_host_dump -- TEST INFRASTRUCTURE: the host-only alll_pinned_propagate (include/alll.h,
// DESIGN.md §4.10) as a stand-alone program, so that tests/test_prop_host.py can run it under the
// address and undefined-behaviour sanitizers without loading anything into Python.  Links
// alll_host.cpp alone.
//
// input (little endian): u32 n_vars, u32 m, u64 offsets[m + 1], u32 n_literals, u32 literals[n_literals],
// u32 n_thr, u32 thr[n_thr].  Every array is held at its exact size: a read past it is a sanitizer report.
// usage: prop_host_dump <input file> <max_rounds> <output file>
//   prints "rc <rc>" and "res <status> <rounds> <n_forced> <conflict_clause>", then the same for a
//   second call on the propagated thresholds; writes them (u32 each) to the output file
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "alll.h"

// (alll_host.cpp reports its error text through the runtime, which is not linked here)
extern "C" void alll_internal_set_error(const char* msg) { (void)msg; }

namespace {

template <typename T>
std::vector<T> many(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<uint32_t> head = many<uint32_t>(f, 2);
    const std::vector<uint64_t> offs = many<uint64_t>(f, (size_t)head[1] + 1);
    const std::vector<uint32_t> lits = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    std::vector<uint32_t> thr = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    fclose(f);
    const uint64_t max_rounds = strtoull(argv[2], nullptr, 10);
    const alll_problem prob{head[0], 0, head[1], offs.data(), lits.data()};
    for (int call = 0; call < 2; ++call) {
        alll_propagate_result res{12345, 12345, 12345, 12345};  // (a refused call leaves it alone)
        const int rc = alll_pinned_propagate(&prob, thr.data(), thr.size(), max_rounds, &res);
        printf("rc %d\nres %d %u %llu %llu\n", rc, res.status, res.rounds, (unsigned long long)res.n_forced,
               (unsigned long long)res.conflict_clause);
        if (call == 0) {
            FILE* o = fopen(argv[3], "wb");
            if (!o) return 2;
            if (!thr.empty() && fwrite(thr.data(), 4, thr.size(), o) != thr.size()) return 2;
            fclose(o);
        }
    }
    // the null refusals
    alll_propagate_result res{};
    if (alll_pinned_propagate(nullptr, thr.data(), thr.size(), 0, &res) != ALLL_ERR_INVALID_ARG) return 3;
    if (alll_pinned_propagate(&prob, thr.data(), thr.size(), 0, nullptr) != ALLL_ERR_INVALID_ARG) return 3;
    if (head[0] && alll_pinned_propagate(&prob, nullptr, head[0], 0, &res) != ALLL_ERR_INVALID_ARG) return 3;
    return 0;
}
