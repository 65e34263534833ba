// pinned_conflict_dump -- TEST INFRASTRUCTURE: the host-only alll_pinned_conflict (include/alll.h,
// DESIGN.md §4.8) as a stand-alone program, so that tests/test_batch_bias_host.py can run it under
// the address and undefined-behaviour sanitizers without loading anything into Python.  Links
// alll_host.cpp alone.
//
// input (little endian): u32 n_vars, u32 m, u64 offsets[m + 1], u32 n_literals, u32 literals[n_literals],
// u32 n_thr, u32 thr[n_thr].  Every array is held at its exact size: a read past it is a sanitizer report.
// usage: pinned_conflict_dump <input file>      prints "rc <rc>" and "clause <index>"
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
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<uint32_t> head = many<uint32_t>(f, 2);
    const std::vector<uint64_t> offs = many<uint64_t>(f, (size_t)head[1] + 1);
    const std::vector<uint32_t> lits = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    const std::vector<uint32_t> thr = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    fclose(f);
    const alll_problem prob{head[0], 0, head[1], offs.data(), lits.data()};
    uint64_t clause = 12345;  // (a refused call leaves it alone)
    const int rc = alll_pinned_conflict(&prob, thr.data(), thr.size(), &clause);
    printf("rc %d\nclause %llu\n", rc, (unsigned long long)clause);
    // the null refusals
    if (alll_pinned_conflict(nullptr, thr.data(), thr.size(), &clause) != ALLL_ERR_INVALID_ARG) return 3;
    if (alll_pinned_conflict(&prob, thr.data(), thr.size(), nullptr) != ALLL_ERR_INVALID_ARG) return 3;
    if (head[0] && alll_pinned_conflict(&prob, nullptr, head[0], &clause) != ALLL_ERR_INVALID_ARG) return 3;
    return 0;
}
