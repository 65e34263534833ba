// split_host_dump -- TEST INFRASTRUCTURE: the host-only alll_pinned_scores (include/alll.h,
// DESIGN.md §4.11) as a stand-alone program, so that tests/test_split_host.py can run it under the
// address and undefined-behaviour sanitizers without loading anything into Python.  Links
// alll_host.cpp alone.
//
// input (little endian): u32 n_vars, u32 m, u64 offsets[m + 1], u32 n_literals, u32 literals[n_literals],
// u32 has_thr, u32 n_thr, u32 thr[n_thr].  Every array is held at its exact size: a read past it is a
// sanitizer report.  has_thr == 0: the call passes a null thr (every variable free).
// usage: split_host_dump <input file> <output file>
//   prints "rc <rc>" and "res <var> <score_pos> <score_neg> <n_open> <pad>"; writes the 2 * n_vars
//   scores (u64 each) to the output file.  A refused call leaves the record and the scores at 12345.
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
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<uint32_t> head = many<uint32_t>(f, 2);
    const std::vector<uint64_t> offs = many<uint64_t>(f, (size_t)head[1] + 1);
    const std::vector<uint32_t> lits = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    const bool has_thr = many<uint32_t>(f, 1)[0] != 0;
    const std::vector<uint32_t> thr = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    fclose(f);
    const alll_problem prob{head[0], 0, head[1], offs.data(), lits.data()};
    std::vector<uint64_t> scores(2 * (size_t)head[0], 12345);
    alll_split_result res{12345, 12345, 12345, 12345, 12345};  // (a refused call leaves it alone)
    const int rc = alll_pinned_scores(&prob, has_thr ? thr.data() : nullptr, thr.size(), scores.data(), &res);
    printf("rc %d\nres %u %llu %llu %llu %u\n", rc, res.var, (unsigned long long)res.score_pos,
           (unsigned long long)res.score_neg, (unsigned long long)res.n_open, res.pad);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!scores.empty() && fwrite(scores.data(), 8, scores.size(), o) != scores.size()) return 2;
    fclose(o);
    // the record alone, and the null refusals
    if (rc == ALLL_OK) {
        alll_split_result only{};
        if (alll_pinned_scores(&prob, has_thr ? thr.data() : nullptr, thr.size(), nullptr, &only) != ALLL_OK) return 3;
        if (only.var != res.var || only.score_pos != res.score_pos || only.score_neg != res.score_neg ||
            only.n_open != res.n_open || only.pad != 0)
            return 3;
    }
    if (alll_pinned_scores(nullptr, thr.data(), thr.size(), scores.data(), &res) != ALLL_ERR_INVALID_ARG) return 3;
    if (alll_pinned_scores(&prob, thr.data(), thr.size(), scores.data(), nullptr) != ALLL_ERR_INVALID_ARG) return 3;
    return 0;
}
