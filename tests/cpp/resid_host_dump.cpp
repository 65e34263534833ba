// resid_host_dump -- TEST INFRASTRUCTURE: the host-only alll_pinned_residual (include/alll.h,
// DESIGN.md §4.12) as a stand-alone program, so that tests/test_resid_host.py can run it under the
// address and undefined-behaviour sanitizers without loading anything into Python.  Links
// alll_host.cpp alone.
//
// input (little endian): u32 n_vars, u32 m, u64 offsets[m + 1], u32 n_literals, u32 literals[n_literals],
// u32 has_thr, u32 n_thr, u32 thr[n_thr].  Every array is held at its exact size: a read past it is a
// sanitizer report.  has_thr == 0: the call passes a null thr (every variable free).
// usage: resid_host_dump <input file> <output file>
//   prints "rc <rc>" and "res <n_vars> <n_clauses> <n_literals> <n_falsified> <first_falsified> <pad>";
//   writes to the output file, each at its capacity (the original sizes: a write past one is a
//   sanitizer report): u64 offsets[m + 1], u32 literals[n_literals], u32 var_map[n_vars],
//   u64 clause_map[m], u32 thr_out[n_vars].  A refused call leaves the record and the arrays at 12345.
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

template <typename T>
bool put(FILE* o, const std::vector<T>& v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), o) == v.size();
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
    const uint32_t nv = head[0], m = head[1];
    const alll_problem prob{nv, 0, m, offs.data(), lits.data()};
    const uint32_t* t = has_thr ? thr.data() : nullptr;
    std::vector<uint64_t> r_offs((size_t)m + 1, 12345), r_cmap(m, 12345);
    std::vector<uint32_t> r_lits(lits.size(), 12345), r_vmap(nv, 12345), r_thr(nv, 12345);
    alll_residual_result res{12345, 12345, 12345, 12345, 12345, 12345};  // (a refused call leaves it alone)
    const int rc = alll_pinned_residual(&prob, t, thr.size(), &res, r_offs.data(), r_lits.data(), r_vmap.data(),
                                        r_cmap.data(), r_thr.data());
    printf("rc %d\nres %u %llu %llu %llu %llu %u\n", rc, res.n_vars, (unsigned long long)res.n_clauses,
           (unsigned long long)res.n_literals, (unsigned long long)res.n_falsified,
           (unsigned long long)res.first_falsified, res.pad);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!put(o, r_offs) || !put(o, r_lits) || !put(o, r_vmap) || !put(o, r_cmap) || !put(o, r_thr)) return 2;
    fclose(o);
    // the record alone, one array alone, and the null refusals
    if (rc == ALLL_OK) {
        alll_residual_result only{};
        if (alll_pinned_residual(&prob, t, thr.size(), &only, nullptr, nullptr, nullptr, nullptr, nullptr) != ALLL_OK) return 3;
        if (only.n_vars != res.n_vars || only.n_clauses != res.n_clauses || only.n_literals != res.n_literals ||
            only.n_falsified != res.n_falsified || only.first_falsified != res.first_falsified || only.pad != 0)
            return 3;
        std::vector<uint32_t> again(lits.size(), 12345);
        if (alll_pinned_residual(&prob, t, thr.size(), &only, nullptr, again.data(), nullptr, nullptr, nullptr) != ALLL_OK) return 3;
        if (again != r_lits) return 3;
    }
    if (alll_pinned_residual(nullptr, thr.data(), thr.size(), &res, r_offs.data(), nullptr, nullptr, nullptr, nullptr) !=
        ALLL_ERR_INVALID_ARG)
        return 3;
    if (alll_pinned_residual(&prob, thr.data(), thr.size(), nullptr, r_offs.data(), nullptr, nullptr, nullptr, nullptr) !=
        ALLL_ERR_INVALID_ARG)
        return 3;
    return 0;
}
