// probe_host_dump -- TEST INFRASTRUCTURE: the host-only alll_pinned_probe (include/alll.h, DESIGN.md
// §4.13) as a stand-alone program, so that tests/test_probe_host.py can run it under the address and
// undefined-behaviour sanitizers without loading anything into Python.  Links alll_host.cpp alone.
//
// input (little endian): u32 n_vars, u32 m, u64 offsets[m + 1], u32 n_literals, u32 literals[n_literals],
// u32 has_thr, u32 n_thr, u32 thr[n_thr], u32 max_rounds, u32 n_probes, u32 probes[n_probes].  Every
// array is held at its exact size: a read or write past it is a sanitizer report.  has_thr == 0: the
// call passes a null thr (every variable a fair coin).
// usage: probe_host_dump <input file> <output file>
//   prints "rc <rc>" and per probe "res <status> <rounds> <n_forced> <conflict_clause>"; writes pm_rows
//   then pv_rows (n_probes x ceil(n_vars/32) u32 each) to the output file.  A refused call leaves the
//   records and the rows at 12345.
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
    const uint32_t max_rounds = many<uint32_t>(f, 1)[0];
    const std::vector<uint32_t> probes = many<uint32_t>(f, many<uint32_t>(f, 1)[0]);
    fclose(f);
    const alll_problem prob{head[0], 0, head[1], offs.data(), lits.data()};
    const size_t np = probes.size(), nw = ((size_t)head[0] + 31) / 32;
    std::vector<alll_propagate_result> res(np, alll_propagate_result{12345, 12345, 12345, 12345});
    std::vector<uint32_t> pm(np * nw, 12345), pv(np * nw, 12345);
    const std::vector<uint32_t> thr_before = thr;
    const int rc = alll_pinned_probe(&prob, has_thr ? thr.data() : nullptr, thr.size(), probes.data(), np, max_rounds,
                                     res.data(), pm.data(), pv.data());
    if (thr != thr_before) return 3;  // (the base thresholds are only read)
    printf("rc %d\n", rc);
    for (const alll_propagate_result& r : res)
        printf("res %d %u %llu %llu\n", r.status, r.rounds, (unsigned long long)r.n_forced, (unsigned long long)r.conflict_clause);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (!pm.empty() && (fwrite(pm.data(), 4, pm.size(), o) != pm.size() || fwrite(pv.data(), 4, pv.size(), o) != pv.size())) return 2;
    fclose(o);
    // the records alone are the same records; the null refusals
    if (rc == ALLL_OK) {
        std::vector<alll_propagate_result> only(np);
        if (alll_pinned_probe(&prob, has_thr ? thr.data() : nullptr, thr.size(), probes.data(), np, max_rounds, only.data(),
                              nullptr, nullptr) != ALLL_OK)
            return 3;
        for (size_t i = 0; i < np; ++i)
            if (only[i].status != res[i].status || only[i].rounds != res[i].rounds || only[i].n_forced != res[i].n_forced ||
                only[i].conflict_clause != res[i].conflict_clause)
                return 3;
    }
    if (alll_pinned_probe(nullptr, thr.data(), thr.size(), probes.data(), np, 0, res.data(), nullptr, nullptr) !=
        ALLL_ERR_INVALID_ARG)
        return 3;
    if (alll_pinned_probe(&prob, thr.data(), thr.size(), probes.data(), np, 0, nullptr, nullptr, nullptr) != ALLL_ERR_INVALID_ARG)
        return 3;
    return 0;
}
