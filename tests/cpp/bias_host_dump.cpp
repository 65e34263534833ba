// bias_host_dump -- the two host-only helpers of the per-variable probabilities (include/alll.h:
// alll_var_threshold, alll_biased_initial_assignment) as a stand-alone program, so
// that tests/test_bias_host.py can run them under the address and undefined-behaviour sanitizers
// without loading anything into Python.  Links alll_host.cpp alone.
//
//   bias_host_dump thr <bits>...          every argument the 64 bits of a double in hex; prints one
//                                         line "thr <rc> <threshold>" per argument
//   bias_host_dump init <seed> <n> <file> the file holds n little-endian uint32 thresholds; prints
//                                         "rc <rc>" and "bits <n characters 0/1>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "alll.h"

// (alll_host.cpp reports its error text through the runtime, which is not linked here)
extern "C" void alll_internal_set_error(const char* msg) { (void)msg; }

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "thr")) {
        for (int i = 2; i < argc; ++i) {
            const uint64_t bits = strtoull(argv[i], nullptr, 16);
            double p;
            memcpy(&p, &bits, 8);
            uint32_t t = 12345u;
            const int rc = alll_var_threshold(p, &t);
            printf("thr %d %u\n", rc, t);
        }
        return alll_var_threshold(0.5, nullptr) == ALLL_ERR_INVALID_ARG ? 0 : 3;
    }
    if (argc == 5 && !strcmp(argv[1], "init")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0);
        const uint32_t n = (uint32_t)strtoul(argv[3], nullptr, 0);
        std::vector<uint32_t> thr(n);  // exactly n entries: a read past them is a sanitizer report
        FILE* f = fopen(argv[4], "rb");
        if (!f || fread(thr.data(), 4, n, f) != n) return 2;
        fclose(f);
        std::vector<uint8_t> out(n);
        const int rc = alll_biased_initial_assignment(seed, n, thr.data(), out.data());
        std::string s;
        for (uint8_t b : out) s += b ? '1' : '0';
        printf("rc %d\nbits %s\n", rc, s.c_str());
        return 0;
    }
    fprintf(stderr, "usage: bias_host_dump thr <bits>... | init <seed> <n> <file>\n");
    return 2;
}
