// batch_thr_layout_dump -- TEST INFRASTRUCTURE: the LDS layout of the batch kernel without and with
// LDS-resident thresholds (alll_batch.h: small_lds_layout, small_thr_fits_lds)
// as a stand-alone program.  tests/test_batch_bias_host.py builds it with a plain host compiler under
// the address and undefined-behaviour sanitizers (no HIP, no GPU, nothing loaded into Python).
//
// usage: batch_thr_layout_dump <max_vars> <max_clauses> <max_lits>
// prints "plain", "with" (the ten fields of SmallLds each), "thr_at", "fits" and "budget".
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "alll_batch.h"

namespace {

void line(const char* key, const alll::SmallLds& l) {
    printf("%s %u %u %u %u %u %u %u %u %u %u\n", key, l.lits, l.offs, l.vmask, l.claim, l.A, l.prefix, l.ctl, l.list,
           l.list_stride, l.bytes);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const uint32_t n = (uint32_t)strtoul(argv[1], nullptr, 0), m = (uint32_t)strtoul(argv[2], nullptr, 0),
                   l = (uint32_t)strtoul(argv[3], nullptr, 0);
    uint32_t at = 0;
    line("plain", alll::small_lds_layout(n, m, l));
    line("with", alll::small_lds_layout(n, m, l, &at));
    printf("thr_at %u\nfits %d\nbudget %u\n", at, alll::small_thr_fits_lds(n, m, l) ? 1 : 0, alll::SMALL_LDS_BUDGET);
    return 0;
}
