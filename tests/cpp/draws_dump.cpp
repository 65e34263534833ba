// draws_dump -- the random streams of alll_draws.h as a stand-alone host
// program, so that tests/test_draws_host.py can compare every named draw with the oracle, under the
// address and undefined-behaviour sanitizers, without loading anything into Python.  Includes the
// header alone: no HIP, nothing of the library.  All numbers are printed in hex.
//
//   draws_dump kat                         the three Random123 known-answer vectors: "kat x y z w"
//   draws_dump words <seed> <n> <it>...    "fill <n words>", then "resample <it> <n words>" per round
//   draws_dump biased <seed> <it> <n> <file>
//                                          the file holds n little-endian uint32 thresholds (zeros are
//                                          added up to whole words, as the kernels' copies have them);
//                                          "fill <words>" by biased_fill_word, "draw16 <words>" by two
//                                          biased_draw16 per word, "var <words>" by biased_resample_var
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alll_draws.h"

using namespace alll;

static void print_words(const char* tag, const std::vector<uint32_t>& w) {
    printf("%s", tag);
    for (uint32_t x : w) printf(" %x", x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "kat")) {
        const uint32_t in[3][6] = {{0, 0, 0, 0, 0, 0},
                                   {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
                                   {0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u, 0xA4093822u, 0x299F31D0u}};
        for (const auto& c : in) {
            const Word4 o = philox4(c[0], c[1], c[2], c[3], c[4], c[5]);
            printf("kat %x %x %x %x\n", o.x, o.y, o.z, o.w);
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "words")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0);
        const uint32_t n = (uint32_t)strtoul(argv[3], nullptr, 0), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        std::vector<uint32_t> out(n);
        for (uint32_t w = 0; w < n; ++w) out[w] = fill_word(k0, k1, w);
        print_words("fill", out);
        for (int i = 4; i < argc; ++i) {
            const uint64_t it = strtoull(argv[i], nullptr, 0);
            for (uint32_t w = 0; w < n; ++w) out[w] = resample_word(k0, k1, it, w);
            printf("resample %llx", (unsigned long long)it);
            print_words("", out);
        }
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "biased")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0), it = strtoull(argv[3], nullptr, 0);
        const uint32_t n = (uint32_t)strtoul(argv[4], nullptr, 0), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        const uint32_t n_words = (n + 31) / 32;
        std::vector<uint32_t> t(32 * (size_t)n_words, 0u);  // exactly whole words: a read past them is a report
        FILE* f = fopen(argv[5], "rb");
        if (!f || fread(t.data(), 4, n, f) != n) return 2;
        fclose(f);
        std::vector<Word4> thr(8 * (size_t)n_words);  // the same thresholds, four to a call
        if (n_words) memcpy(thr.data(), t.data(), 4 * t.size());
        std::vector<uint32_t> fill(n_words), d16(n_words), var(n_words, 0u);
        for (uint32_t w = 0; w < n_words; ++w) {
            fill[w] = biased_fill_word(k0, k1, w, thr.data() + 8 * (size_t)w);
            d16[w] = biased_draw16(k0, k1, it, 8 * w, thr.data() + 8 * (size_t)w) |
                     biased_draw16(k0, k1, it, 8 * w + 4, thr.data() + 8 * (size_t)w + 4) << 16;
        }
        for (uint32_t v = 0; v < n; ++v)
            var[v >> 5] |= (uint32_t)biased_bit(biased_resample_var(k0, k1, it, v), t[v]) << (v & 31u);
        print_words("fill", fill);
        print_words("draw16", d16);
        print_words("var", var);
        return 0;
    }
    fprintf(stderr, "usage: draws_dump kat | words <seed> <n> <it>... | biased <seed> <it> <n> <file>\n");
    return 2;
}
