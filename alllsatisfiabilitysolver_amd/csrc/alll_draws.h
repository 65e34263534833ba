// alll_draws.h -- the random streams (include/alll.h): Philox4x32-10 and the
// four draws made from it.  The only definition: every kernel (alll_kernels.hip, alll_small.hip) and
// the host's restatements (alll_host.cpp) call the functions below, with the key as (k0, k1) -- a
// context's seed or a group item's, low word first.  Compiles as device code under hipcc and as plain
// C++ without any HIP header.
//
//   fill             word w                   = Philox(key, {w,      0,     FILL,            0}).x
//   resample         word w, round it         = Philox(key, {w,      it_lo, RESAMPLE,        it_hi}).x
//   biased fill      variable v               = Philox(key, {v >> 2, 0,     BIASED_FILL,     0})[v & 3] < thr[v]
//   biased resample  variable v, round it     = Philox(key, {v >> 2, it_lo, BIASED_RESAMPLE, it_hi})[v & 3] < thr[v]
//
// (bit v % 32 of a word is variable v; thr == 0xFFFFFFFF always yields 1, thr == 0 never.)  Counter
// word 2 is the plane: the four planes are disjoint, so no two draws share a Philox call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ALLL_HD __host__ __device__ __forceinline__
#define ALLL_UNROLL _Pragma("unroll")
#else
#define ALLL_HD inline
#define ALLL_UNROLL
#endif

namespace alll {

// Four 32-bit words: a Philox counter or output in Random123 order, or the thresholds of a call's
// four variables (16 bytes, loaded at once).
struct alignas(16) Word4 {
    uint32_t x, y, z, w;
};

constexpr uint32_t PLANE_FILL = 0xFFFFFFFFu;
constexpr uint32_t PLANE_BIASED_FILL = 0xFFFFFFFEu;
constexpr uint32_t PLANE_RESAMPLE = 0u;
constexpr uint32_t PLANE_BIASED_RESAMPLE = 1u;

ALLL_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// Philox4x32-10, the constants of Random123 (pinned by its known-answer vectors through the oracle).
ALLL_HD Word4 philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    ALLL_UNROLL
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0;
        const uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Word4{c0, c1, c2, c3};
}

// ---- the unbiased draws: 32 variables per call, element 0
ALLL_HD uint32_t fill_word(uint32_t k0, uint32_t k1, uint32_t w) {
    return philox4(w, 0u, PLANE_FILL, 0u, k0, k1).x;
}
ALLL_HD uint32_t resample_word(uint32_t k0, uint32_t k1, uint64_t it, uint32_t w) {
    return philox4(w, (uint32_t)it, PLANE_RESAMPLE, (uint32_t)(it >> 32), k0, k1).x;
}

// ---- the biased draws: call q holds the words of the variables 4q .. 4q + 3
ALLL_HD Word4 biased_fill_call(uint32_t k0, uint32_t k1, uint32_t q) {
    return philox4(q, 0u, PLANE_BIASED_FILL, 0u, k0, k1);
}
ALLL_HD Word4 biased_resample_call(uint32_t k0, uint32_t k1, uint64_t it, uint32_t q) {
    return philox4(q, (uint32_t)it, PLANE_BIASED_RESAMPLE, (uint32_t)(it >> 32), k0, k1);
}
ALLL_HD uint32_t call_word(const Word4 u, uint32_t e) {  // element e of a call: variable 4q + e
    return e == 0 ? u.x : e == 1 ? u.y : e == 2 ? u.z : u.w;
}
// a variable is 1 when its word lies below its threshold (a word of 0xFFFFFFFF is below none: the pin)
ALLL_HD bool biased_bit(uint32_t u, uint32_t t) { return (u < t) | (t == 0xFFFFFFFFu); }
// -> bit j = the draw of the call's variable j
ALLL_HD uint32_t biased_bits4(const Word4 u, const Word4 t) {
    return (uint32_t)biased_bit(u.x, t.x) | (uint32_t)biased_bit(u.y, t.y) << 1 | (uint32_t)biased_bit(u.z, t.z) << 2 |
           (uint32_t)biased_bit(u.w, t.w) << 3;
}
// word w of the biased fill from its 32 thresholds t8[0..7]: the 8 calls 8w .. 8w + 7
ALLL_HD uint32_t biased_fill_word(uint32_t k0, uint32_t k1, uint32_t w, const Word4* t8) {
    uint32_t x = 0;
    ALLL_UNROLL
    for (uint32_t j = 0; j < 8; ++j) x |= biased_bits4(biased_fill_call(k0, k1, 8u * w + j), t8[j]) << (4 * j);
    return x;
}
// The 16 biased resample bits of a lane: the four calls q4 .. q4 + 3 of round `it`, their variables'
// thresholds t4[0..3] (64 contiguous bytes).  -> bit i = variable 4 * q4 + i.
ALLL_HD uint32_t biased_draw16(uint32_t k0, uint32_t k1, uint64_t it, uint32_t q4, const Word4* t4) {
    uint32_t x = 0;
    ALLL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) x |= biased_bits4(biased_resample_call(k0, k1, it, q4 + j), t4[j]) << (4 * j);
    return x;
}
// one variable's word of the biased resample (-> biased_bit with its threshold)
ALLL_HD uint32_t biased_resample_var(uint32_t k0, uint32_t k1, uint64_t it, uint32_t v) {
    return call_word(biased_resample_call(k0, k1, it, v >> 2), v & 3u);
}

}  // namespace alll
