// alll_score.hip -- split scores of the free variables (gfx950, wave64; include/alll.h, alll_var_scores;
// DESIGN.md §4.11).  One call is k_prop_pack (alll_propagate.hip: PM / PV from the thresholds) and
//   k_score_scan     a lane per clause, in clause order: the clause is classified and its free
//                    occurrences f counted, then an open clause adds w(f) to S[l] of every free
//                    occurrence (64-bit atomicAdd) and 1 to its item's n_open
//   k_score_pick_max a lane per assignment word: T = S[2v] + S[2v+1] of its 32 variables, the word's
//                    largest T and the lowest variable that has it; atomicMax of T per item
//   k_score_pick_var a lane per word: the words that hold their item's maximum, atomicMin of the variable
//   k_score_record   a lane per item: the record, in the item's local numbering
// Sums of integers, max and min: nothing depends on the order of the lanes.  No grid barrier, no
// spin-wait, no inline assembly.
#include "alll_score.h"

#include <algorithm>
#include <cstdlib>

#include "alll_rt_util.h"

namespace alll {

namespace {

constexpr uint32_t SCORE_LIT_MASK = 0x7FFFFFFFu;  // (bit 31 of the AoS literals: hot-variable flag)
constexpr int SCORE_THREADS = 256;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// AGG: the adds to a hot-flagged literal (a hub: thousands of clauses hold it) are summed over the
// wave's lanes that hold the same literal at the same position first, and one lane adds the sum.
// (Measured against the plain scan, DESIGN.md §4.11: within 3 % at 10 M clauses either way -- a wave
// holds a hub's literal once to three times per position; a workgroup-wide table would be the next step.)
template <bool AGG>
__global__ __launch_bounds__(SCORE_THREADS) void k_score_scan(const ScoreArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * SCORE_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = c < a.m;
    uint64_t j0 = 0, j1 = 0;
    if (valid) {
        if (a.k) {
            j0 = c * a.k;
            j1 = j0 + a.k;
        } else {
            j0 = a.offs[c];
            j1 = a.offs[c + 1];
        }
    }
    bool sat = false;
    uint32_t f = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t l = a.lits[j] & SCORE_LIT_MASK, v = l >> 1, sh = v & 31u;
        if ((a.PM[v >> 5] >> sh) & 1u) {
            if (((a.PV[v >> 5] >> sh) & 1u) != (l & 1u)) {  // a true literal
                sat = true;
                break;
            }
        } else {
            ++f;
        }
    }
    const bool open = valid && !sat;
    // the item's open clauses: per wave first where the wave lies in one item, then one atomic
    {
        const uint64_t c0 = c - lane;  // (the wave's first clause)
        bool one_item = true;
        uint32_t first = 0;
        if (a.clause_base && c0 < a.m) {
            const uint64_t cl = c0 + 63u < a.m ? c0 + 63u : a.m - 1u;
            first = prop_clause_item(a.clause_base, a.n_items, (uint32_t)c0);
            one_item = first == prop_clause_item(a.clause_base, a.n_items, (uint32_t)cl);
        }
        if (one_item) {
            const uint32_t sum = wave_sum(open ? 1u : 0u);
            if (lane == 0 && sum) atomicAdd(&a.n_open[first], (unsigned long long)sum);
        } else if (open) {
            atomicAdd(&a.n_open[prop_clause_item(a.clause_base, a.n_items, (uint32_t)c)], 1ull);
        }
    }
    const uint32_t w = 1u << (16u - (f < 16u ? f : 16u));
    const uint32_t len = (open && f) ? (uint32_t)(j1 - j0) : 0u;  // (an open clause holds no true literal)
    if (!AGG) {
        for (uint32_t q = 0; q < len; ++q) {
            const uint32_t l = a.lits[j0 + q] & SCORE_LIT_MASK, v = l >> 1;
            if (!((a.PM[v >> 5] >> (v & 31u)) & 1u)) atomicAdd(&a.S[l], (unsigned long long)w);
        }
        return;
    }
    // every lane of the wave walks the wave's longest clause: the shuffles below need all of them
    uint32_t max_len = len;
    for (int d = 32; d > 0; d >>= 1) max_len = max(max_len, (uint32_t)__shfl_xor(max_len, d));
    for (uint32_t q = 0; q < max_len; ++q) {
        uint32_t l = 0;
        bool pend = false;
        if (q < len) {
            const uint32_t raw = a.lits[j0 + q];
            l = raw & SCORE_LIT_MASK;
            const uint32_t v = l >> 1;
            if (!((a.PM[v >> 5] >> (v & 31u)) & 1u)) {
                if (raw >> 31) pend = true;
                else atomicAdd(&a.S[l], (unsigned long long)w);
            }
        }
        for (unsigned long long left = __ballot(pend); left; left = __ballot(pend)) {
            const uint32_t leader = (uint32_t)__ffsll(left) - 1u;
            const uint32_t L = __shfl(l, (int)leader);
            const bool mine = pend && l == L;
            const uint32_t sum = wave_sum(mine ? w : 0u);  // (at most 64 x 32768)
            if (lane == leader) atomicAdd(&a.S[L], (unsigned long long)sum);
            pend = pend && !mine;
        }
    }
}

__global__ __launch_bounds__(SCORE_THREADS) void k_score_pick_max(const ScoreArgs a) {
    const uint32_t w = blockIdx.x * SCORE_THREADS + threadIdx.x;
    const bool valid = w < a.n_words;
    uint32_t item = 0, var = ~0u;
    unsigned long long T = 0;
    if (valid) {
        item = a.word_item ? a.word_item[w] : 0u;
        uint32_t mask;
        if (a.words) mask = a.words[w].tail_mask;
        else mask = (w == a.n_words - 1u && (a.n_vars & 31u)) ? (1u << (a.n_vars & 31u)) - 1u : ~0u;
        const ulonglong2* s = reinterpret_cast<const ulonglong2*>(a.S + 64ull * w);  // S[2v], S[2v+1]
#pragma unroll 8
        for (uint32_t b = 0; b < 32; ++b) {
            const ulonglong2 x = s[b];
            const unsigned long long t = x.x + x.y;
            if (((mask >> b) & 1u) && t > T) {  // (ascending: the lowest variable keeps a tie)
                T = t;
                var = 32u * w + b;
            }
        }
        a.word_T[w] = T;
        a.word_v[w] = var;
    }
    // the item's maximum: per wave first where the wave lies in one item, then one atomic
    const uint32_t first = __shfl(item, 0);
    if (__all(!valid || item == first)) {
        unsigned long long mx = T;
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(mx, d);
            mx = o > mx ? o : mx;
        }
        if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&a.best_T[first], mx);
    } else if (T) {
        atomicMax(&a.best_T[item], T);
    }
}

__global__ __launch_bounds__(SCORE_THREADS) void k_score_pick_var(const ScoreArgs a) {
    const uint32_t w = blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (w >= a.n_words) return;
    const uint32_t item = a.word_item ? a.word_item[w] : 0u;
    const unsigned long long T = a.word_T[w];
    if (T && T == a.best_T[item]) atomicMin(&a.best_v[item], a.word_v[w]);
}

__global__ __launch_bounds__(SCORE_THREADS) void k_score_record(const ScoreArgs a) {
    const uint32_t i = blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (i >= a.n_items) return;
    const uint32_t var_base = a.item_vars[2 * i], n_vars = a.item_vars[2 * i + 1], v = a.best_v[i];
    alll_split_result r{0, 0, a.n_open[i], n_vars, 0};
    if (v != ~0u) {
        r.score_pos = a.S[2ull * v];
        r.score_neg = a.S[2ull * v + 1];
        r.var = v - var_base;
    }
    a.res[i] = r;
}

// (measurement, DESIGN.md §4.11: ALLL_SCORE_PLAIN=1 runs the scan without the wave's aggregation)
bool score_plain() {
    const char* e = getenv("ALLL_SCORE_PLAIN");
    return e && atoi(e) != 0;
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + SCORE_THREADS - 1) / SCORE_THREADS)); }

}  // namespace

int score_drive(const PropArgs& p, const std::vector<uint32_t>& item_vars, alll_split_result* results,
                std::vector<uint64_t>* S_host, hipStream_t s) {
    const uint32_t n = p.n_items, nw = p.n_words;
    if (n == 0) return ALLL_OK;
    // one allocation: S and the 64-bit arrays first, then the 32-bit ones
    const size_t n_S = 64ull * nw;
    const size_t bytes64 = (n_S + nw + 2ull * n) * 8 + sizeof(alll_split_result) * n;
    const size_t bytes32 = (4ull * nw + nw + n + 2ull * n) * 4;
    char* base = nullptr;
    if (hipMalloc((void**)&base, bytes64 + bytes32 + 16) != hipSuccess)
        return fail(ALLL_ERR_OOM, "var scores: hipMalloc(%zu bytes) failed", bytes64 + bytes32 + 16);
    ScoreArgs a{};
    a.lits = p.lits;
    a.offs = p.offs;
    a.m = p.m;
    a.k = p.k;
    a.n_vars = p.n_vars;
    a.n_words = nw;
    a.n_items = n;
    a.words = p.words;
    a.word_item = n > 1 ? p.word_item : nullptr;
    a.clause_base = n > 1 ? p.clause_base : nullptr;
    a.S = reinterpret_cast<unsigned long long*>(base);
    a.word_T = a.S + n_S;
    a.n_open = a.word_T + nw;
    a.best_T = a.n_open + n;
    a.res = reinterpret_cast<alll_split_result*>(a.best_T + n);
    uint32_t* bits = reinterpret_cast<uint32_t*>(base + bytes64);  // PM, PV, F1, F0 (k_prop_pack clears the last two)
    a.PM = bits;
    a.PV = bits + nw;
    a.word_v = bits + 4ull * nw;
    a.best_v = a.word_v + nw;
    uint32_t* d_item_vars = a.best_v + n;
    a.item_vars = d_item_vars;
    PropArgs pk = p;
    pk.PM = bits;
    pk.PV = bits + nw;
    pk.F1 = bits + 2ull * nw;
    pk.F0 = bits + 3ull * nw;
    auto run = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(d_item_vars, item_vars.data(), 8ull * n, hipMemcpyHostToDevice));
        // S, word_T, n_open and best_T start at 0
        HIP_TRY(hipMemsetAsync(base, 0, (n_S + nw + 2ull * n) * 8, s));
        HIP_TRY(hipMemsetAsync(a.best_v, 0xFF, 4ull * n, s));
        if (p.thr) HIP_TRY(launch_prop_pack(pk, s));
        else if (nw) HIP_TRY(hipMemsetAsync(bits, 0, 8ull * nw, s));  // every variable free
        if (a.m) {
            if (score_plain()) hipLaunchKernelGGL(k_score_scan<false>, grid_for(a.m), dim3(SCORE_THREADS), 0, s, a);
            else hipLaunchKernelGGL(k_score_scan<true>, grid_for(a.m), dim3(SCORE_THREADS), 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        if (nw) {
            hipLaunchKernelGGL(k_score_pick_max, grid_for(nw), dim3(SCORE_THREADS), 0, s, a);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_score_pick_var, grid_for(nw), dim3(SCORE_THREADS), 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_score_record, grid_for(n), dim3(SCORE_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(results, a.res, sizeof(alll_split_result) * n, hipMemcpyDeviceToHost));
        if (S_host) {
            S_host->resize(n_S);
            if (n_S) HIP_TRY(hipMemcpy(S_host->data(), a.S, n_S * 8, hipMemcpyDeviceToHost));
        }
        return ALLL_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(base);
    return rc;
}

}  // namespace alll
