// alll_residual.hip -- the residual formula under the pins (gfx950, wave64; include/alll.h,
// alll_residual): a stable compaction of every item's clauses and variables.  One
// call is k_prop_pack (alll_propagate.hip: PM / PV from the thresholds) and a reduce / scan / emit
// scheme in tiles of RESID_TILE:
//   k_resid_classify    a lane per clause, in clause order: kept or dropped, its free occurrences f;
//                       the kept-variable bits in KM (atomicOr), the tile's sums of kept clauses and
//                       of residual literals, the item's falsified count and first falsified clause
//   k_resid_count_vars  a lane per assignment word: popcount(KM & tail_mask), the tile's sum
//   k_resid_scan_tiles  three workgroups, one per tile-sum array: its exclusive scan, RESID_TILE sums
//                       per trip with a carry
//   k_resid_item_bases  a lane per item boundary: kept clauses, residual literals and kept variables of
//                       the union before it (the tile's prefix and the part of the tile before it)
//   k_resid_emit_words  a lane per word: the word's prefix WP, var_map and thr_out of its kept variables
//   k_resid_emit_clauses a lane per clause: clause_map, the item-local offsets, the renumbered literals
//   k_resid_record      a lane per item: the record and the item's last offset
// Every position is a prefix sum of integers in clause (variable) order: nothing depends on the order
// of the lanes.  No decoupled look-back, no grid barrier, no spin-wait, no inline assembly.
#include "alll_residual.h"

#include <algorithm>

#include "alll_rt_util.h"

namespace alll {

namespace {

constexpr uint32_t RESID_LIT_MASK = 0x7FFFFFFFu;  // (bit 31 of the AoS literals: hot-variable flag)
constexpr unsigned long long RESID_NONE = ~0ull;
constexpr int RESID_WAVES = RESID_TILE / 64;

// Exclusive prefix of x over the workgroup's RESID_TILE lanes and the workgroup's total.  sh:
// RESID_WAVES entries of LDS; every lane of the workgroup calls it.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T x, T* sh, T& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
    for (uint32_t i = 0; i < (uint32_t)RESID_WAVES; ++i) {
        if (i < wave) before += sh[i];
        all += sh[i];
    }
    __syncthreads();  // (sh is free for the next call)
    total = all;
    return before + inc - x;
}

__device__ __forceinline__ void clause_range(const ResidArgs& a, uint64_t c, uint64_t& j0, uint64_t& j1) {
    if (a.k) {
        j0 = c * a.k;
        j1 = j0 + a.k;
    } else {
        j0 = a.offs[c];
        j1 = a.offs[c + 1];
    }
}

__device__ __forceinline__ uint32_t word_mask(const ResidArgs& a, uint32_t w) {
    if (a.words) return a.words[w].tail_mask;
    return (w == a.n_words - 1u && (a.n_vars & 31u)) ? (1u << (a.n_vars & 31u)) - 1u : ~0u;
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_classify(const ResidArgs a) {
    __shared__ uint32_t sh[RESID_WAVES];
    const uint64_t c = (uint64_t)blockIdx.x * RESID_TILE + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = c < a.m;
    uint64_t j0 = 0, j1 = 0;
    if (valid) clause_range(a, c, j0, j1);
    bool sat = false;
    uint32_t f = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t l = a.lits[j] & RESID_LIT_MASK, v = l >> 1, sh_ = v & 31u;
        if ((a.PM[v >> 5] >> sh_) & 1u) {
            if (((a.PV[v >> 5] >> sh_) & 1u) != (l & 1u)) {  // a true literal
                sat = true;
                break;
            }
        } else {
            ++f;
        }
    }
    const bool kept = valid && !sat;
    if (!kept) f = 0;
    if (valid) a.keptlen[c] = kept ? f + 1u : 0u;
    // the kept variables: the free occurrences of a kept clause.  The mask only grows, so the bit is
    // tested first, with a load of device scope (where the atomics land).  (Measured against a plain
    // load at 10 M clauses: 937 us against 928 us, no difference -- DESIGN.md §4.12.)
    if (f) {
        for (uint64_t j = j0; j < j1; ++j) {
            const uint32_t v = (a.lits[j] & RESID_LIT_MASK) >> 1, bit = 1u << (v & 31u);
            if ((a.PM[v >> 5] & bit) == 0u &&
                (__hip_atomic_load(&a.KM[v >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u)
                atomicOr(&a.KM[v >> 5], bit);
        }
    }
    // the item's falsified clauses: per wave first where the wave lies in one item, then one atomic
    {
        const bool dead = kept && f == 0;
        const uint64_t c0 = c - lane;  // (the wave's first clause)
        bool one_item = true;
        uint32_t first = 0;
        if (a.clause_base && c0 < a.m) {
            const uint64_t cl = c0 + 63u < a.m ? c0 + 63u : a.m - 1u;
            first = prop_clause_item(a.clause_base, a.n_items, (uint32_t)c0);
            one_item = first == prop_clause_item(a.clause_base, a.n_items, (uint32_t)cl);
        }
        if (one_item) {
            const unsigned long long deads = __ballot(dead);
            if (lane == 0 && deads) {
                atomicAdd(&a.n_fals[first], (unsigned long long)__popcll(deads));
                atomicMin(&a.first_fals[first], (unsigned long long)(c0 + (uint32_t)__ffsll(deads) - 1u));
            }
        } else if (dead) {
            const uint32_t i = prop_clause_item(a.clause_base, a.n_items, (uint32_t)c);
            atomicAdd(&a.n_fals[i], 1ull);
            atomicMin(&a.first_fals[i], (unsigned long long)c);
        }
    }
    uint32_t n_kept, n_lits;
    block_excl_scan<uint32_t>(kept ? 1u : 0u, sh, n_kept);
    block_excl_scan<uint32_t>(f, sh, n_lits);
    if (threadIdx.x == 0) {
        a.ts_c[blockIdx.x] = n_kept;
        a.ts_l[blockIdx.x] = n_lits;
    }
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_count_vars(const ResidArgs a) {
    __shared__ uint32_t sh[RESID_WAVES];
    const uint32_t w = blockIdx.x * RESID_TILE + threadIdx.x;
    const uint32_t cnt = w < a.n_words ? __popc(a.KM[w] & word_mask(a, w)) : 0u;
    uint32_t total;
    block_excl_scan<uint32_t>(cnt, sh, total);
    if (threadIdx.x == 0) a.ts_v[blockIdx.x] = total;
}

// blockIdx.x: 0 kept clauses, 1 residual literals, 2 kept variables
__global__ __launch_bounds__(RESID_TILE) void k_resid_scan_tiles(const ResidArgs a) {
    __shared__ unsigned long long sh[RESID_WAVES];
    const uint32_t* ts = blockIdx.x == 0 ? a.ts_c : blockIdx.x == 1 ? a.ts_l : a.ts_v;
    unsigned long long* tp = blockIdx.x == 0 ? a.tp_c : blockIdx.x == 1 ? a.tp_l : a.tp_v;
    const uint32_t T = blockIdx.x == 2 ? a.n_tiles_w : a.n_tiles_c;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < T; base += RESID_TILE) {  // (uniform over the workgroup)
        const uint32_t i = base + threadIdx.x;
        unsigned long long total;
        const unsigned long long before = block_excl_scan<unsigned long long>(i < T ? ts[i] : 0u, sh, total);
        if (i < T) tp[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) tp[T] = carry;
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_item_bases(const ResidArgs a) {
    const uint32_t i = blockIdx.x * RESID_TILE + threadIdx.x;
    if (i > a.n_items) return;
    // (an item's end is the next item's start; the last boundary is the union's end)
    const uint64_t cb = i < a.n_items ? a.items[i].clause_base : a.m;
    const uint32_t wb = i < a.n_items ? a.items[i].word_base : a.n_words;
    const uint64_t tc = cb / RESID_TILE;
    unsigned long long bc = a.tp_c[tc], bl = a.tp_l[tc];
    for (uint64_t c = tc * RESID_TILE; c < cb; ++c) {
        const uint32_t kl = a.keptlen[c];
        if (kl) {
            bc += 1u;
            bl += kl - 1u;
        }
    }
    const uint32_t tw = wb / RESID_TILE;
    unsigned long long bv = a.tp_v[tw];
    for (uint32_t w = tw * RESID_TILE; w < wb; ++w) bv += __popc(a.KM[w] & word_mask(a, w));
    a.base_c[i] = bc;
    a.base_l[i] = bl;
    a.base_v[i] = bv;
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_emit_words(const ResidArgs a) {
    __shared__ uint32_t sh[RESID_WAVES];
    const uint32_t w = blockIdx.x * RESID_TILE + threadIdx.x;
    const bool valid = w < a.n_words;
    const uint32_t km = valid ? a.KM[w] & word_mask(a, w) : 0u;
    uint32_t total;
    const uint32_t wp = (uint32_t)a.tp_v[blockIdx.x] + block_excl_scan<uint32_t>(__popc(km), sh, total);
    if (!valid) return;
    a.WP[w] = wp;
    if (!a.out_var_map || !km) return;
    const uint32_t var_base = a.items[a.word_item ? a.word_item[w] : 0u].var_base;
    const bool biased = a.thr && (!a.wbias || ((a.wbias[w >> 5] >> (w & 31u)) & 1u));
    uint32_t u = wp;
    for (uint32_t r = km; r; r &= r - 1u, ++u) {
        const uint32_t v = 32u * w + (uint32_t)__ffs(r) - 1u;
        a.out_var_map[u] = v - var_base;
        a.out_thr[u] = biased ? a.thr[v] : 0x80000000u;
    }
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_emit_clauses(const ResidArgs a) {
    __shared__ uint32_t sh[RESID_WAVES];
    const uint64_t c = (uint64_t)blockIdx.x * RESID_TILE + threadIdx.x;
    const uint32_t kl = c < a.m ? a.keptlen[c] : 0u;
    const uint32_t f = kl ? kl - 1u : 0u;
    uint32_t total;
    const uint32_t kept_before = block_excl_scan<uint32_t>(kl ? 1u : 0u, sh, total);
    const uint32_t lits_before = block_excl_scan<uint32_t>(f, sh, total);
    if (!kl) return;
    const uint32_t i = a.clause_base ? prop_clause_item(a.clause_base, a.n_items, (uint32_t)c) : 0u;
    const unsigned long long pc = a.tp_c[blockIdx.x] + kept_before;
    unsigned long long pl = a.tp_l[blockIdx.x] + lits_before;
    a.out_clause_map[pc] = c - a.items[i].clause_base;
    a.out_offsets[pc + i] = pl - a.base_l[i];
    if (!f) return;
    const uint32_t var0 = (uint32_t)a.base_v[i];
    uint64_t j0, j1;
    clause_range(a, c, j0, j1);
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t l = a.lits[j] & RESID_LIT_MASK, v = l >> 1, bit = 1u << (v & 31u);
        if (a.PM[v >> 5] & bit) continue;
        const uint32_t u = a.WP[v >> 5] + __popc(a.KM[v >> 5] & (bit - 1u)) - var0;
        a.out_lits[pl++] = 2u * u + (l & 1u);
    }
}

__global__ __launch_bounds__(RESID_TILE) void k_resid_record(const ResidArgs a) {
    const uint32_t i = blockIdx.x * RESID_TILE + threadIdx.x;
    if (i >= a.n_items) return;
    const ResidItem it = a.items[i];
    const unsigned long long first = a.first_fals[i];
    alll_residual_result r;
    r.n_clauses = a.base_c[i + 1] - a.base_c[i];
    r.n_literals = a.base_l[i + 1] - a.base_l[i];
    r.n_falsified = a.n_fals[i];
    r.first_falsified = first == RESID_NONE ? it.n_clauses : first - it.clause_base;
    r.n_vars = (uint32_t)(a.base_v[i + 1] - a.base_v[i]);
    r.pad = 0;
    a.res[i] = r;
    if (a.out_offsets) a.out_offsets[a.base_c[i + 1] + i] = r.n_literals;
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + RESID_TILE - 1) / RESID_TILE)); }

// carves arrays out of one allocation, each at a multiple of 16 bytes
struct Carver {
    size_t at = 0;
    char* base = nullptr;
    template <typename T>
    T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;  // (no base: the sizing walk)
        at += (n * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
};

}  // namespace

int resid_drive(const PropArgs& p, const std::vector<ResidItem>& items, uint64_t n_literals,
                alll_residual_result* results, const ResidOut& out, hipStream_t s) {
    const uint32_t n = p.n_items, nw = p.n_words;
    if (n == 0) return ALLL_OK;
    const bool arrays = out.offsets || out.literals || out.var_map || out.clause_map || out.thr_out;
    ResidArgs a{};
    a.lits = p.lits;
    a.offs = p.offs;
    a.m = p.m;
    a.k = p.k;
    a.n_vars = p.n_vars;
    a.n_words = nw;
    a.n_items = n;
    a.n_tiles_c = (uint32_t)((p.m + RESID_TILE - 1) / RESID_TILE);
    a.n_tiles_w = (nw + RESID_TILE - 1) / RESID_TILE;
    a.thr = p.thr;
    a.words = p.words;
    a.wbias = p.wbias;
    a.word_item = n > 1 ? p.word_item : nullptr;
    a.clause_base = n > 1 ? p.clause_base : nullptr;
    uint32_t* bits = nullptr;      // PM, PV, F1, F0 (k_prop_pack clears the last two)
    ResidItem* d_items = nullptr;
    size_t zero_bytes = 0;         // the head of the allocation that starts at 0: n_fals, KM
    auto carve = [&](char* base) {
        Carver cv;
        cv.base = base;
        a.n_fals = cv.take<unsigned long long>(n);
        a.KM = cv.take<uint32_t>(nw);
        zero_bytes = cv.at;
        a.first_fals = cv.take<unsigned long long>(n);
        a.base_c = cv.take<unsigned long long>(n + 1ull);
        a.base_l = cv.take<unsigned long long>(n + 1ull);
        a.base_v = cv.take<unsigned long long>(n + 1ull);
        a.tp_c = cv.take<unsigned long long>(a.n_tiles_c + 1ull);
        a.tp_l = cv.take<unsigned long long>(a.n_tiles_c + 1ull);
        a.tp_v = cv.take<unsigned long long>(a.n_tiles_w + 1ull);
        a.res = cv.take<alll_residual_result>(n);
        a.ts_c = cv.take<uint32_t>(a.n_tiles_c);
        a.ts_l = cv.take<uint32_t>(a.n_tiles_c);
        a.ts_v = cv.take<uint32_t>(a.n_tiles_w);
        bits = cv.take<uint32_t>(4ull * nw);
        a.WP = cv.take<uint32_t>(nw);
        a.keptlen = cv.take<uint32_t>(p.m);
        d_items = cv.take<ResidItem>(n);
        if (arrays) {
            a.out_offsets = cv.take<unsigned long long>(p.m + n);
            a.out_clause_map = cv.take<unsigned long long>(p.m);
            a.out_lits = cv.take<uint32_t>(n_literals);
            a.out_var_map = cv.take<uint32_t>(p.n_vars);
            a.out_thr = cv.take<uint32_t>(p.n_vars);
        }
        return cv.at;
    };
    const size_t bytes = carve(nullptr) + 16;
    char* base = nullptr;
    if (hipMalloc((void**)&base, bytes) != hipSuccess)
        return fail(ALLL_ERR_OOM, "residual: hipMalloc(%zu bytes) failed", bytes);
    carve(base);
    a.items = d_items;
    a.PM = bits;
    a.PV = bits + nw;
    PropArgs pk = p;
    pk.PM = bits;
    pk.PV = bits + nw;
    pk.F1 = bits + 2ull * nw;
    pk.F0 = bits + 3ull * nw;
    auto run = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(d_items, items.data(), sizeof(ResidItem) * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(base, 0, zero_bytes, s));
        HIP_TRY(hipMemsetAsync(a.first_fals, 0xFF, 8ull * n, s));
        if (p.thr) HIP_TRY(launch_prop_pack(pk, s));
        else if (nw) HIP_TRY(hipMemsetAsync(bits, 0, 8ull * nw, s));  // every variable free
        const dim3 block(RESID_TILE);
        if (a.m) {
            hipLaunchKernelGGL(k_resid_classify, grid_for(a.m), block, 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        if (nw) {
            hipLaunchKernelGGL(k_resid_count_vars, grid_for(nw), block, 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_resid_scan_tiles, dim3(3), block, 0, s, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_resid_item_bases, grid_for(n + 1ull), block, 0, s, a);
        HIP_TRY(hipGetLastError());
        if (arrays && nw) {
            hipLaunchKernelGGL(k_resid_emit_words, grid_for(nw), block, 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        if (arrays && a.m) {
            hipLaunchKernelGGL(k_resid_emit_clauses, grid_for(a.m), block, 0, s, a);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_resid_record, grid_for(n), block, 0, s, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(results, a.res, sizeof(alll_residual_result) * n, hipMemcpyDeviceToHost));
        // the used prefixes only
        uint64_t nc = 0, nl = 0, nv = 0;
        for (uint32_t i = 0; i < n; ++i) {
            nc += results[i].n_clauses;
            nl += results[i].n_literals;
            nv += results[i].n_vars;
        }
        if (nc > p.m || nl > n_literals || nv > p.n_vars)
            return fail(ALLL_ERR_HIP, "residual: the compaction exceeds the instance (%llu clauses, %llu literals, "
                        "%llu variables)", (unsigned long long)nc, (unsigned long long)nl, (unsigned long long)nv);
        if (out.offsets) HIP_TRY(hipMemcpy(out.offsets, a.out_offsets, 8ull * (nc + n), hipMemcpyDeviceToHost));
        if (out.clause_map && nc) HIP_TRY(hipMemcpy(out.clause_map, a.out_clause_map, 8ull * nc, hipMemcpyDeviceToHost));
        if (out.literals && nl) HIP_TRY(hipMemcpy(out.literals, a.out_lits, 4ull * nl, hipMemcpyDeviceToHost));
        if (out.var_map && nv) HIP_TRY(hipMemcpy(out.var_map, a.out_var_map, 4ull * nv, hipMemcpyDeviceToHost));
        if (out.thr_out && nv) HIP_TRY(hipMemcpy(out.thr_out, a.out_thr, 4ull * nv, hipMemcpyDeviceToHost));
        return ALLL_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(base);
    return rc;
}

}  // namespace alll
