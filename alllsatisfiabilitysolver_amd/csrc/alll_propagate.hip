// alll_propagate.hip -- unit propagation of the pinned variables (gfx950, wave64; include/alll.h,
// alll_propagate_pins).  A round is three launches:
//   k_prop_pack   (once per call) a lane per assignment word: its 32 thresholds (128 contiguous bytes)
//                 into a bit of PM (pinned) and of PV (value), which the scan gathers from
//   k_prop_scan   a lane per clause, in clause order: a falsified clause lowers its item's conflict
//                 word (atomicMin), a unit sets its variable's bit in F1 or F0 (atomicOr)
//   k_prop_apply  a lane per word: new = (F1 | F0) & ~PM becomes pins in PM, PV and the thresholds,
//                 unless the word's item has ended or the scan found it a conflict; F1, F0 cleared
// and the host reads the items' records in between (prop_drive).  Every clause of a round is judged
// against the PM / PV of the round's start (the scan only reads them, the apply only writes them), and
// min / or do not depend on the order of the lanes.  No grid barrier, no spin-wait, no inline assembly.
#include "alll_propagate.h"

#include <algorithm>

#include "alll_rt_util.h"

namespace alll {

namespace {

constexpr uint32_t PROP_LIT_MASK = 0x7FFFFFFFu;  // (bit 31 of the AoS literals: hot-variable flag)
constexpr int PROP_THREADS = 256;

__global__ __launch_bounds__(PROP_THREADS) void k_prop_pack(const PropArgs a) {
    const uint32_t w = blockIdx.x * PROP_THREADS + threadIdx.x;
    if (w >= a.n_words) return;
    // the word's variables that can be pins: those of an item that has thresholds, not its padding
    uint32_t valid;
    if (a.words) {
        valid = ((a.wbias[w >> 5] >> (w & 31u)) & 1u) ? a.words[w].tail_mask : 0u;
    } else {
        valid = (w == a.n_words - 1u && (a.n_vars & 31u)) ? (1u << (a.n_vars & 31u)) - 1u : ~0u;
    }
    const uint4* t = reinterpret_cast<const uint4*>(a.thr + 32ull * w);
    uint32_t pm = 0, pv = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
        const uint4 x = t[q];
        const uint32_t e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t bit = 1u << (4 * q + j);
            if (e[j] == 0u || e[j] == 0xFFFFFFFFu) pm |= bit;
            if (e[j] == 0xFFFFFFFFu) pv |= bit;
        }
    }
    a.PM[w] = pm & valid;
    a.PV[w] = pv & valid;
    a.F1[w] = 0;
    a.F0[w] = 0;
}

__global__ __launch_bounds__(PROP_THREADS) void k_prop_scan(const PropArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * PROP_THREADS + threadIdx.x;
    if (c >= a.m) return;
    uint64_t j0, j1;
    if (a.k) {
        j0 = c * a.k;
        j1 = j0 + a.k;
    } else {
        j0 = a.offs[c];
        j1 = a.offs[c + 1];
    }
    // (the PV word is needed for a pinned variable only: most gathers are the PM word's alone.  A
    // variant for the fixed widths that issued all K literal loads and all 2 K gathers before judging
    // the clause was slower at 10 M clauses, 193 us against 124 us: DESIGN.md §4.10)
    bool sat = false, same = true;
    uint32_t n_free = 0, unit = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t l = a.lits[j] & PROP_LIT_MASK, v = l >> 1, sh = v & 31u;
        const uint32_t pm = (a.PM[v >> 5] >> sh) & 1u;
        if (pm) {
            const uint32_t pv = (a.PV[v >> 5] >> sh) & 1u;
            if (pv != (l & 1u)) {  // a true literal
                sat = true;
                break;
            }
        } else if (n_free++ == 0) {
            unit = l;
        } else {
            same = same && l == unit;
        }
    }
    if (sat || (n_free && !same)) return;
    if (n_free == 0) {
        const uint32_t i = a.clause_base ? prop_clause_item(a.clause_base, a.n_items, (uint32_t)c) : 0u;
        atomicMin(&a.items[i].conflict, (unsigned long long)c);
    } else {
        const uint32_t v = unit >> 1;
        atomicOr(((unit & 1u) ? a.F0 : a.F1) + (v >> 5), 1u << (v & 31u));
    }
}

template <bool DRY>
__global__ __launch_bounds__(PROP_THREADS) void k_prop_apply(const PropArgs a) {
    const uint32_t w = blockIdx.x * PROP_THREADS + threadIdx.x;
    uint32_t item = 0, n_new = 0;
    if (w < a.n_words) {
        item = a.word_item ? a.word_item[w] : 0u;
        const uint32_t f1 = a.F1[w], f0 = a.F0[w];
        if (f1 | f0) {
            a.F1[w] = 0;
            a.F0[w] = 0;
            const PropItem& it = a.items[item];
            const uint32_t pm = a.PM[w];
            // (an ended item, and one the scan found a conflict in, keeps its thresholds)
            const uint32_t nw = (it.active && it.conflict == PROP_NO_CONFLICT) ? (f1 | f0) & ~pm : 0u;
            n_new = __popc(nw);
            if (nw && !DRY) {
                a.PM[w] = pm | nw;
                a.PV[w] = a.PV[w] | (nw & f1);  // (forced both ways: pinned to 1)
                for (uint32_t r = nw; r; r &= r - 1u) {
                    const uint32_t bit = __ffs(r) - 1u;
                    a.thr[32ull * w + bit] = ((f1 >> bit) & 1u) ? 0xFFFFFFFFu : 0u;
                }
            }
        }
    }
    // the round's forced count: per wave first where the wave lies in one item, then one atomic
    const uint32_t first = __shfl(item, 0);
    if (__all(item == first)) {
        uint32_t sum = n_new;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&a.items[first].forced, sum);
    } else if (n_new) {
        atomicAdd(&a.items[item].forced, n_new);
    }
}

}  // namespace

hipError_t launch_prop_pack(const PropArgs& a, hipStream_t s) {
    if (a.n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_prop_pack, dim3((a.n_words + PROP_THREADS - 1) / PROP_THREADS), dim3(PROP_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_prop_scan(const PropArgs& a, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_prop_scan, dim3((uint32_t)((a.m + PROP_THREADS - 1) / PROP_THREADS)), dim3(PROP_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_prop_apply(const PropArgs& a, bool dry, hipStream_t s) {
    if (a.n_words == 0) return hipSuccess;
    const dim3 grid((a.n_words + PROP_THREADS - 1) / PROP_THREADS), block(PROP_THREADS);
    if (dry) hipLaunchKernelGGL(k_prop_apply<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_prop_apply<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

int prop_drive(PropArgs a, const uint8_t* on, uint64_t max_rounds, alll_propagate_result* results, hipStream_t s) {
    const uint32_t n = a.n_items;
    std::vector<PropItem> rec(n);
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        rec[i] = PropItem{PROP_NO_CONFLICT, 0u, on[i] ? 1u : 0u};
        results[i] = alll_propagate_result{a.m, 0, 0, on[i] ? ALLL_PROP_FIXPOINT : ALLL_PROP_NONE};
        any = any || on[i];
    }
    if (!any) return ALLL_OK;
    uint32_t* bits = nullptr;  // PM, PV, F1, F0
    PropItem* d_rec = nullptr;
    const size_t wbytes = (size_t)a.n_words * 4;
    if (hipMalloc((void**)&bits, std::max<size_t>(4 * wbytes, 16)) != hipSuccess)
        return fail(ALLL_ERR_OOM, "propagate: hipMalloc(%zu bytes) failed", 4 * wbytes);
    if (hipMalloc((void**)&d_rec, sizeof(PropItem) * n) != hipSuccess) {
        (void)hipFree(bits);
        return fail(ALLL_ERR_OOM, "propagate: hipMalloc(%zu bytes) failed", sizeof(PropItem) * n);
    }
    a.PM = bits;
    a.PV = bits + a.n_words;
    a.F1 = bits + 2ull * a.n_words;
    a.F0 = bits + 3ull * a.n_words;
    a.items = d_rec;
    auto run = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(d_rec, rec.data(), sizeof(PropItem) * n, hipMemcpyHostToDevice));
        HIP_TRY(launch_prop_pack(a, s));
        // every applying round pins at least one more variable of every item it keeps active
        const uint64_t bound = max_rounds ? max_rounds : (uint64_t)a.n_vars + 1;
        for (uint64_t round = 0; round <= bound; ++round) {
            const bool dry = round >= bound;
            HIP_TRY(launch_prop_scan(a, s));
            HIP_TRY(launch_prop_apply(a, dry, s));
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipMemcpy(rec.data(), d_rec, sizeof(PropItem) * n, hipMemcpyDeviceToHost));
            bool left = false;
            for (uint32_t i = 0; i < n; ++i) {
                PropItem& r = rec[i];
                if (!r.active) continue;
                alll_propagate_result& o = results[i];
                if (r.conflict != PROP_NO_CONFLICT) {
                    o.status = ALLL_PROP_CONFLICT;
                    o.conflict_clause = r.conflict;
                    r.active = 0;
                } else if (r.forced == 0) {
                    o.status = ALLL_PROP_FIXPOINT;
                    r.active = 0;
                } else if (dry) {
                    o.status = ALLL_PROP_ROUND_CAP;
                    r.active = 0;
                } else {
                    o.rounds += 1;
                    o.n_forced += r.forced;
                    left = true;
                }
                r.forced = 0;
            }
            if (!left) return ALLL_OK;
            HIP_TRY(hipMemcpy(d_rec, rec.data(), sizeof(PropItem) * n, hipMemcpyHostToDevice));
        }
        return fail(ALLL_ERR_HIP, "propagate: the rounds did not end within their bound");
    };
    const int rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(bits);
    (void)hipFree(d_rec);
    return rc;
}

}  // namespace alll
