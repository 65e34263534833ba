// alll_probe.hip -- failed-literal probing: 64 propagations per pass over the clauses (gfx950, wave64;
// include/alll.h, alll_probe_literals).  A slab is 64 probes; per slab and variable
// two 64-bit words hold "pinned by probe p's own propagation" (DM) and "its value" (DV), bit p for
// probe p.  The base's pins stay in the 1-bit PM / PV bitmaps of k_prop_pack (alll_propagate.hip).
// A chunk of slabs goes through the same launches, the slab is the grid's second dimension:
//   k_probe_seed    a lane per probe: bit p of DM[v] (and of DV[v] for a positive literal), 64-bit
//                   atomicOr -- probes of a slab may share a variable; a probe on a variable the base
//                   pins is ALLL_PROP_NONE and never runs
// and per round
//   k_probe_scan    a lane per clause, in clause order: the clause is read once and judged for the 64
//                   probes in 64-bit registers (sat; one, two: a saturating count of distinct free
//                   literals); a falsified clause lowers the probe's conflict word (atomicMin), a
//                   unit sets the probes' bits in F1[v] or F0[v] (64-bit atomicOr).  Nothing else is
//                   written: every clause is judged against the round's start
//   k_probe_judge   64 lanes per slab: the probes whose new variables are counted (running, no
//                   conflict) and those whose units are applied (not at the cap of max_rounds)
//   k_probe_apply   a lane per variable: new = (F1 | F0) & ~DM becomes pins in DM / DV under the apply
//                   mask (forced both ways: 1 wins), F1 and F0 cleared, the new bits counted per probe
//   k_probe_settle  64 lanes per slab: conflict, fixpoint (nothing new), round cap or one more round;
//                   the slab's mask of running probes, and the word the host reads per round
// then k_probe_rows: the 64 x 64 bit transpose (lane = variable, __ballot of bit p = 64 variables of
// probe p) into the probes' rows, OR-ed with the base bitmaps.  min / or / sums of integers: nothing
// depends on the order of the lanes.  No grid barrier, no spin-wait, no inline assembly.
#include "alll_probe.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "alll_rt_util.h"

namespace alll {

namespace {

typedef unsigned long long u64;

constexpr uint32_t PROBE_LIT_MASK = 0x7FFFFFFFu;  // (bit 31 of the AoS literals: hot-variable flag)
constexpr int PROBE_THREADS = 256;
constexpr uint32_t PROBE_REG_WIDTH = 8;           // clauses up to this width are judged from registers

__device__ __forceinline__ uint32_t base_bit(const uint32_t* B, uint32_t v) { return (B[v >> 5] >> (v & 31u)) & 1u; }

// The kernels are written once, for the argument struct A: ProbeArgs is a context (the grid's second
// dimension is the slab), GroupProbeArgs a group (it is the layer; masks and records are per slot).
template <class A>
constexpr bool IS_GROUP = std::is_same<A, GroupProbeArgs>::value;

// the slot of (item, layer y of the chunk), ~0u: the item has no probe there
__device__ __forceinline__ uint32_t group_slot(const GroupProbeArgs& a, uint32_t item, uint32_t y) {
    const uint32_t s0 = a.slot_base[item];
    return y < a.slot_base[item + 1] - s0 ? s0 + y : ~0u;
}

template <class A>
__global__ __launch_bounds__(64) void k_probe_seed(const A a) {
    const uint32_t slab = blockIdx.x, lane = threadIdx.x, p = slab * PROBE_SLAB + lane;
    bool run = false;
    uint32_t l = 0, layer = slab, var0 = 0;  // the probe's literal, its delta layer, its item's first variable
    bool have;
    if constexpr (IS_GROUP<A>) {
        const uint32_t item = a.slot_item[slab];
        const GroupProbeItem it = a.items[item];
        layer = slab - a.slot_base[item];
        const uint32_t q = (a.layer0 + layer) * PROBE_SLAB + lane;  // (the item's own probe index)
        have = q < it.n_probes;
        if (have) l = a.probes[it.probe_base + q];
        var0 = 32u * it.word_base;
    } else {
        have = p < a.n_probes;
        if (have) l = a.probes[p];
    }
    if (have) {
        const uint32_t v = var0 + (l >> 1);
        run = !base_bit(a.PM, v);
        if (run) {
            const size_t at = (size_t)layer * a.nv_pad + v;
            atomicOr(a.DM + at, 1ull << lane);
            if (!(l & 1u)) atomicOr(a.DV + at, 1ull << lane);
        }
    }
    a.rec[p] = ProbeRec{PROP_NO_CONFLICT, 0u, 0u, 0u, run ? ALLL_PROP_FIXPOINT : ALLL_PROP_NONE};
    const u64 act = __ballot(run);
    if (lane == 0) {
        a.act[slab] = act;
        a.cnt[slab] = 0;
        a.app[slab] = 0;
    }
}

template <class A>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_scan(const A a) {
    uint32_t slab = blockIdx.y;  // (a group: the layer here, the clause's slot below)
    const uint32_t layer = blockIdx.y;
    uint64_t c;
    u64 act;
    if constexpr (IS_GROUP<A>) {
        c = (uint64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
        // the clause's item: one lookup for the workgroup when its first and last clause share an item
        // (act is then a uniform load, and a workgroup without a running probe returns at once)
        const uint64_t b0 = (uint64_t)blockIdx.x * PROBE_THREADS;  // (the union's clause indices fit 32 bits)
        if (b0 >= a.m) return;
        const uint32_t c0 = (uint32_t)b0, c1 = (uint32_t)((b0 + PROBE_THREADS < a.m ? b0 + PROBE_THREADS : a.m) - 1u);
        const uint32_t i0 = prop_clause_item(a.clause_base, a.n_items, c0);
        if (a.clause_base[i0 + 1] > c1) {
            slab = group_slot(a, i0, layer);
            if (slab == ~0u) return;
            act = a.act[slab];
            if (!act || c >= a.m) return;
        } else {
            if (c >= a.m) return;
            slab = group_slot(a, prop_clause_item(a.clause_base, a.n_items, (uint32_t)c), layer);
            if (slab == ~0u) return;
            act = a.act[slab];
            if (!act) return;
        }
    } else {
        act = a.act[slab];
        if (!act) return;  // (every probe of the slab has ended)
        c = (uint64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
        if (c >= a.m) return;
    }
    uint64_t j0, j1;
    if (a.k) {
        j0 = c * a.k;
        j1 = j0 + a.k;
    } else {
        j0 = a.offs[c];
        j1 = a.offs[c + 1];
    }
    const size_t s0 = (size_t)layer * a.nv_pad;
    const u64 *DM = a.DM + s0, *DV = a.DV + s0;
    u64 *F1 = a.F1 + s0, *F0 = a.F0 + s0;
    const uint32_t len = (uint32_t)(j1 - j0);
    // sat: probes in which a literal is true; one / two: probes with at least one / two distinct free
    // literals.  A literal is judged from the base bit first, else from bit p of DM / DV: a variable
    // the base pins never has its delta words fetched.  An occurrence equal to an earlier literal of
    // the clause counts once (the identity of a literal is the same in all 64 probes).
    u64 sat = 0, one = 0, two = 0;
    if (len <= PROBE_REG_WIDTH) {
        uint32_t L[PROBE_REG_WIDTH];  // the distinct literals the base leaves free (~0u: none at i)
        u64 FR[PROBE_REG_WIDTH];      // ... the probes in which they are free
#pragma unroll
        for (uint32_t i = 0; i < PROBE_REG_WIDTH; ++i) {
            L[i] = ~0u;
            FR[i] = 0;
            if (i < len && (act & ~sat)) {
                const uint32_t l = a.lits[j0 + i] & PROBE_LIT_MASK, v = l >> 1;
                if (base_bit(a.PM, v)) {
                    if (base_bit(a.PV, v) != (l & 1u)) sat = ~0ull;  // true in the base
                } else {
                    bool dup = false;
#pragma unroll
                    for (uint32_t q = 0; q < i; ++q) dup = dup || L[q] == l;
                    if (!dup) {
                        const u64 dm = DM[v];
                        if (dm) {
                            const u64 dv = DV[v];
                            sat |= dm & ((l & 1u) ? ~dv : dv);
                        }
                        L[i] = l;
                        FR[i] = ~dm;
                        two |= one & ~dm;
                        one |= ~dm;
                    }
                }
            }
        }
        const u64 open = act & ~sat;
        for (u64 r = open & ~one; r; r &= r - 1ull)
            atomicMin(&a.rec[slab * PROBE_SLAB + (uint32_t)__ffsll(r) - 1u].conflict, (u64)c);
        const u64 unit = open & one & ~two;
        if (unit) {
#pragma unroll
            for (uint32_t i = 0; i < PROBE_REG_WIDTH; ++i) {
                const u64 u = unit & FR[i];
                if (u) atomicOr(((L[i] & 1u) ? F0 : F1) + (L[i] >> 1), u);
            }
        }
        return;
    }
    // wider clauses: the same judgement, the earlier literals and the delta words re-read
    for (uint64_t j = j0; j < j1 && (act & ~sat); ++j) {
        const uint32_t l = a.lits[j] & PROBE_LIT_MASK, v = l >> 1;
        if (base_bit(a.PM, v)) {
            if (base_bit(a.PV, v) != (l & 1u)) sat = ~0ull;
            continue;
        }
        bool dup = false;
        for (uint64_t q = j0; q < j && !dup; ++q) dup = (a.lits[q] & PROBE_LIT_MASK) == l;
        if (dup) continue;
        const u64 dm = DM[v];
        if (dm) {
            const u64 dv = DV[v];
            sat |= dm & ((l & 1u) ? ~dv : dv);
        }
        two |= one & ~dm;
        one |= ~dm;
    }
    const u64 open = act & ~sat;
    for (u64 r = open & ~one; r; r &= r - 1ull)
        atomicMin(&a.rec[slab * PROBE_SLAB + (uint32_t)__ffsll(r) - 1u].conflict, (u64)c);
    const u64 unit = open & one & ~two;
    if (!unit) return;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint32_t l = a.lits[j] & PROBE_LIT_MASK, v = l >> 1;
        if (base_bit(a.PM, v)) continue;
        bool dup = false;
        for (uint64_t q = j0; q < j && !dup; ++q) dup = (a.lits[q] & PROBE_LIT_MASK) == l;
        if (dup) continue;
        const u64 u = unit & ~DM[v];
        if (u) atomicOr(((l & 1u) ? F0 : F1) + v, u);
    }
}

__global__ __launch_bounds__(64) void k_probe_judge(const ProbeArgs a) {
    const uint32_t slab = blockIdx.x, lane = threadIdx.x;
    const ProbeRec& r = a.rec[slab * PROBE_SLAB + lane];
    const bool ok = ((a.act[slab] >> lane) & 1ull) && r.conflict == PROP_NO_CONFLICT;
    // (a probe at its cap applies nothing; whether a unit exists is still counted: fixpoint before cap)
    const bool capped = a.max_rounds && r.rounds >= a.max_rounds;
    const u64 cnt = __ballot(ok), app = __ballot(ok && !capped);
    if (lane == 0) {
        a.cnt[slab] = cnt;
        a.app[slab] = app;
        if (slab == 0) *a.any_active = 0;
    }
}

template <class A>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_apply(const A a) {
    uint32_t slab = blockIdx.y;  // (a group: the layer here, the variable's slot below)
    const uint32_t layer = blockIdx.y;
    const uint32_t v = blockIdx.x * PROBE_THREADS + threadIdx.x;
    u64 cnt = 0;
    if constexpr (IS_GROUP<A>) {
        // the variable's item: items start at word boundaries, so the two words of a wave can belong to
        // two items -- cnt, app and the records are the half-wave's (no lane leaves before the ballots)
        slab = v < a.n_vars ? group_slot(a, a.word_item[v >> 5], layer) : ~0u;
        if (slab != ~0u) cnt = a.cnt[slab];
    } else {
        cnt = a.cnt[slab];
        if (!cnt) return;  // (the slab has ended, or every running probe is in conflict: F1 / F0 are not read again)
    }
    u64 nw = 0;
    if (v < a.n_vars && (!IS_GROUP<A> || cnt)) {
        const size_t at = (size_t)layer * a.nv_pad + v;
        const u64 f1 = a.F1[at], f0 = a.F0[at];
        if (f1 | f0) {
            a.F1[at] = 0;
            a.F0[at] = 0;
            if (!base_bit(a.PM, v)) {
                const u64 dm = a.DM[at];
                nw = (f1 | f0) & ~dm & cnt;
                const u64 ap = nw & a.app[slab];
                if (ap) {
                    a.DM[at] = dm | ap;
                    a.DV[at] = a.DV[at] | (ap & f1);  // (forced both ways: pinned to 1)
                }
            }
        }
    }
    // the probes' forced counts: the transpose of the wave's 64 words
    // (an atomic per set bit instead was measured no faster: DESIGN.md §4.13)
    ProbeRec* rec = a.rec + (size_t)slab * PROBE_SLAB;  // (a group: the lane's own slot's)
    if (!__any(nw != 0)) return;
    u64 all = nw;
    for (int d = 32; d > 0; d >>= 1) all |= __shfl_xor(all, d);
    for (u64 r = all; r; r &= r - 1ull) {  // (wave-uniform)
        const uint32_t p = (uint32_t)__ffsll(r) - 1u;
        const u64 b = __ballot((nw >> p) & 1ull);
        if constexpr (IS_GROUP<A>) {
            // split at the word border: lanes 0 and 32 count their own half for their own item's probe p
            // (a half with a new variable has a slot, and its first lane holds the half's lowest variable)
            if ((threadIdx.x & 31u) == 0) {
                const uint32_t n = (uint32_t)__popc((uint32_t)(b >> (threadIdx.x & 32u)));
                if (n) atomicAdd(&rec[p].forced, n);
            }
        } else {
            const uint32_t n = (uint32_t)__popcll(b);
            if ((threadIdx.x & 63u) == 0) atomicAdd(&rec[p].forced, n);
        }
    }
}

__global__ __launch_bounds__(64) void k_probe_settle(const ProbeArgs a) {
    const uint32_t slab = blockIdx.x, lane = threadIdx.x;
    ProbeRec& r = a.rec[slab * PROBE_SLAB + lane];
    bool run = (a.act[slab] >> lane) & 1ull;
    if (run) {
        if (r.conflict != PROP_NO_CONFLICT) {
            r.status = ALLL_PROP_CONFLICT;
            run = false;
        } else if (r.forced == 0) {  // (a unit always forces a free variable: no unit = nothing new)
            r.status = ALLL_PROP_FIXPOINT;
            run = false;
        } else if (a.max_rounds && r.rounds >= a.max_rounds) {
            r.status = ALLL_PROP_ROUND_CAP;
            run = false;
        } else {
            r.rounds += 1;
            r.n_forced += r.forced;
        }
        r.forced = 0;
    }
    const u64 act = __ballot(run);
    if (lane == 0) {
        a.act[slab] = act;
        if (act) atomicOr(a.any_active, 1u);
    }
}

template <class A>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_rows(const A a) {
    const uint32_t slab = blockIdx.y, lane = threadIdx.x & 63u;  // (a group: the layer)
    const uint32_t v = blockIdx.x * PROBE_THREADS + threadIdx.x;
    u64 dm = 0, dv = 0;
    if (v < a.n_vars) {
        const size_t at = (size_t)slab * a.nv_pad + v;
        dm = a.DM[at];
        dv = a.DV[at];
    }
    // lane p keeps the 64 variables of probe p < np: the 64 x 64 bit transpose of the wave's delta words
    auto transpose = [&](uint32_t np, u64& row_m, u64& row_v) {
        for (uint32_t p = 0; p < np; ++p) {
            const u64 bm = __ballot((dm >> p) & 1ull), bv = __ballot((dv >> p) & 1ull);
            if (lane == p) {
                row_m = bm;
                row_v = bv;
            }
        }
    };
    if constexpr (IS_GROUP<A>) {
        // the two words of the wave can belong to two items, with their own probe counts, row widths
        // and row bases (all wave-uniform): per word the probes whose rows hold it, where row 0 of them
        // starts, the row's width and the word's place in it
        const uint32_t w0 = (v - lane) >> 5;  // (the wave's first variable is a multiple of 64)
        uint32_t np_h[2] = {0u, 0u}, width[2] = {0u, 0u}, at_w[2] = {0u, 0u};
        size_t row0[2] = {0, 0};
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t w = w0 + h;
            if (w >= a.n_words) break;
            const uint32_t item = a.word_item[w], slot = group_slot(a, item, slab);
            if (slot == ~0u) continue;
            const GroupProbeItem it = a.items[item];
            const uint32_t left = it.n_probes - (a.layer0 + slab) * PROBE_SLAB;
            np_h[h] = left < PROBE_SLAB ? left : PROBE_SLAB;
            width[h] = it.n_words;
            at_w[h] = w - it.word_base;
            row0[h] = (size_t)a.slot_row[slot];
        }
        u64 row_m = 0, row_v = 0;
        transpose(np_h[0] > np_h[1] ? np_h[0] : np_h[1], row_m, row_v);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            if (lane >= np_h[h]) continue;  // (padding variables past the item's n_vars stay 0: no clause holds them)
            const size_t at = row0[h] + (size_t)lane * width[h] + at_w[h];
            a.pm_rows[at] = (uint32_t)(row_m >> (32u * h)) | a.PM[w0 + h];
            a.pv_rows[at] = (uint32_t)(row_v >> (32u * h)) | a.PV[w0 + h];
        }
    } else {
        const uint32_t p0 = slab * PROBE_SLAB;
        const uint32_t np = a.n_probes - p0 < PROBE_SLAB ? a.n_probes - p0 : PROBE_SLAB;
        u64 row_m = 0, row_v = 0;
        transpose(np, row_m, row_v);
        if (lane >= np) return;
        const uint32_t w0 = (v - lane) >> 5;  // (the wave's first variable is a multiple of 64)
        const size_t row = (size_t)(p0 + lane) * a.n_words;
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t w = w0 + h;
            if (w >= a.n_words) break;
            a.pm_rows[row + w] = (uint32_t)(row_m >> (32u * h)) | a.PM[w];
            a.pv_rows[row + w] = (uint32_t)(row_v >> (32u * h)) | a.PV[w];
        }
    }
}

uint32_t env_u32(const char* name) {
    const char* e = getenv(name);
    const long x = e ? atol(e) : 0;
    return x > 0 ? (uint32_t)std::min<long>(x, PROBE_MAX_CHUNK) : 0u;
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

uint32_t probe_forced_chunk() { return env_u32("ALLL_PROBE_SLABS"); }

int probe_drive(const PropArgs& p, const uint32_t* probes, uint64_t n_probes, uint64_t max_rounds,
                alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, hipStream_t s) {
    if (n_probes == 0) return ALLL_OK;
    const uint32_t nw = p.n_words, nv = p.n_vars;
    const uint32_t nv_pad = (nv + 63u) & ~63u;
    const bool rows = pm_rows || pv_rows;
    const uint64_t total_slabs = (n_probes + PROBE_SLAB - 1) / PROBE_SLAB;
    // the chunk: slabs whose scratch fits the byte budget (4 x 8 bytes per variable and slab, the
    // records and, when asked for, 2 x 64 rows of n_words words), or what ALLL_PROBE_SLABS says -- a
    // forced value is not held against the budget (at most PROBE_MAX_CHUNK; too large: ALLL_ERR_OOM)
    const size_t delta_bytes = 32ull * nv_pad;
    const size_t row_bytes = rows ? 2ull * PROBE_SLAB * nw * 4 : 0;
    const size_t per_slab = delta_bytes + row_bytes + PROBE_SLAB * (sizeof(ProbeRec) + 4) + 3 * 8;
    uint64_t chunk = env_u32("ALLL_PROBE_SLABS");
    if (!chunk) chunk = std::max<uint64_t>(1, std::min<uint64_t>(PROBE_BUDGET_BYTES / per_slab, PROBE_MAX_CHUNK));
    chunk = std::min(chunk, total_slabs);
    const size_t n_rec = (size_t)chunk * PROBE_SLAB;
    // one allocation: the 64-bit arrays first, then the 32-bit ones
    const size_t o_rec = delta_bytes * chunk;
    const size_t o_mask = o_rec + up16(sizeof(ProbeRec) * n_rec);
    const size_t o_any = o_mask + 3 * 8 * chunk;
    const size_t o_probes = up16(o_any + 4);
    const size_t o_bits = o_probes + 4 * n_rec;
    const size_t o_rows = up16(o_bits + 16ull * nw);
    const size_t bytes = o_rows + row_bytes * chunk + 16;
    char* base = nullptr;
    if (hipMalloc((void**)&base, bytes) != hipSuccess) return fail(ALLL_ERR_OOM, "probe: hipMalloc(%zu bytes) failed", bytes);
    ProbeArgs a{};
    a.lits = p.lits;
    a.offs = p.offs;
    a.m = p.m;
    a.k = p.k;
    a.n_vars = nv;
    a.n_words = nw;
    a.nv_pad = nv_pad;
    // (a probe applies at most n_vars rounds: a larger cap is none)
    a.max_rounds = (max_rounds && max_rounds <= nv) ? (uint32_t)max_rounds : 0u;
    a.DM = reinterpret_cast<u64*>(base);
    a.DV = a.DM + (size_t)chunk * nv_pad;
    a.F1 = a.DV + (size_t)chunk * nv_pad;
    a.F0 = a.F1 + (size_t)chunk * nv_pad;
    a.rec = reinterpret_cast<ProbeRec*>(base + o_rec);
    a.act = reinterpret_cast<u64*>(base + o_mask);
    a.cnt = a.act + chunk;
    a.app = a.cnt + chunk;
    a.any_active = reinterpret_cast<uint32_t*>(base + o_any);
    uint32_t* d_probes = reinterpret_cast<uint32_t*>(base + o_probes);
    a.probes = d_probes;
    uint32_t* bits = reinterpret_cast<uint32_t*>(base + o_bits);  // PM, PV, F1, F0 of k_prop_pack
    a.PM = bits;
    a.PV = bits + nw;
    a.pm_rows = reinterpret_cast<uint32_t*>(base + o_rows);
    a.pv_rows = a.pm_rows + (size_t)chunk * PROBE_SLAB * nw;
    PropArgs pk = p;
    pk.PM = bits;
    pk.PV = bits + nw;
    pk.F1 = bits + 2ull * nw;
    pk.F0 = bits + 3ull * nw;
    std::vector<ProbeRec> rec(n_rec);
    auto run = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));
        if (p.thr) HIP_TRY(launch_prop_pack(pk, s));
        else if (nw) HIP_TRY(hipMemsetAsync(bits, 0, 8ull * nw, s));  // every variable free
        // every applying round pins at least one more variable of every probe it keeps running
        const uint64_t bound = a.max_rounds ? a.max_rounds : (uint64_t)nv + 1;
        for (uint64_t first = 0; first < n_probes; first += chunk * PROBE_SLAB) {
            const uint32_t np = (uint32_t)std::min<uint64_t>(chunk * PROBE_SLAB, n_probes - first);
            const uint32_t ns = (np + PROBE_SLAB - 1) / PROBE_SLAB;
            a.n_probes = np;
            a.n_slabs = ns;
            HIP_TRY(hipMemcpyAsync(d_probes, probes + first, 4ull * np, hipMemcpyHostToDevice, s));
            if (nv_pad) HIP_TRY(hipMemsetAsync(base, 0, delta_bytes * chunk, s));
            hipLaunchKernelGGL(k_probe_seed<ProbeArgs>, dim3(ns), dim3(64), 0, s, a);
            HIP_TRY(hipGetLastError());
            const dim3 g_scan((uint32_t)((a.m + PROBE_THREADS - 1) / PROBE_THREADS), ns);
            const dim3 g_var((nv_pad + PROBE_THREADS - 1) / PROBE_THREADS, ns);
            bool ended = false;
            for (uint64_t round = 0; round <= bound && !ended; ++round) {
                if (a.m) hipLaunchKernelGGL(k_probe_scan<ProbeArgs>, g_scan, dim3(PROBE_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_probe_judge, dim3(ns), dim3(64), 0, s, a);
                if (nv) hipLaunchKernelGGL(k_probe_apply<ProbeArgs>, g_var, dim3(PROBE_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_probe_settle, dim3(ns), dim3(64), 0, s, a);
                HIP_TRY(hipGetLastError());
                uint32_t any = 0;
                HIP_TRY(hipMemcpyAsync(&any, a.any_active, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                ended = any == 0;
            }
            if (!ended) return fail(ALLL_ERR_HIP, "probe: the rounds did not end within their bound");
            if (rows && nw) {
                hipLaunchKernelGGL(k_probe_rows<ProbeArgs>, g_var, dim3(PROBE_THREADS), 0, s, a);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(rec.data(), a.rec, sizeof(ProbeRec) * (size_t)ns * PROBE_SLAB, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < np; ++i) {
                const ProbeRec& r = rec[i];
                results[first + i] = alll_propagate_result{r.status == ALLL_PROP_CONFLICT ? r.conflict : a.m, r.n_forced,
                                                           r.rounds, r.status};
            }
            if (pm_rows && nw)
                HIP_TRY(hipMemcpyAsync(pm_rows + first * nw, a.pm_rows, 4ull * np * nw, hipMemcpyDeviceToHost, s));
            if (pv_rows && nw)
                HIP_TRY(hipMemcpyAsync(pv_rows + first * nw, a.pv_rows, 4ull * np * nw, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return ALLL_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(base);
    return rc;
}

// The group form (alll_group_probe.h plans it): per chunk of layers the same launches over the union, the
// seed, judge and settle kernels a workgroup per slot, the scan, apply and rows kernels a layer per
// grid row.  One allocation sized for the largest chunk, freed before the return.
int group_probe_drive(const PropArgs& p, const GroupProbePlan& plan, const GroupItem* items, const uint32_t* probes,
                      uint64_t max_rounds, alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows,
                      hipStream_t s) {
    if (plan.n_probes == 0) return ALLL_OK;
    const uint32_t nw = p.n_words, nv = p.n_vars, nv_pad = plan.nv_pad, n_items = (uint32_t)plan.items.size();
    const bool rows = pm_rows && pv_rows;
    uint32_t max_layers = 0, max_slots = 0;
    uint64_t max_rows = 0;
    for (const GroupProbeChunk& c : plan.chunks) {
        max_layers = std::max(max_layers, c.n_layers);
        max_slots = std::max(max_slots, c.n_slots);
        max_rows = std::max(max_rows, c.row_words);
    }
    const size_t delta_bytes = 32ull * nv_pad;
    const size_t n_rec = (size_t)max_slots * PROBE_SLAB;
    // one allocation: the 64-bit arrays first, then the 32-bit ones
    const size_t o_rec = delta_bytes * max_layers;
    const size_t o_mask = o_rec + up16(sizeof(ProbeRec) * n_rec);
    const size_t o_srow = o_mask + 3 * 8 * (size_t)max_slots;
    const size_t o_any = o_srow + 8 * ((size_t)max_slots + 1);
    const size_t o_probes = up16(o_any + 4);
    const size_t o_items = up16(o_probes + 4 * (size_t)plan.n_probes);
    const size_t o_sbase = o_items + sizeof(GroupProbeItem) * n_items;
    const size_t o_sitem = up16(o_sbase + 4 * ((size_t)n_items + 1));
    const size_t o_bits = up16(o_sitem + 4 * (size_t)max_slots);
    const size_t o_rows = up16(o_bits + 16ull * nw);
    const size_t bytes = o_rows + 8 * (size_t)max_rows + 16;
    char* base = nullptr;
    if (hipMalloc((void**)&base, bytes) != hipSuccess)
        return fail(ALLL_ERR_OOM, "group probe: hipMalloc(%zu bytes) failed", bytes);
    GroupProbeArgs a{};
    a.lits = p.lits;
    a.offs = p.offs;
    a.m = p.m;
    a.k = p.k;
    a.n_vars = nv;
    a.n_words = nw;
    a.nv_pad = nv_pad;
    // (a probe of an item applies fewer rounds than the item has variables: a larger cap is none)
    a.max_rounds = (max_rounds && max_rounds <= plan.max_item_vars) ? (uint32_t)max_rounds : 0u;
    a.DM = reinterpret_cast<u64*>(base);
    a.DV = a.DM + (size_t)max_layers * nv_pad;
    a.F1 = a.DV + (size_t)max_layers * nv_pad;
    a.F0 = a.F1 + (size_t)max_layers * nv_pad;
    a.rec = reinterpret_cast<ProbeRec*>(base + o_rec);
    a.act = reinterpret_cast<u64*>(base + o_mask);
    a.cnt = a.act + max_slots;
    a.app = a.cnt + max_slots;
    u64* d_srow = reinterpret_cast<u64*>(base + o_srow);
    a.slot_row = d_srow;
    a.any_active = reinterpret_cast<uint32_t*>(base + o_any);
    uint32_t* d_probes = reinterpret_cast<uint32_t*>(base + o_probes);
    a.probes = d_probes;
    GroupProbeItem* d_items = reinterpret_cast<GroupProbeItem*>(base + o_items);
    a.items = d_items;
    uint32_t* d_sbase = reinterpret_cast<uint32_t*>(base + o_sbase);
    a.slot_base = d_sbase;
    uint32_t* d_sitem = reinterpret_cast<uint32_t*>(base + o_sitem);
    a.slot_item = d_sitem;
    uint32_t* bits = reinterpret_cast<uint32_t*>(base + o_bits);  // PM, PV, F1, F0 of k_prop_pack
    a.PM = bits;
    a.PV = bits + nw;
    a.pm_rows = reinterpret_cast<uint32_t*>(base + o_rows);
    a.pv_rows = a.pm_rows + max_rows;
    a.word_item = p.word_item;
    a.clause_base = p.clause_base;
    a.n_items = n_items;
    a.n_probes = (uint32_t)plan.n_probes;
    PropArgs pk = p;
    pk.PM = bits;
    pk.PV = bits + nw;
    pk.F1 = bits + 2ull * nw;
    pk.F0 = bits + 3ull * nw;
    std::vector<ProbeRec> rec(n_rec);
    std::vector<uint32_t> slot_base, slot_item, h_pm(rows ? max_rows : 0), h_pv(rows ? max_rows : 0);
    std::vector<uint64_t> slot_row;
    auto run = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));
        if (p.thr) HIP_TRY(launch_prop_pack(pk, s));  // (the items without thresholds: no pins)
        else if (nw) HIP_TRY(hipMemsetAsync(bits, 0, 8ull * nw, s));
        HIP_TRY(hipMemcpyAsync(d_probes, probes, 4ull * plan.n_probes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_items, plan.items.data(), sizeof(GroupProbeItem) * n_items, hipMemcpyHostToDevice, s));
        // every applying round pins at least one more variable of every probe it keeps running
        const uint64_t bound = a.max_rounds ? a.max_rounds : (uint64_t)plan.max_item_vars + 1;
        for (const GroupProbeChunk& c : plan.chunks) {
            const uint32_t nl = c.n_layers, ns = c.n_slots;
            group_probe_chunk_slots(plan, c, rows, slot_base, slot_item, slot_row);
            a.n_slabs = ns;
            a.layer0 = c.layer0;
            HIP_TRY(hipMemcpyAsync(d_sbase, slot_base.data(), 4ull * slot_base.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_sitem, slot_item.data(), 4ull * ns, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_srow, slot_row.data(), 8ull * slot_row.size(), hipMemcpyHostToDevice, s));
            // (all four tables, at the largest chunk's strides)
            if (nv_pad) HIP_TRY(hipMemsetAsync(base, 0, delta_bytes * max_layers, s));
            const ProbeArgs& slots = a;  // (judge and settle: a workgroup per slot, the context's kernels)
            hipLaunchKernelGGL(k_probe_seed<GroupProbeArgs>, dim3(ns), dim3(64), 0, s, a);
            HIP_TRY(hipGetLastError());
            const dim3 g_scan((uint32_t)((a.m + PROBE_THREADS - 1) / PROBE_THREADS), nl);
            const dim3 g_var((nv_pad + PROBE_THREADS - 1) / PROBE_THREADS, nl);
            bool ended = false;
            for (uint64_t round = 0; round <= bound && !ended; ++round) {
                if (a.m) hipLaunchKernelGGL(k_probe_scan<GroupProbeArgs>, g_scan, dim3(PROBE_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_probe_judge, dim3(ns), dim3(64), 0, s, slots);
                if (nv) hipLaunchKernelGGL(k_probe_apply<GroupProbeArgs>, g_var, dim3(PROBE_THREADS), 0, s, a);
                hipLaunchKernelGGL(k_probe_settle, dim3(ns), dim3(64), 0, s, slots);
                HIP_TRY(hipGetLastError());
                uint32_t any = 0;
                HIP_TRY(hipMemcpyAsync(&any, a.any_active, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                ended = any == 0;
            }
            if (!ended) return fail(ALLL_ERR_HIP, "group probe: the rounds did not end within their bound");
            if (rows && c.row_words) {
                hipLaunchKernelGGL(k_probe_rows<GroupProbeArgs>, g_var, dim3(PROBE_THREADS), 0, s, a);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(h_pm.data(), a.pm_rows, 4ull * c.row_words, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(h_pv.data(), a.pv_rows, 4ull * c.row_words, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipMemcpyAsync(rec.data(), a.rec, sizeof(ProbeRec) * (size_t)ns * PROBE_SLAB, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t slot = 0; slot < ns; ++slot) {
                const uint32_t i = slot_item[slot], layer = c.layer0 + (slot - slot_base[i]);
                const GroupProbeItem& it = plan.items[i];
                const uint32_t first = layer * PROBE_SLAB, np = std::min(PROBE_SLAB, it.n_probes - first);
                for (uint32_t q = 0; q < np; ++q) {
                    const ProbeRec& r = rec[(size_t)slot * PROBE_SLAB + q];
                    // the item's own clause index
                    results[(size_t)it.probe_base + first + q] = alll_propagate_result{
                        r.status == ALLL_PROP_CONFLICT ? r.conflict - items[i].clause_base : items[i].n_clauses, r.n_forced,
                        r.rounds, r.status};
                }
                if (rows && it.n_words) {
                    const size_t to = plan.row_base[i] + (size_t)first * it.n_words, n = 4ull * np * it.n_words;
                    memcpy(pm_rows + to, h_pm.data() + slot_row[slot], n);
                    memcpy(pv_rows + to, h_pv.data() + slot_row[slot], n);
                }
            }
        }
        return ALLL_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(s);
    (void)hipFree(base);
    return rc;
}

}  // namespace alll
