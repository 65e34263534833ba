// alll_small.hip -- the LDS-resident batch kernel (gfx950, wave64).
//
// One workgroup owns one item of the batch for one slice of at most `slice` iterations: it loads
// the item's clauses (16-bit literals and offsets), assignment and loop state into LDS, runs
//   eval      clause evaluation (Clause.h:34-46), a ballot per 64 clauses
//   compact   ordered compaction of the violated clauses (prefix over the ballots, mbcnt ranks:
//             ascending clause order, SATInstance.h:264-280) and the end check
//   LFMIS     exact lexicographically-first MIS in clause order by LDS claims per variable
//             (populate_mis_parallel with one set, SATInstance.h:391-451)
//   resample  Philox4x32-10 of every variable of every MIS clause (SATInstance.h:340-365), by
//             LDS atomics on the assignment words, as the clause joins the MIS
// with workgroup barriers only, and writes the assignment and the state back.  No global atomic,
// no spin-wait, no grid barrier: every loop is bounded (the slice; LFMIS rounds <= violated
// clauses), and the host relaunches until every item is done.  Integer / bit work only.
// Two instantiations of one body: k_small for a batch without per-variable thresholds, k_small_biased
// for a batch in which at least one item has some.
#include "alll_small.h"
#include "alll_draws.h"

namespace alll {

namespace {

// LFMIS claim key of clause c in round r: later rounds hold smaller keys, so a round's claims beat
// what earlier rounds left behind and the claim words need no reset between rounds; 0 (below
// every key: r <= 8192) marks a variable covered by an MIS clause.
constexpr uint32_t SM_ID_BITS = 13;
constexpr uint32_t SM_EPOCH0 = 8193;
constexpr uint32_t SM_JOINED = 0x8000u;  // list entry flag: the clause joined the MIS this round
static_assert(ALLL_BATCH_MAX_CLAUSES <= (1u << SM_ID_BITS), "clause ids fit the claim key");
static_assert(ALLL_BATCH_MAX_CLAUSES < SM_EPOCH0, "a round's epoch never reaches 0");
static_assert(ALLL_BATCH_MAX_VARS <= 8192 && ALLL_BATCH_MAX_LITERALS <= 65535, "16-bit literals and offsets");

__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {  // set bits below the own lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Per-variable thresholds of a biased batch: the item's own, LDS-resident (lds)
// when the batch's layout with them fits, else read from the pool in global memory (glb); `on` is
// the item's flag (SmallItem::pad), uniform over the workgroup.
struct SmallThr {
    const uint32_t* lds;
    const uint32_t* __restrict__ glb;
    bool on, in_lds;
};

// clause [j0, j1) joins the MIS: its variables are covered (claim word 0) and resampled in round
// {it_lo, it_hi} (the loop holds the round as the two words: k_small's machine code depends on it).
// BIASED and an item with thresholds: every variable takes its own biased draw (alll_draws.h); a
// variable that occurs twice is drawn twice to the same value.
template <bool BIASED>
__device__ __forceinline__ void small_join(uint32_t* s_claim, uint32_t* s_A, uint32_t* s_ctl, const uint16_t* s_lits,
                                           uint32_t j0, uint32_t j1, uint32_t it_lo, uint32_t it_hi, uint32_t k0,
                                           uint32_t k1, const SmallThr& T) {
    const uint64_t it = (uint64_t)it_hi << 32 | it_lo;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t v = s_lits[j] >> 1, bit = 1u << (v & 31u);
        s_claim[v] = 0;
        bool one;
        if (BIASED && T.on) {
            const uint32_t x = biased_resample_var(k0, k1, it, v);
            one = biased_bit(x, T.in_lds ? T.lds[v] : T.glb[v]);
        } else {
            one = (resample_word(k0, k1, it, v >> 5) & bit) != 0;
        }
        if (one) atomicOr(&s_A[v >> 5], bit);
        else atomicAnd(&s_A[v >> 5], ~bit);
    }
    atomicAdd(&s_ctl[2], 1u);
    atomicAdd(&s_ctl[3], j1 - j0);
}

// The kernel's body.  BIASED = false is the kernel of a batch without thresholds (g_thr and thr_lds
// unused); BIASED = true serves a batch with at least one biased item: thr_lds is the byte offset of
// the LDS thresholds, 0 when the batch reads them from g_thr (item i's at 32 * a_at, zero-padded).
// TRACK (best-assignment tracking): a pass that finds strictly fewer violated clauses
// than every pass before it copies the assignment it evaluated (s_A, untouched since the eval) to the
// item's words of g_best, before the solved and the capped break; the record's two numbers travel in
// SmallState from launch to launch.  The LDS layout is the untracked one.
template <bool BIASED, bool TRACK = false>
__device__ __forceinline__ void small_body(const SmallItem* __restrict__ items, SmallState* __restrict__ states,
                                                const uint16_t* __restrict__ g_lits,
                                                const uint16_t* __restrict__ g_offs, uint32_t* __restrict__ g_A,
                                                const SmallLds& L, const uint32_t slice,
                                                const uint32_t serial_max, const uint32_t* __restrict__ g_thr,
                                                const uint32_t thr_lds, uint32_t* __restrict__ g_best = nullptr) {
    extern __shared__ __align__(16) unsigned char smem[];
    const SmallItem it = items[blockIdx.x];
    SmallState st = states[blockIdx.x];
    if (st.done != 0 || st.n_iter >= st.limit_eval) return;  // finished, or nothing asked of it

    uint16_t* const s_lits = (uint16_t*)(smem + L.lits);
    uint16_t* const s_offs = (uint16_t*)(smem + L.offs);
    unsigned long long* const s_vmask = (unsigned long long*)(smem + L.vmask);
    uint32_t* const s_claim = (uint32_t*)(smem + L.claim);
    uint32_t* const s_A = (uint32_t*)(smem + L.A);
    uint32_t* const s_prefix = (uint32_t*)(smem + L.prefix);
    uint32_t* const s_ctl = (uint32_t*)(smem + L.ctl);  // [0], [1] live counts of the lists; [2] |MIS|; [3] resamples
    uint16_t* const s_list = (uint16_t*)(smem + L.list);

    const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = it.m, groups = (m + 63u) / 64u;

    // ---- load: 16-byte vectors (the pools pad every problem to 8 elements)
    {
        const uint4* src = (const uint4*)(g_lits + it.lits_at);
        uint4* dst = (uint4*)s_lits;
        for (uint32_t i = tid; i < (it.n_lits + 7u) / 8u; i += nt) dst[i] = src[i];
        src = (const uint4*)(g_offs + it.offs_at);
        dst = (uint4*)s_offs;
        for (uint32_t i = tid; i < (m + 1u + 7u) / 8u; i += nt) dst[i] = src[i];
        for (uint32_t w = tid; w < it.n_words; w += nt) s_A[w] = g_A[it.a_at + w];
        if (tid < 8) s_ctl[tid] = 0;
        if (BIASED && it.pad && thr_lds) {  // (32 * n_words entries in the pool: whole 16-byte vectors)
            src = (const uint4*)(g_thr + 32ull * it.a_at);
            dst = (uint4*)(smem + thr_lds);
            for (uint32_t i = tid; i < (it.n_vars + 3u) / 4u; i += nt) dst[i] = src[i];
        }
    }
    __syncthreads();
    const SmallThr T{(const uint32_t*)(smem + thr_lds), BIASED ? g_thr + 32ull * it.a_at : nullptr,
                     BIASED && it.pad != 0, thr_lds != 0};

    const uint32_t k0 = (uint32_t)it.seed, k1 = (uint32_t)(it.seed >> 32);
    uint64_t n_iter = st.n_iter;
    uint64_t add_mis = 0, add_res = 0;  // (thread 0)
    uint32_t done = 0, u = st.n_violated, rounds_max = st.rounds_max;

    for (uint32_t s = 0; s < slice && n_iter < st.limit_eval; ++s) {
        ++n_iter;
        // ---- eval: a ballot per 64 clauses (whole waves take part; clauses past m are not violated)
        for (uint32_t v = tid; v < it.n_vars; v += nt) s_claim[v] = ~0u;
        for (uint32_t base = 0; base < m; base += nt) {
            const uint32_t c = base + tid;
            bool viol = false;
            if (c < m) {
                viol = true;
                for (uint32_t j = s_offs[c], j1 = s_offs[c + 1]; j < j1; ++j) {
                    const uint32_t l = s_lits[j], v = l >> 1;
                    if (((s_A[v >> 5] >> (v & 31u)) & 1u) != (l & 1u)) { viol = false; break; }
                }
            }
            const unsigned long long mask = __ballot(viol);
            if (lane == 0 && c < m) s_vmask[c >> 6] = mask;
        }
        __syncthreads();
        // ---- violated clauses before every ballot (wave 0), the count
        if (tid == 0) { s_ctl[0] = 0; s_ctl[1] = 0; }
        if (wave == 0) {
            uint32_t run = 0;
            for (uint32_t g0 = 0; g0 < groups; g0 += 64u) {
                const uint32_t g = g0 + lane;
                const uint32_t cnt = g < groups ? (uint32_t)__popcll(s_vmask[g]) : 0u;
                uint32_t incl = cnt;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t t = __shfl_up(incl, d);
                    if ((int)lane >= d) incl += t;
                }
                if (g < groups) s_prefix[g] = run + incl - cnt;
                run += __shfl(incl, 63);
            }
            if (lane == 0) s_prefix[groups] = run;
        }
        __syncthreads();
        u = s_prefix[groups];
        if (TRACK && u < st.best_u) {  // (uniform: every thread holds the state)
            st.best_u = u;
            st.best_iter = n_iter;
            for (uint32_t w = tid; w < it.n_words; w += nt) g_best[it.a_at + w] = s_A[w];
        }
        if (u == 0) { done = 1; break; }                     // solved (check_if_noUNSAT)
        if (n_iter >= st.limit_nores) { done = 2; break; }   // the capped pass does not resample

        // ---- ordered compaction into list 0, with the claims of LFMIS round 0
        for (uint32_t base = 0; base < m; base += nt) {
            const uint32_t c = base + tid;
            if (c >= m) continue;
            const unsigned long long mask = s_vmask[c >> 6];
            if (!((mask >> lane) & 1ull)) continue;
            s_list[s_prefix[c >> 6] + lane_rank(mask)] = (uint16_t)c;
            if (u <= serial_max) continue;  // (the serial greedy below claims nothing)
            const uint32_t key = (SM_EPOCH0 << SM_ID_BITS) | c;
            for (uint32_t j = s_offs[c], j1 = s_offs[c + 1]; j < j1; ++j) atomicMin(&s_claim[s_lits[j] >> 1], key);
        }
        __syncthreads();

        // ---- LFMIS rounds: a live clause that holds the minimum on all its variables joins (and
        // is resampled at once: MIS clauses are variable-disjoint, nothing reads the assignment
        // before the next eval); the clauses that share a variable with a joiner die; the others
        // claim again for the next round.  The lowest live clause always joins: rounds <= u.
        const uint32_t it_lo = (uint32_t)(n_iter - 1), it_hi = (uint32_t)((n_iter - 1) >> 32);
        uint32_t live = u, cur = 0, r = 0;
        if (u <= serial_max) {
            // ---- one-wave serial greedy (serial_max <= 64): lane i holds the i-th violated clause;
            // in clause order each one joins unless a variable of it is covered already.  Exact by
            // definition; a step costs an LDS round trip, so it pays only for very small sets.
            if (wave == 0) {
                const uint32_t c = lane < u ? s_list[lane] : 0u;
                const uint32_t j0 = s_offs[c], j1 = lane < u ? s_offs[c + 1] : j0;
                for (uint32_t i = 0; i < u; ++i) {
                    if (lane == i) {
                        bool open = true;
                        for (uint32_t j = j0; j < j1; ++j) open &= *(volatile uint32_t*)&s_claim[s_lits[j] >> 1] != 0u;
                        if (open) small_join<BIASED>(s_claim, s_A, s_ctl, s_lits, j0, j1, it_lo, it_hi, k0, k1, T);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // lane i's cover marks before lane i + 1 looks
                }
            }
            __syncthreads();
            live = 0;
            r = 1;
        }
        while (live != 0 && r < u) {
            uint16_t* const lc = s_list + cur * L.list_stride;
            uint16_t* const ln = s_list + (cur ^ 1u) * L.list_stride;
            const uint32_t ep = (SM_EPOCH0 - r) << SM_ID_BITS;
            for (uint32_t i = tid; i < live; i += nt) {
                const uint32_t c = lc[i], j0 = s_offs[c], j1 = s_offs[c + 1];
                bool win = true;
                for (uint32_t j = j0; j < j1; ++j) win &= s_claim[s_lits[j] >> 1] == (ep | c);
                if (!win) continue;
                small_join<BIASED>(s_claim, s_A, s_ctl, s_lits, j0, j1, it_lo, it_hi, k0, k1, T);
                lc[i] = (uint16_t)(c | SM_JOINED);
            }
            __syncthreads();
            if (tid == 0) s_ctl[cur] = 0;  // (everyone has read it; the round after next appends to it)
            const uint32_t ep_next = (SM_EPOCH0 - r - 1u) << SM_ID_BITS;
            for (uint32_t i = tid; i < live; i += nt) {
                const uint32_t c = lc[i];
                if (c & SM_JOINED) continue;
                const uint32_t j0 = s_offs[c], j1 = s_offs[c + 1];
                bool dead = false;
                for (uint32_t j = j0; j < j1; ++j) dead |= s_claim[s_lits[j] >> 1] == 0u;
                if (dead) continue;
                ln[atomicAdd(&s_ctl[cur ^ 1u], 1u)] = (uint16_t)c;
                for (uint32_t j = j0; j < j1; ++j) atomicMin(&s_claim[s_lits[j] >> 1], ep_next | c);
            }
            __syncthreads();
            cur ^= 1u;
            live = s_ctl[cur];
            ++r;
        }
        rounds_max = max(rounds_max, r);
        if (tid == 0) {
            add_mis += s_ctl[2];
            add_res += s_ctl[3];
            s_ctl[2] = 0;
            s_ctl[3] = 0;
        }
    }

    // ---- write back
    __syncthreads();
    for (uint32_t w = tid; w < it.n_words; w += nt) g_A[it.a_at + w] = s_A[w];
    if (tid == 0) {
        st.n_iter = n_iter;
        st.n_resamples += add_res;
        st.sum_mis += add_mis;
        st.n_violated = u;
        st.done = done;
        st.rounds_max = rounds_max;
        states[blockIdx.x] = st;
    }
}

__global__ void __launch_bounds__(1024) k_small(const SmallItem* __restrict__ items, SmallState* __restrict__ states,
                                                const uint16_t* __restrict__ g_lits,
                                                const uint16_t* __restrict__ g_offs, uint32_t* __restrict__ g_A,
                                                const SmallLds L, const uint32_t slice,
                                                const uint32_t serial_max) {
    small_body<false>(items, states, g_lits, g_offs, g_A, L, slice, serial_max, nullptr, 0u);
}

__global__ void __launch_bounds__(1024) k_small_biased(const SmallItem* __restrict__ items,
                                                       SmallState* __restrict__ states,
                                                       const uint16_t* __restrict__ g_lits,
                                                       const uint16_t* __restrict__ g_offs, uint32_t* __restrict__ g_A,
                                                       const SmallLds L, const uint32_t slice,
                                                       const uint32_t serial_max, const uint32_t* __restrict__ g_thr,
                                                       const uint32_t thr_lds) {
    small_body<true>(items, states, g_lits, g_offs, g_A, L, slice, serial_max, g_thr, thr_lds);
}

// ... with best-assignment tracking
__global__ void __launch_bounds__(1024) k_small_best(const SmallItem* __restrict__ items, SmallState* __restrict__ states,
                                                     const uint16_t* __restrict__ g_lits,
                                                     const uint16_t* __restrict__ g_offs, uint32_t* __restrict__ g_A,
                                                     const SmallLds L, const uint32_t slice, const uint32_t serial_max,
                                                     uint32_t* __restrict__ g_best) {
    small_body<false, true>(items, states, g_lits, g_offs, g_A, L, slice, serial_max, nullptr, 0u, g_best);
}

__global__ void __launch_bounds__(1024) k_small_biased_best(const SmallItem* __restrict__ items,
                                                            SmallState* __restrict__ states,
                                                            const uint16_t* __restrict__ g_lits,
                                                            const uint16_t* __restrict__ g_offs,
                                                            uint32_t* __restrict__ g_A, const SmallLds L,
                                                            const uint32_t slice, const uint32_t serial_max,
                                                            const uint32_t* __restrict__ g_thr, const uint32_t thr_lds,
                                                            uint32_t* __restrict__ g_best) {
    small_body<true, true>(items, states, g_lits, g_offs, g_A, L, slice, serial_max, g_thr, thr_lds, g_best);
}

__global__ void k_small_init(const SmallItem* __restrict__ items, uint32_t* __restrict__ g_A) {
    const SmallItem it = items[blockIdx.x];
    for (uint32_t w = threadIdx.x; w < it.n_words; w += blockDim.x) {
        uint32_t x = fill_word((uint32_t)it.seed, (uint32_t)(it.seed >> 32), w);
        if (w == it.n_words - 1u && (it.n_vars & 31u)) x &= (1u << (it.n_vars & 31u)) - 1u;
        g_A[it.a_at + w] = x;
    }
}

// Unit propagation of the item's pins, a workgroup per item, all rounds in one
// launch.  A round: every lane judges clauses (from the 16-bit pools) against the item's thresholds in
// the pool as the last round left them; a falsified clause lowers s_conf, a unit sets its variable's
// bit in s_F1 or s_F0 (LDS atomics: min and or do not depend on the order); after the barrier the
// round ends the item (conflict, no unit, the cap) or the lanes write the forced pins to the pool.
// Barriers only; the loop is bounded by max_rounds, or by n_vars + 1 rounds (a round that applies
// pins at least one more variable).  Items without thresholds (pad == 0) are left alone.
__global__ __launch_bounds__(256) void k_small_propagate(const SmallItem* __restrict__ items,
                                                         const uint16_t* __restrict__ g_lits,
                                                         const uint16_t* __restrict__ g_offs, uint32_t* g_thr,
                                                         const uint32_t max_rounds, SmallProp* __restrict__ out) {
    __shared__ uint32_t s_F1[ALLL_BATCH_MAX_VARS / 32], s_F0[ALLL_BATCH_MAX_VARS / 32];
    __shared__ uint32_t s_conf, s_forced;
    const SmallItem it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    if (it.pad == 0) {
        if (tid == 0) out[blockIdx.x] = SmallProp{it.m, 0u, 0u, (uint32_t)ALLL_PROP_NONE};
        return;
    }
    const uint16_t* lits = g_lits + it.lits_at;
    const uint16_t* offs = g_offs + it.offs_at;
    uint32_t* thr = g_thr + 32ull * it.a_at;
    for (uint32_t w = tid; w < it.n_words; w += nt) s_F1[w] = s_F0[w] = 0;
    if (tid == 0) {
        s_conf = it.m;
        s_forced = 0;
    }
    __syncthreads();
    const uint32_t bound = max_rounds ? max_rounds : it.n_vars + 1u;
    uint32_t rounds = 0, n_forced = 0, status = ALLL_PROP_FIXPOINT, conflict = it.m;
    for (uint32_t round = 0; round <= bound; ++round) {
        for (uint32_t c = tid; c < it.m; c += nt) {
            bool sat = false, same = true;
            uint32_t n_free = 0, unit = 0;
            for (uint32_t j = offs[c]; j < offs[c + 1]; ++j) {
                const uint32_t l = lits[j], t = thr[l >> 1];
                if (t == ((l & 1u) ? 0u : 0xFFFFFFFFu)) {  // a true literal
                    sat = true;
                    break;
                }
                if (t == ((l & 1u) ? 0xFFFFFFFFu : 0u)) continue;
                if (n_free++ == 0) unit = l;
                else same = same && l == unit;
            }
            if (sat || (n_free && !same)) continue;
            if (n_free == 0) atomicMin(&s_conf, c);
            else atomicOr(((unit & 1u) ? s_F0 : s_F1) + (unit >> 6), 1u << ((unit >> 1) & 31u));
        }
        __syncthreads();
        conflict = s_conf;
        if (conflict == it.m) {  // (uniform: every lane reads the same word)
            uint32_t cnt = 0;
            for (uint32_t w = tid; w < it.n_words; w += nt) cnt += __popc(s_F1[w] | s_F0[w]);
            for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
            if ((tid & 63u) == 0 && cnt) atomicAdd(&s_forced, cnt);
        }
        __syncthreads();
        const uint32_t forced = s_forced;
        if (conflict != it.m) {
            status = ALLL_PROP_CONFLICT;
            break;
        }
        if (forced == 0) break;  // (fixpoint)
        if (round >= bound) {
            status = ALLL_PROP_ROUND_CAP;
            break;
        }
        // apply: every unit's variable was free at the round's start (forced both ways: pinned to 1)
        for (uint32_t w = tid; w < it.n_words; w += nt) {
            const uint32_t f1 = s_F1[w], f0 = s_F0[w];
            for (uint32_t r = f1 | f0; r; r &= r - 1u) {
                const uint32_t bit = __ffs(r) - 1u;
                thr[32u * w + bit] = ((f1 >> bit) & 1u) ? 0xFFFFFFFFu : 0u;
            }
            s_F1[w] = s_F0[w] = 0;
        }
        rounds += 1;
        n_forced += forced;
        __syncthreads();  // (orders the pool's new pins before the next round's loads, within the workgroup)
        if (tid == 0) s_forced = 0;
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = SmallProp{conflict, n_forced, rounds, status};
}

__global__ void k_small_limits(SmallState* __restrict__ states, uint32_t n_items, int solve, uint64_t value) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    SmallState& st = states[i];
    if (solve) {
        st.limit_eval = value;
        st.limit_nores = value;
    } else {
        st.limit_eval = value > ~0ull - st.n_iter ? ~0ull : st.n_iter + value;
        st.limit_nores = ~0ull;
    }
    if (st.done == 2) st.done = 0;
}

}  // namespace

hipError_t small_prepare() {
    // (the attribute is the kernel's, not the batch's: the footprint of an item at the limits)
    const SmallLds top = small_lds_layout(ALLL_BATCH_MAX_VARS, ALLL_BATCH_MAX_CLAUSES, ALLL_BATCH_MAX_LITERALS);
    hipError_t e = hipFuncSetAttribute((const void*)k_small, hipFuncAttributeMaxDynamicSharedMemorySize, (int)top.bytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)k_small_best, hipFuncAttributeMaxDynamicSharedMemorySize, (int)top.bytes);
    if (e != hipSuccess) return e;
    // (with LDS thresholds a layout goes up to the budget; beyond it the batch reads them from global memory)
    e = hipFuncSetAttribute((const void*)k_small_biased_best, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SMALL_LDS_BUDGET);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)k_small_biased, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)SMALL_LDS_BUDGET);
}

hipError_t launch_small_init(const SmallBatch& b, hipStream_t s) {
    hipLaunchKernelGGL(k_small_init, dim3(b.n_items), dim3(64), 0, s, b.items, b.A);
    return hipGetLastError();
}

hipError_t launch_small_limits(const SmallBatch& b, bool solve, uint64_t value, hipStream_t s) {
    hipLaunchKernelGGL(k_small_limits, dim3((b.n_items + 255u) / 256u), dim3(256), 0, s, b.states, b.n_items,
                       solve ? 1 : 0, value);
    return hipGetLastError();
}

hipError_t launch_small_slice(const SmallBatch& b, uint32_t slice, hipStream_t s) {
    if (b.best) {  // best-assignment tracking: the same choice among the tracked instantiations
        if (b.biased) {
            const uint32_t bytes = b.thr_lds ? b.lds_thr_bytes : b.lds.bytes;
            hipLaunchKernelGGL(k_small_biased_best, dim3(b.n_items), dim3(b.threads), bytes, s, b.items, b.states,
                               b.lits, b.offs, b.A, b.lds, slice, b.serial_max, b.thr, b.thr_lds, b.best);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(k_small_best, dim3(b.n_items), dim3(b.threads), b.lds.bytes, s, b.items, b.states, b.lits,
                           b.offs, b.A, b.lds, slice, b.serial_max, b.best);
        return hipGetLastError();
    }
    if (b.biased) {  // at least one item has thresholds
        const uint32_t bytes = b.thr_lds ? b.lds_thr_bytes : b.lds.bytes;
        hipLaunchKernelGGL(k_small_biased, dim3(b.n_items), dim3(b.threads), bytes, s, b.items, b.states, b.lits,
                           b.offs, b.A, b.lds, slice, b.serial_max, b.thr, b.thr_lds);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_small, dim3(b.n_items), dim3(b.threads), b.lds.bytes, s, b.items, b.states, b.lits, b.offs,
                       b.A, b.lds, slice, b.serial_max);
    return hipGetLastError();
}

hipError_t launch_small_propagate(const SmallBatch& b, uint32_t* thr, uint32_t max_rounds, SmallProp* out,
                                  hipStream_t s) {
    hipLaunchKernelGGL(k_small_propagate, dim3(b.n_items), dim3(256), 0, s, b.items, b.lits, b.offs, thr, max_rounds, out);
    return hipGetLastError();
}

}  // namespace alll
