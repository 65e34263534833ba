// alll_small.h -- launchers of the LDS-resident batch kernel (alll_small.hip) for the device
// set-up (alll_batch_runtime.cpp).  All asynchronous on `s`.
#pragma once
#include <hip/hip_runtime.h>

#include "alll_batch.h"

namespace alll {

// device image of a batch (what plan_batch packed, uploaded)
struct SmallBatch {
    const SmallItem* items;
    SmallState* states;
    const uint16_t* lits;
    const uint16_t* offs;
    uint32_t* A;
    uint32_t n_items;
    uint32_t threads;   // workgroup size
    uint32_t serial_max;  // violated sets up to this size (<= 64) take the one-wave serial greedy, 0: never
    SmallLds lds;
    // per-variable thresholds (alll_batch_set_var_thresholds)
    const uint32_t* thr;     // the pool: item i's thresholds at 32 * a_at, zero-padded to its words; null until the first call
    uint32_t thr_lds;        // byte offset of the LDS-resident thresholds behind lds, 0: the kernel reads the pool
    uint32_t lds_thr_bytes;  // dynamic LDS with them
    bool biased;             // an item has thresholds: the biased instantiation is launched
    // best-assignment tracking (alll_batch_track_best): item i's record words at a_at of a
    // second assignment pool; null: off, the untracked instantiations are launched
    uint32_t* best;
};

// what k_small_propagate leaves per item
struct SmallProp {
    uint32_t conflict;  // smallest falsified clause, the item's m when there is none
    uint32_t n_forced;
    uint32_t rounds;
    uint32_t status;    // ALLL_PROP_*
};

// the dynamic LDS attribute of both instantiations of the kernel (on the batch's device, before its first slice)
hipError_t small_prepare();
// initial assignment of every item: word w = Philox(seed, {w, 0, 0xFFFFFFFF, 0}).x, tail cleared
hipError_t launch_small_init(const SmallBatch& b, hipStream_t s);
// solve = true: limit_eval = limit_nores = value (alll_solve's cap); false: limit_eval = n_iter +
// value, limit_nores = none (alll_run); a stop at limit_nores is lifted either way
hipError_t launch_small_limits(const SmallBatch& b, bool solve, uint64_t value, hipStream_t s);
// one slice: every unfinished item runs at most `slice` iterations (b.biased: the instantiation with thresholds)
hipError_t launch_small_slice(const SmallBatch& b, uint32_t slice, hipStream_t s);
// unit propagation of the pins of every item that has thresholds (pad != 0), all rounds in one launch;
// thr: the threshold pool (b.thr, written); max_rounds 0: until a fixpoint or a conflict; out: n_items
hipError_t launch_small_propagate(const SmallBatch& b, uint32_t* thr, uint32_t max_rounds, SmallProp* out, hipStream_t s);

}  // namespace alll
