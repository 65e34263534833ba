// alll_group_dev.h -- device side of the block-diagonal groups: what the group's
// kernels (alll_kernels.hip, k_group_*), the one-instance runtime (alll_runtime.cpp, which launches
// them inside the captured iteration of a context that has a group attached) and the group's own
// runtime (alll_group_runtime.cpp) share.  Not part of the public ABI.
#pragma once
#include "alll_group.h"
#include "alll_internal.h"

namespace alll {

// Statistics of one item, kept on the device by the finishing block of k_group_resample.
struct GroupItemState {
    uint64_t end_iter;     // eval pass at which the item had no violated clause (counted); 0: unfinished
    uint64_t sum_mis;      // sum |MIS| of the item's clauses
    uint64_t n_resamples;  // sum of clause lengths over the item's MIS clauses
    uint64_t n_violated;   // the item's violated clauses at its last eval pass
};

struct GroupCtl {
    uint64_t acc_iter;     // eval pass (DevState::n_iter) whose counts the item states hold
    uint64_t pad;
};

constexpr uint32_t GROUP_SCRATCH = 3;  // per item and pass: violated clauses, MIS clauses, MIS literals

struct GroupDev {
    const GroupWord* words;       // per assignment word of the union
    const uint32_t* clause_base;  // n_items + 1 ascending clause bases (item of a clause: binary search)
    const uint32_t* perm;         // evaluation position -> clause id (nullptr: clause order)
    unsigned long long* scratch;  // n_items x GROUP_SCRATCH counts of the current pass (zero between passes)
    GroupItemState* items;
    GroupCtl* ctl;
    uint32_t n_items;
    uint32_t pad;
};

// Best-assignment tracking of a group: passed to the tracked kernels only, so the
// kernels of a group that does not track keep their arguments.  The words of the records are
// LoopBuffers::A_best (the union's, an item's at its word base).
struct GroupBest {
    unsigned long long* rec;    // per item {fewest violated clauses of a pass (~0: none yet), that pass}
    uint32_t* improved;         // per item: the current pass is its record (k_group_best)
    const uint32_t* word_item;  // per assignment word of the union: its item
};

// Launchers (alll_kernels.hip).  All asynchronous on `s`.
hipError_t launch_group_init(const LoopBuffers& b, const GroupDev& g, hipStream_t s);
// after the LFMIS tail: the pass's violated clauses and MIS clauses counted per item
hipError_t launch_group_account(const ClauseView& cv, const LoopBuffers& b, const GroupDev& g, hipStream_t s);
// the keyed resample (in place of k_resample_vars) and, in one more workgroup, the items' states;
// wbias (with b.thr): a bit per assignment word, set for the words of the items
// that have thresholds -- k_group_resample_biased; nullptr: k_group_resample.  gb (with b.A_best):
// k_group_best, then the tracked forms of the two
hipError_t launch_group_resample(const LoopBuffers& b, const GroupDev& g, const uint32_t* wbias, const GroupBest* gb,
                                 hipStream_t s);

}  // namespace alll

// ---- the one-instance context as the group's runtime drives it (alll_runtime.cpp)
struct alll_ctx;
namespace alll {

struct CtxAccess {
    int device;
    hipStream_t stream;
    const LoopBuffers* b;
    const ClauseView* cv;
    const DevState* h_state;   // pinned mirror, fresh after ctx_read_state
    const uint32_t* perm;      // host copy: evaluation position -> clause id (n_perm entries; 0: clause order)
    uint64_t n_perm;
};
CtxAccess ctx_access(alll_ctx* c);
// from now on every iteration the context enqueues (or captures) ends with the group's accounting
// and keyed resample instead of k_resample_vars; call before the first iteration
void ctx_attach_group(alll_ctx* c, const GroupDev* g);
int ctx_read_state(alll_ctx* c);  // also reports a loop that stopped on an error
int ctx_write_limits(alll_ctx* c, uint64_t limit_eval, uint64_t limit_nores);  // after ctx_read_state
int ctx_launch_iterations(alll_ctx* c, uint64_t n);
void ctx_assignment_changed(alll_ctx* c);  // the next pass's violated count is unknown
// per-variable probabilities of a group: that the context's options allow them
// (else ALLL_ERR_UNSUPPORTED, before any device work), then the union's thresholds and the per-word
// bits (both null: none) for every iteration enqueued or captured from now on -- captured
// iterations hold the old pointers by value and are dropped.  Stream drained by the caller.
int ctx_bias_supported(alll_ctx* c);
void ctx_set_group_bias(alll_ctx* c, const uint32_t* thr, const uint32_t* wbias);
// best-assignment tracking of a group: the same option check under the feature's
// name, then the union's record words (the context allocates them) and the group's tables, or
// nullptr for off; captured iterations are dropped.  Stream drained by the caller, no iteration made.
int ctx_track_supported(alll_ctx* c);
int ctx_set_group_best(alll_ctx* c, const GroupBest* gb);

}  // namespace alll
