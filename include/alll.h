/*
 * alll.h -- C-ABI of the MI355X-native Moser-Tardos (ALLL) resample loop.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference exposes a
 * header-only C++ API (xmif1/ALLLSatisfiabilitySolver, library/include/SATInstance.h);
 * the compatibility headers in include/alll_compat/ keep that API and call the entry
 * points below.  Every entry point cites the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only; no exceptions cross this boundary; every
 * function returns an alll_status (0 = ok) and alll_last_error() describes the last
 * failure on the calling thread.  Literals use the reference encoding of
 * example/main.cpp:168: DIMACS x>0 -> 2(x-1), -x -> 2(x-1)+1 (variable = l >> 1).
 */
#ifndef ALLL_H
#define ALLL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALLL_ABI_VERSION 1

typedef enum alll_status {
    ALLL_OK = 0,
    ALLL_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bad option */
    ALLL_ERR_BAD_INPUT = 2,     /* malformed CSR or DIMACS (header, missing clauses) */
    ALLL_ERR_LITERAL_RANGE = 3, /* literal variable >= n_vars (reference: UB, Clause.h:40) */
    ALLL_ERR_HIP = 4,           /* HIP runtime failure */
    ALLL_ERR_RCCL = 5,          /* RCCL failure */
    ALLL_ERR_MAX_ITERS = 6,     /* max_iters eval passes done, instance not solved */
    ALLL_ERR_NO_DEVICE = 7,     /* no usable gfx950 device */
    ALLL_ERR_OOM = 8,           /* device or host allocation failed */
    ALLL_ERR_IO = 9,            /* file could not be opened / read */
    ALLL_ERR_UNSUPPORTED = 10   /* size beyond the implementation limits */
} alll_status;

/* Instance in CSR form (replaces vector<ClauseArray*> of Clause<T>*, Clause.h:17-28;
 * the chunking of example/main.cpp:149-178 is irrelevant to the T=1 semantics). */
typedef struct alll_problem {
    uint32_t n_vars;            /* VariablesArray<T>::n_vars (VariablesArray.h:20) */
    uint32_t pad;
    uint64_t n_clauses;
    const uint64_t* offsets;    /* n_clauses+1, offsets[0] = 0, non-decreasing */
    const uint32_t* literals;   /* offsets[n_clauses] encoded literals */
} alll_problem;

/* flags */
#define ALLL_FLAG_NO_GRAPH          (1u << 0) /* launch eagerly instead of replaying a hipGraph */
#define ALLL_FLAG_EXCHANGE_ALLREDUCE (1u << 1) /* multi-GPU: shard resample + allreduce of the
                                                 bit-packed assignment delta (north_star form) */
#define ALLL_FLAG_GENERIC_CSR       (1u << 2) /* disable the fixed-width clause layout */
#define ALLL_FLAG_NO_RANGED         (1u << 3) /* use the L2-gather eval kernel instead of the
                                                 persistent LDS/L2 hybrid */
#define ALLL_FLAG_KERNEL_TIMING     (1u << 4) /* stamp every loop iteration with device wall-clock
                                                 times (alll_loop_times) */
#define ALLL_FLAG_ATOMIC_CLAIMS     (1u << 5) /* LFMIS round 0 by global atomicMin claims instead of
                                                 the variable-bucketed LDS resolution */
#define ALLL_FLAG_LFMIS             (1u << 6) /* n_threads > 1: keep the one-set MIS (the
                                                 lexicographically-first MIS in clause order, fast)
                                                 instead of the reference's T-set round robin */
#define ALLL_FLAG_REFERENCE_RNG     (1u << 7) /* the reference's own random stream instead of Philox:
                                                 RBG<default_random_engine> (RandomBoolGenerator.h,
                                                 libstdc++ minstd_rand0 + uniform_int_distribution
                                                 <unsigned long long>), every engine seeded with the
                                                 next value of std::random_device, for which `seed`
                                                 is the state of the 64-bit LCG stand-in of
                                                 oracle/ref_probe.cpp (x = x*6364136223846793005 +
                                                 1442695040888963407, value x >> 33): the initial
                                                 fill (VariablesArray.h:23-34) and every resample
                                                 round (SATInstance.h:340-365, T = 1) then equal the
                                                 reference's, bit for bit (the draws in parallel by
                                                 jump-ahead; about half the Philox loop's rate at
                                                 10M clauses).  n_threads = 1 (also for the streaming
                                                 solve: bits in yield order), one GPU:
                                                 ALLL_ERR_UNSUPPORTED otherwise */

typedef struct alll_options {
    uint64_t seed;          /* Philox4x32-10 key; replaces std::random_device (SATInstance.h:346) */
    uint64_t max_iters;     /* cap on eval passes (n_iterations); 0 = unlimited like the reference */
    int32_t device;         /* HIP device ordinal; -1 = current device */
    int32_t n_threads;      /* the reference's n_threads T (SATInstance.h:51): T > 1 makes the MIS
                               the round-robin greedy over T clause chunks (populate_mis_parallel,
                               SATInstance.h:414-447; at most 4096 chunks) unless ALLL_FLAG_LFMIS */
    int32_t rank;           /* clause shard of this process (0 .. world-1) */
    int32_t world;          /* number of GPUs the clauses are sharded over (1 = single GPU) */
    uint8_t comm_id[128];   /* RCCL unique id from alll_comm_unique_id() on rank 0 (world > 1);
                               all zero: no RCCL, alll_set_host_exchange() is required.  With
                               world == 1 a non-zero id creates a one-rank communicator and runs
                               the clause-sharded exchange path on one GPU (a rehearsal of the
                               multi-GPU path; the results are the same) */
    uint32_t flags;         /* ALLL_FLAG_* */
    uint32_t grid_rounds;   /* full-grid LFMIS rounds before the tail kernel (0 = default; at most 64) */
    uint64_t stream_batch;  /* 0: SATInstance::solve(vector<ClauseArray*>*) semantics.  > 0: the
                               streaming solve SATInstance::solve(getEnumeratedClause, n_clauses,
                               batch_size) (SATInstance.h:70-153) with this batch size and
                               n_threads clause generators (ClauseGenerator.h:32-71): with one
                               thread the MIS follows the generator's yield order; with n_threads
                               = T > 1 every batch step runs the T-set round robin over the T
                               generators' violated lists, filtered by the MIS so far
                               (SATInstance.h:98-125, 391-447), and the end-of-iteration check
                               runs in lock step.  T > 1 returns
                               ALLL_ERR_UNSUPPORTED for an empty clause, for world > 1, and from
                               alll_solve / alll_run at an iteration whose generators would never
                               finish at the same batch step (the reference's loop does not end
                               there).  ALLL_FLAG_LFMIS keeps the one-thread order for any T.
                               alll_stats reports the reference's statistics (n_iterations =
                               stream iterations, avg_mis_size summed per batch step); max_iters
                               then caps stream iterations */
    const uint64_t* set_starts; /* n_threads > 1: n_threads + 1 non-decreasing clause indices,
                               chunk q = [set_starts[q], set_starts[q+1]), set_starts[0] = 0,
                               set_starts[n_threads] = n_clauses (the sizes of the caller's
                               vector<ClauseArray*>); NULL = the chunking of example/main.cpp:
                               149-178.  Read by alll_create only */
} alll_options;

#define ALLL_MAX_GPU_STATS 64

/* Replaces struct Statistics (SATInstance.h:25-32). */
typedef struct alll_stats {
    uint64_t n_iterations;   /* eval passes, including the final zero-violation pass */
    uint64_t n_resamples;    /* sum of clause lengths over every MIS clause */
    uint64_t avg_mis_size;   /* floor(sum |MIS_i| / n_iterations) (SATInstance.h:317) */
    uint64_t sum_mis_size;
    uint64_t n_violated;     /* violated clauses found by the last eval pass */
    int32_t solved;          /* 1 if the last eval pass found no violated clause */
    int32_t n_gpus;          /* entries used in gpu_resamples */
    uint32_t lfmis_rounds_max;  /* most LFMIS rounds one iteration needed (grid + tail) */
    uint32_t lfmis_tail_rounds; /* rounds run by the tail kernel in the last iteration */
    uint64_t gpu_resamples[ALLL_MAX_GPU_STATS]; /* per clause-shard share of n_resamples */
} alll_stats;

/* Per-phase device time (ms, averaged over the profiled iterations), from HIP events on
 * the solver's stream. */
typedef struct alll_phase_times {
    double eval_ms;          /* clause evaluation + compaction kernel */
    double exchange_ms;      /* RCCL collectives + collect (0 on one GPU) */
    double mis_ms;           /* count reduction + LFMIS rounds + tail */
    double resample_ms;      /* Philox resample kernel */
    double total_ms;         /* whole iteration */
    uint64_t iterations;
} alll_phase_times;

typedef struct alll_ctx alll_ctx;

const char* alll_version(void);
const char* alll_last_error(void);
void alll_default_options(alll_options* opt);

/* Number of visible HIP devices (0 without a GPU; never fails). */
int alll_device_count(void);

/* RCCL unique id for a multi-GPU solver (rank 0 creates it, all ranks pass it in
 * alll_options.comm_id). */
int alll_comm_unique_id(uint8_t out[128]);

/* Host-staged exchange for the clause-sharded mode (alternative to RCCL, e.g. several
 * ranks sharing one GPU, or CPU-side collectives): op ALLL_XCHG_ALLGATHER -- `buf` holds
 * world * `bytes` bytes, this rank's piece at rank * bytes is filled, gather the others in
 * place; op ALLL_XCHG_ALLREDUCE_SUM_U32 -- element-wise sum of `bytes`/4 uint32 in place.
 * Return 0 on success. */
#define ALLL_XCHG_ALLGATHER 0
#define ALLL_XCHG_ALLREDUCE_SUM_U32 1
typedef int (*alll_exchange_fn)(void* user, int op, void* buf, uint64_t bytes);

/* Replaces SATInstance<T>(VariablesArray<T>*, int n_threads) (SATInstance.h:51-56) plus the
 * random initial assignment of VariablesArray<T>(n_vars) (VariablesArray.h:23-34).  Copies
 * the caller's CSR to the device; keeps no caller pointer. */
int alll_create(const alll_problem* prob, const alll_options* opt, alll_ctx** out);
int alll_destroy(alll_ctx* ctx);

/* Use a host-staged exchange instead of RCCL (world > 1; create with an all-zero comm_id). */
int alll_set_host_exchange(alll_ctx* ctx, alll_exchange_fn fn, void* user);

/* Replaces Statistics* SATInstance::solve(vector<ClauseArray*>*) (SATInstance.h:60-66 ->
 * parallel_solve :217-320).  Runs until no clause is violated (ALLL_OK) or max_iters
 * eval passes were done (ALLL_ERR_MAX_ITERS).  Statistics accumulate over calls. */
int alll_solve(alll_ctx* ctx, alll_stats* stats);

/* Fixed-iteration mode (benchmarks, step-by-step parity tests): run n_iters more full
 * iterations (eval + MIS + resample); stops early only when an eval pass finds no
 * violated clause.  Asynchronous unless stats != NULL. */
int alll_run(alll_ctx* ctx, uint64_t n_iters, alll_stats* stats);

int alll_get_stats(alll_ctx* ctx, alll_stats* stats);

/* Replaces bool SATInstance::verify_validity(vector<ClauseArray*>*) const
 * (SATInstance.h:156-173): one device eval pass over the current assignment. */
int alll_verify(alll_ctx* ctx, int* valid, uint64_t* n_violated);

/* Current assignment as n_vars bytes of 0/1 (the bool vars[] of VariablesArray.h:21). */
int alll_get_assignment(alll_ctx* ctx, uint8_t* out, uint64_t n);
int alll_set_assignment(alll_ctx* ctx, const uint8_t* in, uint64_t n);
/* Bit-packed form: ceil(n_vars/32) words, bit v%32 of word v/32. */
int alll_get_assignment_words(alll_ctx* ctx, uint32_t* out, uint64_t n_words);
int alll_set_assignment_words(alll_ctx* ctx, const uint32_t* in, uint64_t n_words);

/* Per-variable resample probabilities and pinned variables.  thr[v] (n == n_vars
 * entries, alll_var_threshold) gives variable v its own draw, at the initial fill and at every
 * resample (round it = n_iterations - 1):
 *   u(v, it) = Philox4x32-10(key = seed, ctr = {v >> 2, it lo, 1, it hi})[v & 3]
 *   u0(v)    = Philox4x32-10(key = seed, ctr = {v >> 2, 0, 0xFFFFFFFE, 0})[v & 3]     (initial fill)
 *   bit      = thr[v] == 0xFFFFFFFF ? 1 : (u < thr[v])
 * (the four output words in Random123 order).  thr = 0 pins the variable to 0 and thr = 0xFFFFFFFF
 * to 1: no resample changes it; any other value gives P(1) = thr / 2^32.  Counter word 2 (0 in the
 * unbiased resample, 0xFFFFFFFF in the unbiased fill) keeps these draws disjoint from the unbiased
 * stream: thr = 2^31 everywhere is a fair coin, but it is NOT the stream of a context without
 * thresholds.  A variable that occurs twice in a clause is drawn once.
 * Allowed only before the first iteration (n_iterations == 0), else ALLL_ERR_INVALID_ARG, as a
 * wrong n.  The call copies the thresholds (no caller pointer is kept), rewrites the assignment
 * with the biased fill and takes effect from the next iteration on; thr == NULL restores the
 * unbiased stream and the unbiased fill.  alll_set_assignment* afterwards is not checked against
 * the pins: a pinned variable keeps whatever value the caller gives it.  A clause whose literals
 * are all pinned false can never be satisfied: the loop then runs to max_iters (not detected on
 * the host; alll_propagate_pins below finds such clauses, also those the pins imply, before the
 * loop starts).  Supported: any n_threads, every flag that does not change results, one GPU.
 * ALLL_ERR_UNSUPPORTED, before any device work (the message names the reason): a context created
 * with ALLL_FLAG_REFERENCE_RNG, ALLL_FLAG_EXCHANGE_ALLREDUCE, world != 1 or a non-zero comm_id, or
 * stream_batch != 0.  (No reference counterpart: the reference draws fair coins.) */
int alll_set_var_thresholds(alll_ctx* ctx, const uint32_t* thr, uint64_t n);

/* The best assignment seen: an anytime answer for runs that end at max_iters.
 * Opt-in, off by default.  While it is on, the device keeps a record of the best eval pass of the
 * loop:
 *   n_violated  the smallest number of violated clauses any eval pass has found;
 *   iteration   the n_iterations value of the first pass that found it (the comparison is a strict
 *               `<`: a later pass that ties the minimum does not replace the record);
 *   words       the assignment that pass evaluated, ceil(n_vars/32) words: the assignment before
 *               that pass's resample.
 * Contract:
 *  - Before any pass has run, iteration == 0, n_violated == UINT64_MAX and `words` is left untouched.
 *  - Only passes of the loop count (alll_solve, alll_run and their batch and group forms);
 *    alll_verify, alll_bench_eval and alll_profile's standalone counts never touch the record.
 *  - The solved pass (no violated clause) and the capped pass (the max_iters-th pass of alll_solve,
 *    which does not resample) are passes like any other: if one is the strict minimum, it is the
 *    record.
 *  - A later alll_run lifts the cap and continues the loop; the record survives the continuation
 *    unchanged until a pass beats it.  run(a) then run(b) gives the record of run(a + b), and
 *    alll_solve in several calls that of one call.
 *  - alll_set_assignment* does not touch the record: the next pass evaluates the new assignment and
 *    replaces the record only if it is strictly better.
 *  - alll_set_var_thresholds and alll_track_best may come in either order while n_iterations == 0
 *    (the record is still empty); the record obeys pins, being an assignment the loop produced.
 *  - Nothing else changes: trajectory, statistics, MIS and violated mask of a tracking context are
 *    bit for bit those of one that does not track.
 * alll_track_best(on != 0 / 0) is allowed only while no iteration has run (the loop's kernels take
 * their buffers by value and captured iterations keep them): afterwards ALLL_ERR_INVALID_ARG, and
 * nothing changes.  It refuses the contexts alll_set_var_thresholds refuses, with
 * ALLL_ERR_UNSUPPORTED before any device work (the message names the reason): ALLL_FLAG_REFERENCE_RNG,
 * ALLL_FLAG_EXCHANGE_ALLREDUCE, world != 1 or a non-zero comm_id, stream_batch != 0.  Supported: any
 * n_threads, ALLL_FLAG_LFMIS and every flag that does not change results.
 * alll_get_best drains the stream; n_violated, iteration and words may each be NULL; n_words must be
 * ceil(n_vars/32) when words is given.  A null handle, a wrong n_words, or a context that does not
 * track (the message says so): ALLL_ERR_INVALID_ARG.  (No reference counterpart: the reference
 * returns the last assignment.) */
int alll_track_best(alll_ctx* ctx, int on);
int alll_get_best(alll_ctx* ctx, uint64_t* n_violated, uint64_t* iteration, uint32_t* words, uint64_t n_words);

/* Unit propagation of the pinned variables.  A literal l (variable v = l >> 1,
 * negated when l & 1) is, under thresholds thr,
 *   false  when thr[v] == (negated ? 0xFFFFFFFF : 0),
 *   true   when thr[v] == (negated ? 0 : 0xFFFFFFFF),
 *   free   otherwise (a bias that is not a pin is free).
 * Propagation runs in rounds; every clause of a round is judged against the thresholds as they stood
 * at the round's start:
 *  1. a clause with a true literal is ignored;
 *  2. a clause with no true and no free literal is falsified (an empty clause is): if any clause is,
 *     the call ends with status ALLL_PROP_CONFLICT, conflict_clause = the smallest falsified clause
 *     index, and the round applies nothing (the thresholds are those of the round's start);
 *  3. otherwise a clause with no true literal whose free literals all are one literal is a unit and
 *     forces it (x x !y with y pinned 1 is a unit; x !x is not);
 *  4. no unit: ALLL_PROP_FIXPOINT;
 *  5. max_rounds != 0 and that many rounds already applied: ALLL_PROP_ROUND_CAP, nothing applied;
 *  6. otherwise every forced literal is applied at once: thr[v] = 0xFFFFFFFF for a forced 2v, 0 for a
 *     forced 2v+1; a variable forced both ways in one round is pinned to 1 (the next round finds the
 *     clause that wanted 0 falsified); rounds += 1, n_forced += the variables changed.
 * The result does not depend on any execution order. */
#define ALLL_PROP_FIXPOINT 0
#define ALLL_PROP_CONFLICT 1
#define ALLL_PROP_ROUND_CAP 2
#define ALLL_PROP_NONE 3          /* group / batch item without thresholds: left alone */
typedef struct alll_propagate_result {
    uint64_t conflict_clause;     /* n_clauses when there is none (item-local index in a group / batch) */
    uint64_t n_forced;            /* variables this call pinned */
    uint32_t rounds;              /* rounds that applied something */
    int32_t status;               /* ALLL_PROP_* */
} alll_propagate_result;          /* 24 bytes */
/* Propagates the pins of the context's thresholds on the device (max_rounds = 0: until a fixpoint or
 * a conflict, at most n_vars + 1 rounds).  Allowed only while n_iterations == 0, on a context that
 * has thresholds, else ALLL_ERR_INVALID_ARG (the message says which); it refuses the contexts
 * alll_set_var_thresholds refuses, with ALLL_ERR_UNSUPPORTED.  Afterwards the context is, bit for
 * bit, a fresh context given the propagated thresholds through alll_set_var_thresholds (the
 * assignment is rewritten with the biased fill); a second call returns the same status with
 * rounds == 0 and n_forced == 0 (after ALLL_PROP_ROUND_CAP it makes up to max_rounds more rounds).  It may come before or after alll_track_best.  A conflict leaves
 * the context usable (the loop then runs to max_iters, as above).
 * alll_get_var_thresholds copies the context's thresholds (n == n_vars), the propagated ones after
 * the call above; a context without thresholds: ALLL_ERR_INVALID_ARG.  (No reference counterpart.) */
int alll_propagate_pins(alll_ctx* ctx, uint64_t max_rounds, alll_propagate_result* res);
int alll_get_var_thresholds(alll_ctx* ctx, uint32_t* out, uint64_t n);

/* Split scores: which free variable to pin next.  The literal states under
 * thresholds thr are those of the propagation above (true, false, free; a bias that is not a pin is
 * free); without thresholds every variable is free.  For every clause c:
 *  - c is open when it has no true literal (an empty clause and a falsified clause are open);
 *  - f(c) is the number of free literal occurrences in c, with multiplicity (x x !y with y pinned 1:
 *    f = 2; x !x: f = 2);
 *  - an open clause with f >= 1 adds w(f) = 1 << (16 - min(f, 16)) to S[l] for every free occurrence
 *    l in it: Jeroslow-Wang weights in integers (32768 for a unit, 8192 for three free literals, 1
 *    from 16 free literals on).  Integers and + only: the result does not depend on any execution
 *    order; with fewer than 2^32 literals S[l] < 2^47;
 *  - a satisfied clause, and an open clause with f = 0, adds nothing.
 * The scores do not detect conflicts: that is the propagation's job.  After a propagation that ended
 * in ALLL_PROP_FIXPOINT, var == n_vars holds exactly when n_open == 0: the pins satisfy every clause. */
typedef struct alll_split_result {
    uint64_t score_pos;           /* S[2 var]     (0 when var == n_vars) */
    uint64_t score_neg;           /* S[2 var + 1] */
    uint64_t n_open;              /* open clauses, falsified and empty ones included */
    uint32_t var;                 /* argmax over v of T(v) = S[2v] + S[2v+1], T > 0, the lowest v on a tie;
                                     n_vars when every T is 0 */
    uint32_t pad;                 /* 0 */
} alll_split_result;              /* 32 bytes */
/* The split record of the context under its current thresholds (a context without thresholds: every
 * variable free), computed on the device; scores: NULL, or n_scores == 2 * n_vars entries that
 * receive S.  Allowed at any time: the call drains the stream and changes nothing in the context --
 * assignment, statistics, best record, thresholds and the trajectory afterwards are bit for bit
 * those of a context that never called it.  It refuses the contexts alll_set_var_thresholds refuses,
 * with ALLL_ERR_UNSUPPORTED; a null context, a null res, a context that belongs to a group or a
 * wrong n_scores: ALLL_ERR_INVALID_ARG.  (No reference counterpart.) */
int alll_var_scores(alll_ctx* ctx, uint64_t* scores, uint64_t n_scores, alll_split_result* res);

/* Failed-literal probing: what happens if a literal is pinned, for many literals at
 * once.  A probe is a literal l = 2v + sign; its result is by definition what alll_pinned_propagate
 * returns on a copy of the thresholds with l pinned true (thr[v] = 0xFFFFFFFF for l = 2v, 0 for
 * l = 2v + 1; no thresholds: every variable a fair coin) under the same max_rounds: the six rules
 * above, unchanged, and the same record -- n_forced does not count the probe's own variable.
 *  - A probe whose variable the base thresholds already pin, either way: ALLL_PROP_NONE, 0 rounds,
 *    0 forced, conflict_clause = n_clauses; its rows (below) are the base's pins.
 *  - Duplicates and both polarities of one variable are allowed: every probe is independent.
 *  - The base need not be a fixpoint; every probe then repeats the base's own implications (and a
 *    base in conflict makes every probe a conflict): callers should propagate the base first.
 * Uses: a probe that ends in ALLL_PROP_CONFLICT is a failed literal (its negation is implied); a
 * variable pinned to the same value under l and under its complement is a necessary assignment;
 * n_forced of both branches is a look-ahead measure for the split variable.
 * The optional rows pm_rows and pv_rows are n_probes x n_words words each, n_words = ceil(n_vars/32):
 * bit v & 31 of pm_rows[p * n_words + (v >> 5)] says that v is pinned when probe p ends (the base's
 * pins, the probe's own and the forced ones), the same bit of pv_rows its value; after a conflict
 * that is the state at the start of the conflict round.  Bits past n_vars are 0, pv is 0 where pm
 * is 0.  A bias is never changed: the rows and the base thresholds give the propagated thresholds
 * of every probe.
 * alll_probe_literals runs the probes on the device under the context's current thresholds (none:
 * every variable free): one pass over the clauses advances 64 probes by a round.  Allowed at any
 * time: the call drains the stream and changes nothing in the context -- assignment, statistics,
 * best record, thresholds and the trajectory afterwards are bit for bit those of a context that
 * never called it.  It refuses the contexts alll_set_var_thresholds refuses, with
 * ALLL_ERR_UNSUPPORTED before any device work; a null context, null results, null probes with
 * n_probes != 0, a probe l >= 2 * n_vars (checked for all probes before anything is written), rows
 * with n_words != ceil(n_vars/32) or a context that belongs to a group: ALLL_ERR_INVALID_ARG.
 * n_probes == 0: ALLL_OK, nothing is written.  n_probes may be any number: the runtime works in
 * chunks of 64-probe slabs under a byte budget for its scratch (env ALLL_PROBE_SLABS forces the
 * chunk's size in slabs, whatever the budget says).  (The group form is alll_group_probe_literals,
 * declared with the groups; no batch form.  No reference counterpart.) */
int alll_probe_literals(alll_ctx* ctx, const uint32_t* probes, uint64_t n_probes, uint64_t max_rounds,
                        alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, uint64_t n_words);

/* The residual formula under the pins: what is left of the instance once the
 * pinned variables are decided.  The literal states under thresholds thr are those of the propagation
 * above (true, false, free; a bias that is not a pin is free); without thresholds every variable is
 * free.
 *  - A clause with a true literal is dropped.
 *  - Every other clause is kept; its residual clause is its free literal occurrences, in their order,
 *    with multiplicity (x x !y with y pinned 1 becomes x x; x !x stays x !x).
 *  - A kept clause with no free occurrence (falsified, or empty in the original) is kept as an empty
 *    clause and counted in n_falsified; first_falsified is the smallest such original index, the
 *    original n_clauses when there is none.
 *  - Kept clauses keep their relative order: clause_map[j] is the original index of residual clause j,
 *    and it ascends.
 *  - A variable is kept when it has a free occurrence in a kept clause.  Kept variables are renumbered
 *    in ascending order: var_map[u] is the original variable of residual variable u, and a residual
 *    literal is 2 u + sign.
 *  - thr_out[u] = thr[var_map[u]]: biases are carried; without thresholds it is 0x80000000.
 *  - offsets are 64-bit, start at 0 and have n_clauses + 1 entries, as in alll_problem.
 * Integers and a stable order: the result does not depend on any execution order.  No subsumption,
 * pure-literal or duplicate removal: the residual is the formula as written, minus what the pins
 * decide.
 * Lift: the full assignment of a residual assignment has the pinned variables at their pins, the kept
 * variables at their residual bits and every other variable 0.  With n_falsified == 0, an assignment
 * that satisfies the residual lifts to one that satisfies the original. */
typedef struct alll_residual_result {
    uint64_t n_clauses;           /* kept clauses */
    uint64_t n_literals;          /* their free literal occurrences */
    uint64_t n_falsified;         /* kept clauses without a free occurrence */
    uint64_t first_falsified;     /* the smallest of them (original index); the original n_clauses: none */
    uint32_t n_vars;              /* kept variables */
    uint32_t pad;                 /* 0 */
} alll_residual_result;           /* 40 bytes */
/* The residual of the context's instance under its current thresholds, compacted on the device.
 * Every output array may be NULL (the record alone); the capacities are the original sizes -- offsets
 * n_clauses + 1, literals the original literal count, var_map and thr_out n_vars, clause_map
 * n_clauses -- which the residual never exceeds; only the used prefixes are written.  Allowed at any
 * time: the call drains the stream and changes nothing in the context.  It refuses the contexts
 * alll_set_var_thresholds refuses, with ALLL_ERR_UNSUPPORTED, before any device work; a null context,
 * a null res or a context that belongs to a group: ALLL_ERR_INVALID_ARG.  (No reference counterpart.) */
int alll_residual(alll_ctx* ctx, alll_residual_result* res, uint64_t* offsets, uint32_t* literals, uint32_t* var_map,
                  uint64_t* clause_map, uint32_t* thr_out);

/* Introspection of the last iteration (parity tests): violated bitmask of the last eval
 * pass (ceil(n_clauses/64) words) and the MIS picked from it (ascending clause order). */
int alll_get_violated_mask(alll_ctx* ctx, uint64_t* out, uint64_t n_words);
int alll_get_mis(alll_ctx* ctx, uint32_t* out, uint64_t cap, uint64_t* n_out);

/* Benchmark helpers.  eval-only launches time the evaluation kernel alone on the current
 * assignment; profile runs n_iters iterations eagerly with HIP events around each phase. */
int alll_bench_eval(alll_ctx* ctx, int reps, double* avg_ms, uint64_t* n_violated);
int alll_profile(alll_ctx* ctx, uint64_t n_iters, alll_phase_times* out);
/* In-loop phase times of iterations [first_iter, first_iter + n_iters) as they ran (graph
 * replay included), from device wall-clock stamps taken by the kernels themselves; needs
 * ALLL_FLAG_KERNEL_TIMING at create.  eval_ms = evaluation kernel (first workgroup start to
 * last workgroup end); exchange_ms = evaluation end to reduce start (collectives + collect on
 * several GPUs, a launch gap on one); mis_ms = reduce start to LFMIS tail end; resample_ms =
 * tail end to the next evaluation start; total_ms = evaluation start to the next one.  Only
 * the last 4096 iterations are kept.  (No reference counterpart: measurement) */
int alll_loop_times(alll_ctx* ctx, uint64_t first_iter, uint64_t n_iters, alll_phase_times* out);
/* Block the host until all work queued on the solver's stream finished. */
int alll_synchronize(alll_ctx* ctx);
/* Bytes the evaluation kernel reads/writes per pass (algorithmic). */
uint64_t alll_eval_bytes(alll_ctx* ctx);
/* Layout in use: 0 generic CSR, k>0 fixed-width-k layout. */
int alll_layout(alll_ctx* ctx);
/* Name of the evaluation kernel the loop launches (e.g. "k_eval_hybrid<3>"). */
const char* alll_eval_kernel(alll_ctx* ctx);
/* 1 when the loop replays captured hipGraphs, 0 when it launches eagerly (ALLL_FLAG_NO_GRAPH, a
 * host-staged exchange, or a capture / instantiation that failed: the loop then falls back to
 * eager launches with the same results); *why (may be NULL) names the reason.  -1: null ctx.
 * (No reference counterpart: measurement honesty of the benchmark) */
int alll_uses_graphs(alll_ctx* ctx, const char** why);
/* Round robin (n_threads > 1): the pass log of the last iteration, 4 words per pass {dirty
 * entries, repair rounds (0xFFFFFFFF: the incremental pass gave up), entries decided, decisions
 * changed} for the incremental passes (zeros for full ones), at most 64 passes, then -- written
 * only with ALLL_FLAG_KERNEL_TIMING, zeros otherwise -- 64 words per pass of repair clock stamps
 * (100 MHz; words 0..5: detect, wide repair, repair, rounds end, repair end, decisions loaded;
 * from word 8 {round entries, stamp} pairs) and one 64-word row of k_fp_bbuild's phase stamps;
 * returns the words written (0 without incremental passes).  (No reference counterpart:
 * measurement) */
int alll_rr_pass_log(alll_ctx* ctx, uint32_t* out, uint32_t n_words);
/* Round robin: grid barriers of the incremental passes' wide repair rounds that timed out since
 * alll_create (each makes its pass give up and a full pass follow: correct, slower); -1 on failure.
 * Non-zero means the repair's workgroups were not all resident (the GPU shared with other work).
 * (No reference counterpart: measurement) */
int64_t alll_rr_barrier_timeouts(alll_ctx* ctx);
/* Owner-epoch counters since alll_create: out[0] round-robin iterations that started their owner
 * epochs over, out[1] round-robin iterations left to the batch kernel because their epochs ran out,
 * out[2] times the one-set loop (n_threads == 1, groups) started its 32-bit owner epochs over,
 * out[3] the one-set loop's first unused epoch.  (No reference counterpart: test support, the
 * tests at the epochs' ends) */
int alll_epoch_counters(alll_ctx* ctx, uint64_t out[4]);
/* Ranks taking part in the clause-sharded solve: ncclCommCount of the RCCL communicator, or
 * alll_options.world with a host-staged exchange (1 on one GPU); -1 on failure.  (The
 * reference counterpart is the thread count of the -p path, example/main.cpp:76-84.) */
int alll_comm_size(alll_ctx* ctx);

/* ---- batches of LDS-resident instances -------------------------------
 * Many small instances, or many seeds of one instance, solved at once: one workgroup owns one
 * item and runs its whole resample loop out of LDS, a grid of workgroups the batch.  Item i
 * behaves exactly as a context created from probs[i] with {seed = seeds[i], n_threads = 1,
 * flags = 0, max_iters}: same initial assignment, same MIS (lexicographically first, clause
 * order), same Philox resample, same statistics.  (No reference counterpart: the reference
 * solves one instance per SATInstance.) */
#define ALLL_BATCH_MAX_VARS 8192u
#define ALLL_BATCH_MAX_CLAUSES 8192u
#define ALLL_BATCH_MAX_LITERALS 24576u   /* a full 3-SAT item of 8192 clauses */
#define ALLL_BATCH_MAX_SLICE 65536u      /* most iterations one kernel launch may run */
#define ALLL_BATCH_FIRST_SOLVED (1u << 0)

typedef struct alll_batch alll_batch;

/* 1 when an item of this size fits a batch, else 0 (host-only). */
int alll_batch_fits(uint32_t n_vars, uint64_t n_clauses, uint64_t n_literals);
/* Item i = probs[i] with seed seeds[i].  Items may share offsets / literals arrays (a portfolio
 * of seeds over one instance): arrays equal in pointer and size are stored once.  Honoured
 * options: device, max_iters (one cap for every item); n_threads != 1, world != 1,
 * stream_batch != 0 and any flag: ALLL_ERR_UNSUPPORTED, as is an item beyond the limits above
 * (the message names the item).  Validated before any device is touched; keeps no caller
 * pointer. */
int alll_batch_create(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items,
                      const alll_options* opt, alll_batch** out);
int alll_batch_destroy(alll_batch* b);
/* The solve of every item: runs until each is solved or has done max_iters eval passes.  Returns
 * ALLL_OK when the call worked; status[i] (may be NULL) is ALLL_OK or ALLL_ERR_MAX_ITERS, stats
 * (may be NULL) holds n_items entries.  The items advance in slices of at most iters_per_launch
 * iterations per kernel launch; with ALLL_BATCH_FIRST_SOLVED the call returns after the first
 * slice in which an item became solved (or when no item can advance): every unfinished item has
 * then run the same whole number of slices, and a later call continues from there.  Statistics
 * accumulate over calls. */
int alll_batch_solve(alll_batch* b, uint32_t flags, alll_stats* stats, int32_t* status);
/* n_iters more full iterations (eval + MIS + resample) of every unfinished item; an item stops
 * early only at an eval pass that finds no violated clause.  stats: n_items entries or NULL. */
int alll_batch_run(alll_batch* b, uint64_t n_iters, alll_stats* stats);
int alll_batch_get_stats(alll_batch* b, uint64_t item, alll_stats* stats);
/* Bit-packed assignment of one item: ceil(n_vars/32) words. */
int alll_batch_get_assignment_words(alll_batch* b, uint64_t item, uint32_t* out, uint64_t n_words);
int alll_batch_set_assignment_words(alll_batch* b, uint64_t item, const uint32_t* in, uint64_t n_words);
/* Iterations per kernel launch, 1 .. ALLL_BATCH_MAX_SLICE; 0 = the measured default. */
int alll_batch_set_slice(alll_batch* b, uint64_t iters_per_launch);
/* alll_set_var_thresholds for one item (n == the item's n_vars; the key is seeds[item]): item i then
 * behaves exactly as a context created from probs[i] with {seed = seeds[i], n_threads = 1, flags = 0,
 * max_iters} and given the same thresholds (the biased fill u0, the biased draw u(v, it) with counter
 * word 2 = 1, the same statistics); items without thresholds keep the unbiased stream bit for bit.
 * Thresholds belong to the item, not to the stored problem: items that share one copy of the clauses
 * may each have their own.  Allowed while that item's n_iterations == 0, else ALLL_ERR_INVALID_ARG,
 * as n != the item's n_vars, a null batch or item >= n_items; a refused call changes nothing.  The
 * call copies the thresholds (no caller pointer is kept) and rewrites that item's assignment words
 * only; thr == NULL (n ignored) restores the unbiased fill and stream of that item.
 * alll_batch_set_assignment_words afterwards is not checked against the pins.  With
 * ALLL_BATCH_FIRST_SOLVED, items that are one instance under different pinned variables make a cube
 * portfolio (alll_pinned_conflict drops the cubes that cannot be met). */
int alll_batch_set_var_thresholds(alll_batch* b, uint64_t item, const uint32_t* thr, uint64_t n);
/* alll_propagate_pins for every item that has thresholds (results: n_items entries), in one kernel
 * launch, a workgroup per item: item i's result, thresholds and refilled words are exactly those of
 * a context of its own; conflict_clause is the item's own clause index.  An item without thresholds
 * is left alone and gets ALLL_PROP_NONE.  Refused with ALLL_ERR_INVALID_ARG when any item has made
 * an iteration.  alll_batch_get_var_thresholds copies one item's thresholds (n == its n_vars; an
 * item without thresholds: ALLL_ERR_INVALID_ARG). */
int alll_batch_propagate_pins(alll_batch* b, uint64_t max_rounds, alll_propagate_result* results);
int alll_batch_get_var_thresholds(alll_batch* b, uint64_t item, uint32_t* out, uint64_t n);
/* alll_track_best / alll_get_best per item (the contract above): switched for every
 * item at once, while no item has made an iteration (else ALLL_ERR_INVALID_ARG); every item keeps
 * its own record, in its own pass count, exactly that of a tracking context created from it.  The
 * records survive the slice boundaries and ALLL_BATCH_FIRST_SOLVED returns.  A null batch,
 * item >= n_items, a wrong n_words or a batch that does not track: ALLL_ERR_INVALID_ARG. */
int alll_batch_track_best(alll_batch* b, int on);
int alll_batch_get_best(alll_batch* b, uint64_t item, uint64_t* n_violated, uint64_t* iteration, uint32_t* words,
                        uint64_t n_words);

/* ---- block-diagonal groups: many instances of any size at once -------
 * The items are laid side by side as one instance with disjoint variable and clause ranges, and
 * the one-instance loop advances all of them by one iteration per iteration: no conflict edge
 * crosses items, so the union's violated set and its lexicographically-first MIS are the unions of
 * the items'.  Every item draws from its own Philox stream (key seeds[i], counter word = its own
 * word index) and keeps its own statistics and end, so item i behaves exactly as a context created
 * from probs[i] with {seed = seeds[i], n_threads = 1, flags = 0, max_iters}: the contract of the
 * batch above without its size limits (the union's are the loop's own).  An item
 * ends at its first eval pass with no violated clause of its own (the pass is counted, also when it
 * is the capped pass); its assignment and counters never change afterwards.  In alll_stats,
 * lfmis_rounds_max and lfmis_tail_rounds are the union's (the LFMIS rounds run over all items at
 * once), n_gpus is 1 and gpu_resamples[0] the item's n_resamples; every other field is the
 * item's own.  (No reference counterpart: the reference solves one instance per SATInstance.) */
#define ALLL_GROUP_FIRST_SOLVED (1u << 0)

typedef struct alll_group alll_group;

/* Item i = probs[i] with seed seeds[i]; items may share offsets / literals arrays (every item gets
 * its own copy of the clauses, shifted to its variables).  Honoured options: device, max_iters (one
 * cap for every item), grid_rounds and the flags that do not change results (ALLL_FLAG_NO_GRAPH,
 * _GENERIC_CSR, _NO_RANGED, _KERNEL_TIMING, _ATOMIC_CLAIMS); seed is unused.  n_threads != 1,
 * world != 1, stream_batch != 0, a non-zero comm_id, ALLL_FLAG_REFERENCE_RNG, _LFMIS,
 * _EXCHANGE_ALLREDUCE and a union beyond the loop's limits: ALLL_ERR_UNSUPPORTED; n_items == 0 or
 * a null pointer: ALLL_ERR_INVALID_ARG; a malformed item: the code alll_create gives, the message
 * names the item.  Validated before any device is touched; keeps no caller pointer. */
int alll_group_create(const alll_problem* probs, const uint64_t* seeds, uint64_t n_items,
                      const alll_options* opt, alll_group** out);
int alll_group_destroy(alll_group* g);
/* Runs until every item is solved or has done max_iters eval passes.  Returns ALLL_OK when the call
 * worked; status[i] (may be NULL) is ALLL_OK or ALLL_ERR_MAX_ITERS, stats (may be NULL) holds
 * n_items entries.  With ALLL_GROUP_FIRST_SOLVED the call returns once at least one item is solved
 * (at once when one already is): the solved item with the smallest n_iterations, the lowest index
 * on a tie, is the winner whatever the others ran meanwhile; every other item has then made a whole
 * number of iterations of its own trajectory and a later call continues from there.  Statistics
 * accumulate over calls. */
int alll_group_solve(alll_group* g, uint32_t flags, alll_stats* stats, int32_t* status);
/* n_iters more full iterations (eval + MIS + resample) of every unfinished item; stops early only
 * when all items are solved.  Asynchronous unless stats (n_items entries) != NULL. */
int alll_group_run(alll_group* g, uint64_t n_iters, alll_stats* stats);
int alll_group_get_stats(alll_group* g, uint64_t item, alll_stats* stats);
/* Bit-packed assignment of one item: ceil(n_vars/32) words.  Setting the assignment of a solved
 * item is refused (ALLL_ERR_INVALID_ARG): a solved item is final. */
int alll_group_get_assignment_words(alll_group* g, uint64_t item, uint32_t* out, uint64_t n_words);
int alll_group_set_assignment_words(alll_group* g, uint64_t item, const uint32_t* in, uint64_t n_words);
/* alll_set_var_thresholds for one item (n == the item's n_vars; v is local to the item and the key
 * is seeds[item]): item i then behaves exactly as a context created from probs[i] with seeds[i] and
 * given the same thresholds; items without thresholds keep the unbiased stream bit for bit.  Only
 * before the group's first iteration; rewrites that item's words only.  With
 * ALLL_GROUP_FIRST_SOLVED, items that are one instance under different pinned variables make a
 * cube portfolio: the first cube solved wins. */
int alll_group_set_var_thresholds(alll_group* g, uint64_t item, const uint32_t* thr, uint64_t n);
/* alll_propagate_pins over the union, all items at once (results: n_items entries): a global round
 * is every unfinished item's own round, and item i's result, thresholds and refilled words are
 * exactly those of a context of its own (rounds, forced count, the conflict clause in its local
 * index).  An item that has ended takes no further part and disturbs no other item; an item without
 * thresholds is left alone and gets ALLL_PROP_NONE.  Only before the group's first iteration.
 * alll_group_get_var_thresholds copies one item's thresholds (n == its n_vars; an item without
 * thresholds: ALLL_ERR_INVALID_ARG). */
int alll_group_propagate_pins(alll_group* g, uint64_t max_rounds, alll_propagate_result* results);
int alll_group_get_var_thresholds(alll_group* g, uint64_t item, uint32_t* out, uint64_t n);
/* alll_var_scores over the union, every item at once in one pass (results: n_items entries): item
 * i's record and scores are exactly those of a context of its own, in its local variable numbering
 * (var == its n_vars when nothing is left).  scores: NULL, or n_scores == the sum over the items of
 * 2 * n_vars_i entries, the items one after another in item order (without the union's word
 * padding).  An item without thresholds has every variable free; whether an item is solved or has
 * ended does not matter (the scores are a function of clauses and thresholds only).  At any time;
 * nothing in the group changes. */
int alll_group_var_scores(alll_group* g, alll_split_result* results, uint64_t* scores, uint64_t n_scores);
/* alll_residual over the union, every item in one pass (results: n_items entries): item i's record
 * and arrays are exactly those of a context of its own, in its local clause and variable numbering.
 * Every array may be NULL; the arrays are laid densely, one item after another in item order: item
 * i's offsets has results[i].n_clauses + 1 entries and starts at 0, its literals results[i].n_literals
 * entries, and so on (capacities: the sums of the items' original sizes, offsets n_clauses_i + 1
 * each).  An item without thresholds has every variable free.  At any time; nothing in the group
 * changes. */
int alll_group_residual(alll_group* g, alll_residual_result* results, uint64_t* offsets, uint32_t* literals,
                        uint32_t* var_map, uint64_t* clause_map, uint32_t* thr_out);
/* alll_track_best / alll_get_best per item (the contract above): switched for every
 * item at once, before the group's first iteration; the same ALLL_ERR_UNSUPPORTED contexts.  Every
 * item keeps its own record, in its local variable numbering and its own pass count, exactly that
 * of a tracking context created from it.  A solved item's record is its final assignment with
 * n_violated = 0 and iteration = its n_iterations; it never changes afterwards, whatever the other
 * items run.  A null group, item >= n_items, a wrong n_words or a group that does not track:
 * ALLL_ERR_INVALID_ARG. */
int alll_group_track_best(alll_group* g, int on);
int alll_group_get_best(alll_group* g, uint64_t item, uint64_t* n_violated, uint64_t* iteration, uint32_t* words,
                        uint64_t n_words);
/* alll_probe_literals for every item of a group at once.  Item i owns
 * probes[probe_offsets[i] .. probe_offsets[i + 1]) (n_items + 1 offsets from 0, not descending; an item
 * may have none), literals in the item's own numbering.  results[probe_offsets[i] + j] is exactly what
 * alll_probe_literals returns for that probe on a context of its own created from the item and given
 * the item's thresholds (none: every variable free): status, rounds and n_forced; conflict_clause is
 * the item's own index, its n_clauses when there is none.  max_rounds is one value for the call.  The
 * items' variables are disjoint, so one pass over the union's clauses advances 64 probes of every item.
 * The rows are optional and go together (both NULL or neither): item after item, item i's block is
 * n_probes_i x n_words_i words, n_words_i = ceil(n_vars_i / 32) with no padding to the union, row j
 * with the contract above; n_row_words must be the sum of the blocks when rows are given.
 * The contract is alll_group_var_scores': allowed at any time, the stream is drained, nothing in the
 * group changes; refused like alll_group_set_var_thresholds, with ALLL_ERR_UNSUPPORTED before any
 * device work.  ALLL_ERR_INVALID_ARG, nothing written: a null group, results or offsets; null probes
 * with a non-zero total; offsets that do not start at 0 or descend; one row array without the other;
 * a probe l >= 2 * n_vars of its own item (checked for all probes first -- such a literal can be a
 * valid one of the union); a wrong n_row_words.  No probes at all: ALLL_OK, nothing written.  Works in
 * chunks of layers (layer L: probes 64 L .. 64 L + 63 of every item that has them) under the byte
 * budget of alll_probe_literals; env ALLL_PROBE_SLABS forces the layers per chunk. */
int alll_group_probe_literals(alll_group* g, const uint32_t* probes, const uint64_t* probe_offsets, uint64_t max_rounds,
                              alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows, uint64_t n_row_words);
/* alll_layout / alll_eval_kernel / alll_epoch_counters of the union. */
int alll_group_layout(alll_group* g);
const char* alll_group_eval_kernel(alll_group* g);
int alll_group_epoch_counters(alll_group* g, uint64_t out[4]);

/* ---- host-side helpers (no GPU needed) ---------------------------------------------- */

/* DIMACS loader with the clause semantics of example/cnf_io (cnf_header_read
 * cnf_io.cpp:487-705 + cnf_data_read :126-328) and the encoding of main.cpp:157-178.
 * Two calls: first with offsets/literals NULL to get the sizes, then with buffers. */
int alll_dimacs_parse(const char* buf, uint64_t len, uint32_t* n_vars, uint64_t* n_clauses,
                      uint64_t* offsets, uint32_t* literals, uint64_t* n_literals);
/* Same from a file path (mmap). */
int alll_dimacs_read(const char* path, uint32_t* n_vars, uint64_t* n_clauses, uint64_t* offsets,
                     uint32_t* literals, uint64_t* n_literals);

/* Clause sharding of the multi-GPU mode (host-only): rank `rank` of `world` owns the clause
 * range [*clause_begin, *clause_end) (contiguous, 4096-clause tile aligned, so rank-major
 * concatenation is clause order) and contributes *mask_words_per_rank 64-bit words to the
 * per-iteration all-gather of the violated bitmask. */
int alll_shard_plan(uint64_t n_clauses, int world, int rank, uint64_t* clause_begin,
                    uint64_t* clause_end, uint64_t* mask_words_per_rank);

/* Multi-GPU plan for one instance on `world` GPUs of one node.  The exact
 * LFMIS and the resample run on every rank whatever the plan (their per-round minima over all
 * clauses would cost ~2 collectives per round), so only the evaluation can shard, and the
 * sharded plan (alll_shard_plan + the RCCL all-gather of the violated bitmask) pays an exchange
 * every iteration.  From the instance's size, the model predicts the evaluation time on one GPU,
 * what sharding saves of it, and the exchange's cost (marking, all-gather, collection of the
 * other shards' violated clauses, the round-0 scatter and reduce the exchange path cannot fuse),
 * with rates measured on one MI355X; `plan` is ALLL_PLAN_SHARD when the saving
 * exceeds the exchange, else ALLL_PLAN_REPLICATE: every rank runs the whole one-GPU loop (no
 * exchange; the trajectories are identical by construction, Philox keyed by seed, iteration
 * and word).  k_avg = literals / clauses. */
#define ALLL_PLAN_REPLICATE 0
#define ALLL_PLAN_SHARD 1
typedef struct {
    double eval_us_1gpu;   /* evaluation of the whole instance on one GPU */
    double eval_saved_us;  /* eval_us_1gpu * (1 - 1/world) */
    double exchange_us;    /* the sharded plan's per-iteration exchange */
    double violated_est;   /* violated clauses per iteration assumed: n_clauses * 2^-k_avg */
    int plan;              /* ALLL_PLAN_REPLICATE or ALLL_PLAN_SHARD */
    int pad;
} alll_multi_plan;
int alll_plan_multi_gpu(uint64_t n_clauses, uint64_t n_literals, uint32_t n_vars, int world,
                        alll_multi_plan* out);

/* The solver's initial assignment for `seed` as n_vars bytes of 0/1 (word w of the packed
 * form = Philox4x32-10(key=seed, ctr={w, 0, 0xFFFFFFFF, 0}).x); used by the compatibility
 * VariablesArray (replaces the random_device fill of VariablesArray.h:23-34). */
int alll_initial_assignment(uint64_t seed, uint32_t n_vars, uint8_t* out);

/* The threshold of probability p for alll_set_var_thresholds: p = 0 -> 0 (pinned to 0), p = 1 ->
 * 0xFFFFFFFF (pinned to 1), else min(floor(p * 2^32), 0xFFFFFFFE) (so p < 2^-32 pins to 0 and no
 * p < 1 pins to 1); NaN or p outside [0, 1]: ALLL_ERR_INVALID_ARG. */
int alll_var_threshold(double p, uint32_t* thr);
/* The biased initial fill (alll_set_var_thresholds, u0) for `seed` and n_vars thresholds, as
 * n_vars bytes of 0/1. */
int alll_biased_initial_assignment(uint64_t seed, uint32_t n_vars, const uint32_t* thr, uint8_t* out);
/* Pins that cannot be met: *clause = the index of the first clause whose literals are all pinned
 * false by thr (n == n_vars entries): a literal 2v when thr[v] == 0, a literal 2v+1 when thr[v] ==
 * 0xFFFFFFFF; an empty clause counts as one.  *clause = n_clauses when there is none.  The loop
 * does not detect such a clause (it runs to max_iters): a cube portfolio drops its dead cubes with
 * this before they occupy a workgroup.  Validates as alll_create: a null pointer or n != n_vars:
 * ALLL_ERR_INVALID_ARG; offsets that do not start at 0 or decrease: ALLL_ERR_BAD_INPUT; a literal
 * of a variable >= n_vars: ALLL_ERR_LITERAL_RANGE (*clause is then left alone). */
int alll_pinned_conflict(const alll_problem* prob, const uint32_t* thr, uint64_t n, uint64_t* clause);

/* The propagation of alll_propagate_pins on the host (the semantics above): thr (n == n_vars
 * entries) is updated in place.  Validation and error codes are those of alll_pinned_conflict;
 * nothing is written on an error.  Status ALLL_PROP_CONFLICT with rounds == 0 holds exactly when
 * alll_pinned_conflict reports the same clause. */
int alll_pinned_propagate(const alll_problem* prob, uint32_t* thr, uint64_t n, uint64_t max_rounds,
                          alll_propagate_result* res);

/* The probes of alll_probe_literals on the host (the semantics above) under thresholds thr (n ==
 * n_vars entries; thr == NULL: every variable a fair coin, n is not looked at): one
 * alll_pinned_propagate per probe.  results: n_probes records; pm_rows, pv_rows: NULL, or n_probes x
 * ceil(n_vars/32) words each.  Validation and error codes are those of alll_pinned_scores; null
 * probes with n_probes != 0 or a probe l >= 2 * n_vars: ALLL_ERR_INVALID_ARG; nothing is written on
 * an error. */
int alll_pinned_probe(const alll_problem* prob, const uint32_t* thr, uint64_t n, const uint32_t* probes, uint64_t n_probes,
                      uint64_t max_rounds, alll_propagate_result* results, uint32_t* pm_rows, uint32_t* pv_rows);

/* The split scores of alll_var_scores on the host (the semantics above) under thresholds thr (n ==
 * n_vars entries; thr == NULL: every variable free, n is not looked at).  scores: NULL, or 2 * n_vars
 * entries that receive S.  Validation and error codes are those of alll_pinned_conflict (but for
 * the null thr); nothing is written on an error. */
int alll_pinned_scores(const alll_problem* prob, const uint32_t* thr, uint64_t n, uint64_t* scores,
                       alll_split_result* res);

/* The residual of alll_residual on the host (the semantics above) under thresholds thr (n == n_vars
 * entries; thr == NULL: every variable free, n is not looked at).  Every output array may be NULL;
 * the capacities are the original sizes: offsets n_clauses + 1, literals the original literal count,
 * var_map and thr_out n_vars, clause_map n_clauses.  Validation and error codes are those of
 * alll_pinned_scores; nothing is written on an error.  (The batch form: batch items are small, and
 * this function serves them.) */
int alll_pinned_residual(const alll_problem* prob, const uint32_t* thr, uint64_t n, alll_residual_result* res,
                         uint64_t* offsets, uint32_t* literals, uint32_t* var_map, uint64_t* clause_map,
                         uint32_t* thr_out);

/* The reference's own initial assignment (VariablesArray.h:23-34) in the reference-RNG mode
 * (ALLL_FLAG_REFERENCE_RNG): `rd_state` is the random_device stand-in's state
 * before the fill draws its one value; the bytes equal the device fill of a context created
 * with that seed and the flag.  Used by the compatibility VariablesArray (env ALLL_REFERENCE_RNG). */
int alll_reference_initial_assignment(uint64_t rd_state, uint32_t n_vars, uint8_t* out);

/* Synthetic random k-SAT with k distinct variables per clause (kind 0 uniform, kind 1
 * power-law P(v) ~ (v+1)^-0.8); clauses [c_begin, c_end) of the instance, fixed width k. */
int alll_generate_ksat(uint64_t gen_seed, uint32_t n_vars, uint64_t n_clauses, uint32_t k,
                       int kind, uint64_t c_begin, uint64_t c_end, uint32_t* literals);

#ifdef __cplusplus
}
#endif
#endif /* ALLL_H */
