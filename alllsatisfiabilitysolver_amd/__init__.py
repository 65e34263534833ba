"""MI355X-native Moser-Tardos (Algorithmic Lovasz Local Lemma) SAT solver.

The hot path -- clause evaluation, violated-clause compaction, exact lexicographically-first
MIS and Philox resampling -- runs in hand-written gfx950 HIP kernels behind the C-ABI of
include/alll.h (liballl.so).  This package is the Python front-end of that library.
"""
from ._native import (AlllError, PROP_CONFLICT, PROP_FIXPOINT, PROP_NONE, PROP_ROUND_CAP, build, lib)  # noqa: F401
from .solver import (BatchSolver, Clause, GroupSolver, SATInstance, Solver, Statistics, VariablesArray,  # noqa: F401
                     batch_fits, solve_portfolio, solve_cubes, solve_cubes_propagated, cube_thresholds, pinned_conflict, propagate_pins, var_thresholds,
                     biased_initial_assignment, var_scores, split_cubes, solve_cubes_split,
                     residual_instance, lift_assignment, solve_cubes_residual,
                     probe_literals, failed_literal_reduce, split_cubes_lookahead, solve_cubes_lookahead,
                     assignment_digest, comm_unique_id, device_count, generate_ksat, generate_mixed, gloo_exchange,
                     parse_dimacs,
                     read_dimacs, shard_plan, plan_multi_gpu)

__version__ = "0.1.0"
