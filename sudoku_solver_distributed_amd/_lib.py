"""ctypes binding of libsudoku_hip.so (the C ABI declared in include/sudoku_hip.h).

There is no fallback: if the library is missing or fails to load, every entry
point raises.  Build it with ``python -m sudoku_solver_distributed_amd.build``
(or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDK_LIB selects another in-tree build of the same ABI (A/B experiments)
LIB_PATH = os.environ.get("SDK_LIB") or os.path.join(_HERE, "libsudoku_hip.so")

SDK_UNSOLVABLE = 0
SDK_SOLVED = 1
SDK_INVALID = -1
SDK_CANCELLED = -2
SDK_FAULT = -3       # internal consistency check failed (never expected)
SDK_NO_RETURN = -4   # sdk_peer_solve_batch: node.py's /solve loop never returns
SDK_PEER_STATE_BYTES = 1600  # sdk_peer_solve_seq: one node's partial_solution + tried sets
SDK_ORDER_GEN = 0    # gen.py:6-28's walk (last row with an empty cell first)
SDK_ORDER_NODE = 1   # node.py:62-74's walk (row-major)
ORDERS = {"gen": SDK_ORDER_GEN, "node": SDK_ORDER_NODE}

# every symbol include/sudoku_hip.h declares
EXPORTS = (
    "sdk_workspace_bytes",
    "sdk_solve_batch",
    "sdk_solve_batch_grid",
    "sdk_solve_batches",
    "sdk_check_batch",
    "sdk_first_candidate_batch",
    "sdk_peer_solve_batch",
    "sdk_peer_solve_seq",
    "sdk_expand_frontier",
    "sdk_read_stats",
    "sdk_snapshot_stats",
    "sdk_verify_workspace",
    "sdk_last_error",
    "sdk_version",
    "sdk_device_cu_count",
    "sdk_set_solve_kernel",
    "sdk_set_plane_tuning",
    "sdk_set_plane_search",
    "sdk_count_scratch_bytes",
    "sdk_count_solutions_batch",
    "sdk_canonical_scratch_bytes",
    "sdk_canonical_batch",
    "sdk_rate_scratch_bytes",
    "sdk_rate_batch",
    "sdk_logic_scratch_bytes",
    "sdk_logic_batch",
    "sdk_path_scratch_bytes",
    "sdk_path_batch",
    "sdk_candidates_scratch_bytes",
    "sdk_candidates_batch",
    "sdk_minimize_scratch_bytes",
    "sdk_minimize_batch",
    "sdk_sample_scratch_bytes",
    "sdk_sample_batch",
    "sdk_unique_candidates_scratch_bytes",
    "sdk_unique_candidates_batch",
    "sdk_count_exact_scratch_bytes",
    "sdk_count_exact_batch",
    "sdk_enumerate_scratch_bytes",
    "sdk_enumerate_batch",
    "sdk_backdoor_scratch_bytes",
    "sdk_backdoor_batch",
    "sdk_unavoidable_scratch_bytes",
    "sdk_unavoidable_batch",
    "sdk_unavoidable_minimal_batch",
    "sdk_hitting_sets_scratch_bytes",
    "sdk_hitting_sets_batch",
)
SDK_KERNELS = {"auto": 1, "packed": 5, "plane": 6}
SDK_MAX_BATCHES = 32  # sdk_solve_batches: batches per launch
SDK_COUNT_MAX_LIMIT = 1024  # sdk_count_solutions_batch: the largest cap
SDK_CANON_SYMMETRIES = 3359232  # sdk_canonical_batch: 2 * 1296 * 1296
SDK_CANON_MAX_SLICES = 2592  # ... and the most parts a board's search is cut into
SDK_RATE_MAX_LEVEL = 4  # sdk_rate_batch: the deepest rule level (trial eliminations)
SDK_RATE_NOT_RUN = -2  # ... and the open count of a level above max_level
SDK_LOGIC_MAX_STEPS = 8  # sdk_logic_batch: the most steps of a ladder
SDK_LOGIC_NOT_RUN = -2  # ... and the open / left count of a step past the ladder's end
# ... its rules: naked singles, hidden singles, locked candidates, subsets of 2..4, fish of 2..4
(SDK_LOGIC_N, SDK_LOGIC_H, SDK_LOGIC_L, SDK_LOGIC_S2, SDK_LOGIC_S3, SDK_LOGIC_S4, SDK_LOGIC_F2, SDK_LOGIC_F3,
 SDK_LOGIC_F4) = (1 << k for k in range(9))
SDK_PATH_DEAD = 0     # sdk_path_batch: the state has no completion
SDK_PATH_SOLVED = 1   # ... the rules solved it
SDK_PATH_STUCK = 2    # ... no rule of the mask removes a candidate
SDK_PATH_LIMITED = 3  # ... max_rounds rounds are done
SDK_MIN_GREEDY = 0  # sdk_minimize_batch: erase givens turn by turn while one completion is left
SDK_MIN_PROBE = 1   # ... or test every given alone against the input board
SDK_EXACT_DONE = 1     # sdk_count_exact_batch: the count is exact
SDK_EXACT_PARTIAL = 2  # ... or a lower bound: the round budget ran out
SDK_ENUM_DONE = 1     # sdk_enumerate_batch: the board's search ran out, its count is exact
SDK_ENUM_PARTIAL = 2  # ... the round budget ran out: a lower bound
SDK_ENUM_LIMITED = 3  # ... the board has at least `limit` completions
SDK_ENUM_MAX_ROWS = 2 ** 31 - 1  # ... and the largest capacity of its list
SDK_BACKDOOR_MAX_LEVEL = 3  # sdk_backdoor_batch: the deepest rule level of the closure
SDK_BACKDOOR_MAX_SIZE = 4   # ... the largest subset tried
SDK_BACKDOOR_MISMATCH = -2  # ... and the size of a grid that is not a completion of its board
SDK_UA_MAX_SIZE = 16     # sdk_unavoidable_batch: the largest set listed
SDK_UA_DONE = 1          # ... the status of a valid grid
SDK_UA_NOT_A_GRID = -2   # ... and of one in which a digit repeats in a unit
SDK_HIT_MAX_CLUES = 32   # sdk_hitting_sets_batch: the largest size k
SDK_HIT_DONE = 1         # ... the status of a family that ran to the end
SDK_HIT_LIMITED = 2      # ... and of one stopped at `limit` rows
SDK_GRID_PIPELINED = 0x10000  # grid_waves flag: another launch is queued behind this one
# device symbol of each solve kernel (rocprofv3 Kernel_Name, profiles/pmc_<symbol>.json)
KERNEL_SYMBOLS = {1: "plane_kernel", 5: "solvep_kernel", 6: "plane_kernel"}

_lib = None


class SudokuHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the HIP library (raises SudokuHipError if it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SudokuHipError(
            f"{LIB_PATH} not found: build it with `python -m sudoku_solver_distributed_amd.build`"
        )
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    L.sdk_workspace_bytes.restype = sz
    L.sdk_workspace_bytes.argtypes = []
    L.sdk_solve_batch.restype = i32
    L.sdk_solve_batch.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp]
    L.sdk_solve_batch_grid.restype = i32
    L.sdk_solve_batch_grid.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, i32]
    pp = ctypes.POINTER(ctypes.c_void_p)
    L.sdk_solve_batches.restype = i32
    L.sdk_solve_batches.argtypes = [pp, pp, pp, ctypes.POINTER(ctypes.c_int64), i32, vp, i32, vp, i32]
    L.sdk_check_batch.restype = i32
    L.sdk_check_batch.argtypes = [vp, vp, i64, i32, vp]
    L.sdk_first_candidate_batch.restype = i32
    L.sdk_first_candidate_batch.argtypes = [vp, vp, vp, i64, vp]
    L.sdk_peer_solve_batch.restype = i32
    L.sdk_peer_solve_batch.argtypes = [vp, vp, vp, vp, i64, vp]
    L.sdk_peer_solve_seq.restype = i32
    L.sdk_peer_solve_seq.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.sdk_expand_frontier.restype = i32
    L.sdk_expand_frontier.argtypes = [vp, i64, vp, vp, vp, i64, i32, vp]
    L.sdk_read_stats.restype = i32
    L.sdk_read_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), i32, vp]
    L.sdk_snapshot_stats.restype = i32
    L.sdk_snapshot_stats.argtypes = [vp, vp, vp]
    L.sdk_verify_workspace.restype = i32
    L.sdk_verify_workspace.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), vp]
    L.sdk_last_error.restype = ctypes.c_char_p
    L.sdk_last_error.argtypes = []
    L.sdk_version.restype = ctypes.c_char_p
    L.sdk_version.argtypes = []
    L.sdk_device_cu_count.restype = i32
    L.sdk_device_cu_count.argtypes = []
    L.sdk_set_solve_kernel.restype = i32
    L.sdk_set_solve_kernel.argtypes = [i32]
    L.sdk_set_plane_tuning.restype = i32
    L.sdk_set_plane_tuning.argtypes = [i32, i32, i32, i32]
    L.sdk_set_plane_search.restype = i32
    L.sdk_set_plane_search.argtypes = [i32]
    L.sdk_count_scratch_bytes.restype = sz
    L.sdk_count_scratch_bytes.argtypes = [i64, i32]
    L.sdk_count_solutions_batch.restype = i32
    L.sdk_count_solutions_batch.argtypes = [vp, vp, vp, i64, i32, vp, sz, i32, vp]
    L.sdk_canonical_scratch_bytes.restype = sz
    L.sdk_canonical_scratch_bytes.argtypes = [i64, i32]
    L.sdk_canonical_batch.restype = i32
    L.sdk_canonical_batch.argtypes = [vp, vp, vp, vp, i64, i32, vp, sz, vp]
    L.sdk_rate_scratch_bytes.restype = sz
    L.sdk_rate_scratch_bytes.argtypes = [i64, i32]
    L.sdk_rate_batch.restype = i32
    L.sdk_rate_batch.argtypes = [vp, vp, vp, vp, i64, i32, vp, sz, vp]
    L.sdk_logic_scratch_bytes.restype = sz
    L.sdk_logic_scratch_bytes.argtypes = [i64, i32]
    L.sdk_logic_batch.restype = i32
    L.sdk_logic_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, sz, vp]
    L.sdk_path_scratch_bytes.restype = sz
    L.sdk_path_scratch_bytes.argtypes = [i64, i32]
    L.sdk_path_batch.restype = i32
    L.sdk_path_batch.argtypes = [vp, vp, ctypes.c_uint32, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]
    L.sdk_candidates_scratch_bytes.restype = sz
    L.sdk_candidates_scratch_bytes.argtypes = [i64, i32]
    L.sdk_candidates_batch.restype = i32
    L.sdk_candidates_batch.argtypes = [vp, vp, vp, i64, vp, sz, i32, vp]
    L.sdk_minimize_scratch_bytes.restype = sz
    L.sdk_minimize_scratch_bytes.argtypes = [i64, i32]
    L.sdk_minimize_batch.restype = i32
    L.sdk_minimize_batch.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp, sz, i32, vp]
    L.sdk_sample_scratch_bytes.restype = sz
    L.sdk_sample_scratch_bytes.argtypes = [i64, i32]
    L.sdk_sample_batch.restype = i32
    L.sdk_sample_batch.argtypes = [vp, vp, vp, i64, i32, ctypes.c_uint64, ctypes.c_uint64, vp, sz, i32, vp]
    L.sdk_unique_candidates_scratch_bytes.restype = sz
    L.sdk_unique_candidates_scratch_bytes.argtypes = [i64, i32]
    L.sdk_unique_candidates_batch.restype = i32
    L.sdk_unique_candidates_batch.argtypes = [vp, vp, vp, vp, i64, vp, sz, i32, vp]
    L.sdk_count_exact_scratch_bytes.restype = sz
    L.sdk_count_exact_scratch_bytes.argtypes = [i64, i32, i64]
    L.sdk_count_exact_batch.restype = i32
    L.sdk_count_exact_batch.argtypes = [vp, vp, vp, i64, i32, i32, i64, vp, sz, i32, vp, ctypes.POINTER(ctypes.c_int64)]
    L.sdk_enumerate_scratch_bytes.restype = sz
    L.sdk_enumerate_scratch_bytes.argtypes = [i64, i32, i64]
    L.sdk_enumerate_batch.restype = i32
    L.sdk_enumerate_batch.argtypes = [vp, i64, vp, vp, i64, i64, vp, vp, i32, i32, i64, vp, sz, i32, vp,
                                      ctypes.POINTER(ctypes.c_int64)]
    L.sdk_backdoor_scratch_bytes.restype = sz
    L.sdk_backdoor_scratch_bytes.argtypes = [i64, i32, i32]
    L.sdk_backdoor_batch.restype = i32
    L.sdk_backdoor_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, sz, i32, vp]
    L.sdk_unavoidable_scratch_bytes.restype = sz
    L.sdk_unavoidable_scratch_bytes.argtypes = [i64, i32]
    L.sdk_unavoidable_batch.restype = i32
    L.sdk_unavoidable_batch.argtypes = [vp, i64, i32, vp, i64, vp, vp, vp, vp, sz, i32, vp]
    L.sdk_unavoidable_minimal_batch.restype = i32
    L.sdk_unavoidable_minimal_batch.argtypes = [vp, vp, i64, vp, i32, vp]
    L.sdk_hitting_sets_scratch_bytes.restype = sz
    L.sdk_hitting_sets_scratch_bytes.argtypes = [i64, i32]
    L.sdk_hitting_sets_batch.restype = i32
    L.sdk_hitting_sets_batch.argtypes = [vp, vp, vp, vp, i64, i32, i64, vp, i64, vp, vp, vp, vp, sz, i32, vp]
    _lib = L
    return L


def active_kernel() -> int:
    """The solve kernel selection now (SDK_KERNEL_*; AUTO runs the plane kernel
    at bench-sized batches)."""
    L = load()
    cur = L.sdk_set_solve_kernel(0)
    L.sdk_set_solve_kernel(cur)
    return cur


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sdk_last_error().decode(errors="replace")
        raise SudokuHipError(f"{what} failed ({rc}): {msg}")


def order_code(order) -> int:
    """'gen' | 'node' | SDK_ORDER_* -> SDK_ORDER_*."""
    if isinstance(order, str):
        if order not in ORDERS:
            raise ValueError(f"order must be one of {sorted(ORDERS)}")
        return ORDERS[order]
    if order not in (SDK_ORDER_GEN, SDK_ORDER_NODE):
        raise ValueError(f"bad order {order!r}")
    return int(order)
