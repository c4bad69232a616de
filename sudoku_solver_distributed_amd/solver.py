"""Device-side batch API over the C ABI (include/sudoku_hip.h).

PyTorch is plumbing here: it owns device memory, streams and
``torch.distributed``; all Sudoku work runs in libsudoku_hip.so.  Nothing in
this module falls back to a CPU path -- without a GPU or without the library
every call raises.

Boards are ``uint8`` tensors of shape ``(n, 81)`` (row-major, 0 = empty).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (SDK_CANCELLED, SDK_COUNT_MAX_LIMIT, SDK_INVALID, SDK_NO_RETURN, SDK_SOLVED, SDK_UNSOLVABLE,
                   SudokuHipError)

# count_exact's defaults (chosen from scripts/exact_bench.py's sweep; at these the heaviest fixture
# board needs 64 to 83 rounds and the empty board comes back PARTIAL after 6.4 s on one MI355X)
EXACT_SLICE = 256
EXACT_MAX_ROUNDS = 512
# unavoidable's first capacity per grid, by max_size: twice the most rows any grid of tests/golden/ua_cases.json has
# at that size (4..12, from its rows at 12); above 12, where the fixture records nothing, that figure grown 2.4 times
# a cell, the growth DESIGN.md §24's table shows.  A guess only: a list that overflows is asked for again in full.
UA_CAPACITY = {4: 32, 5: 32, 6: 162, 7: 162, 8: 170, 9: 330, 10: 578, 11: 1818, 12: 2070, 13: 4968, 14: 11923,
               15: 28615, 16: 68676}
# hitting_sets' first capacity in rows (16 bytes each); a list that overflows is asked for again in full
HIT_CAPACITY = 1 << 16
# the most candidates of one grid sub_puzzles lists (4 GiB of packed rows); more raises instead of an allocation failure
SUB_PUZZLES_MAX_ROWS = 1 << 28
# logic's rules (SDK_LOGIC_*: naked singles, hidden singles, locked candidates, subsets of 2..4, fish of 2..4) and
# the default ladder: singles, hidden singles, locked candidates, pairs, triples / quads, X-wing, swordfish / jellyfish
N, H, L, S2, S3, S4, F2, F3, F4 = (1 << k for k in range(9))
DEFAULT_LADDER = (N, N | H, N | H | L, N | H | L | S2, N | H | L | S2 | S3 | S4, N | H | L | S2 | S3 | S4 | F2, 0x1FF)
ALL = 0x1FF
# the columns of path's events and the names of its classes (the bit indices of a rule mask)
PATH_COLUMNS = ("round", "cls", "m", "I", "u", "removed", "left", "contradiction")
PATH_CLASSES = ("N", "H", "L", "S2", "S3", "S4", "F2", "F3", "F4")

__all__ = [
    "BatchSolver", "get_solver", "as_boards", "SDK_SOLVED", "SDK_UNSOLVABLE",
    "SDK_INVALID", "SDK_CANCELLED", "SDK_NO_RETURN", "SudokuHipError",
]


def _require_gpu(device) -> torch.device:
    if not torch.cuda.is_available():
        raise SudokuHipError("no ROCm GPU visible: the Sudoku solver runs only on the HIP path")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise SudokuHipError(f"device {dev} is not a GPU device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def as_boards(x, device=None, max_value: int = 9) -> torch.Tensor:
    """Anything board-like -> contiguous (n, 81) uint8 tensor (host or device).

    Accepts a 9x9 list of lists (the reference's board type), a list of such
    boards, an 81-char string, numpy arrays and tensors.  Raises ValueError on
    a cell outside 0..max_value: solving takes 0..9 (the reference's walk
    would silently compare other values), the check kernels take any byte
    (0..255, the reference's sum / set arithmetic on them)."""
    if isinstance(x, str):
        x = [int(c) for c in x]
    if isinstance(x, torch.Tensor):
        t = x
    else:
        a = np.asarray(x)
        if a.dtype == object:
            raise ValueError("ragged board")
        if a.size and (a.min() < 0 or a.max() > max_value):
            raise ValueError(f"board cells must be integers 0..{max_value}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))
    if t.numel() % 81 != 0:
        raise ValueError(f"board data of {t.numel()} cells is not a multiple of 81")
    t = t.reshape(-1, 81)
    if t.dtype != torch.uint8:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > max_value):
            raise ValueError(f"board cells must be integers 0..{max_value}")
        t = t.to(torch.uint8)
    if device is not None:
        t = t.to(device, non_blocking=True)
    return t.contiguous()


# Launches in flight and waves per SIMD in each launch's grid
# (solve_inflight's defaults).  A full grid (4 waves per SIMD) leaves a
# launch's drain to the next launch only as its waves exit; smaller grids
# keep several launches resident together.  Each launch in flight has its
# own stream, and streams beyond the process's hardware queues
# ($GPU_MAX_HW_QUEUES, HIP's default 4) share one and serialise: with 8 or
# more queues six launches at 1 wave per SIMD (four resident, two queued),
# else three at 2 (585-593 against 534-537 M boards/s).
GRID_WAVES_INFLIGHT = 2


def default_inflight():
    """(launches in flight, grid waves per SIMD) for this process's hardware
    queue count."""
    try:
        hwq = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        hwq = 4
    return (6, 1) if hwq >= 8 else (3, GRID_WAVES_INFLIGHT)


def pipelined_launches(n_launches: int, inflight: int, pool_last: Optional[int] = None):
    """solve_inflight's per-launch SDK_GRID_PIPELINED flags: every launch
    but the last `pool_last` (default: half the launches in flight, rounded
    up; with one in flight none -- nothing can take a drained launch's
    slots, so each shares its tail through the XCD pool)."""
    if pool_last is None:
        last = n_launches if inflight == 1 else (inflight + 1) // 2
    else:
        last = max(0, pool_last)
    return [i < n_launches - last for i in range(n_launches)]


def _grid_arg(grid_waves: int, pipelined: bool) -> int:
    """sdk_solve_batch_grid / sdk_solve_batches' grid argument: waves per
    SIMD, | SDK_GRID_PIPELINED for a launch with another queued behind it."""
    g = int(grid_waves)
    if g >= _lib.SDK_GRID_PIPELINED:
        raise ValueError("grid_waves must be below 65536")
    return g | (_lib.SDK_GRID_PIPELINED if pipelined and g >= 0 else 0)  # (negative: the library's -2)


class BatchSolver:
    """One per device.  Holds the device workspace of the C ABI.

    Thread-safe: the workspace is single-stream (include/sudoku_hip.h), so
    every call that uses it (solve, stats) runs under one lock, and a call on
    a different stream than the previous one first makes its stream wait for
    the previous stream's work."""

    def __init__(self, device=None):
        self.device = _require_gpu(device)
        self.lib = _lib.load()
        self._lock = threading.Lock()
        self._last_stream = None
        # held by callers that need solve + stats as one step (node.py's backend)
        self.op_lock = threading.RLock()
        self._pool = None  # the solver's streams (_stream_pool)
        self._slots = None  # solve_inflight's (solver, stream) slots (_slot_solvers)
        self._pool_lock = threading.Lock()  # builds _pool / _slots once across threads
        self._count_scratch = None  # count_solutions' scratch, grown on demand (under self._lock)
        self._canon_scratch = None  # canonical's scratch, likewise
        self._rate_scratch = None  # rate's scratch, likewise
        self._logic_scratch = None  # logic's scratch, likewise
        self._path_scratch = None  # path's scratch, likewise
        self._cand_scratch = None  # candidates' scratch, likewise
        self._min_scratch = None  # minimize's scratch, likewise
        self._sample_scratch = None  # sample's scratch, likewise
        self._uniq_scratch = None  # unique_candidates' scratch, likewise
        self._exact_scratch = None  # count_exact's scratch, likewise
        self._backdoor_scratch = None  # backdoors' scratch, likewise
        self._ua_scratch = None  # unavoidable's scratch, likewise
        self._hit_scratch = None  # hitting_sets' scratch, likewise
        with torch.cuda.device(self.device):
            self.workspace = torch.zeros(int(self.lib.sdk_workspace_bytes()), dtype=torch.uint8,
                                         device=self.device)

    # ------------------------------------------------------------ helpers
    def _stream(self, stream) -> int:
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return int(s.cuda_stream)

    def _ws_stream(self, stream) -> int:
        """Stream handle for a workspace call (caller holds self._lock)."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self._last_stream is not None and self._last_stream != s:
            ev = torch.cuda.Event()
            ev.record(self._last_stream)
            s.wait_event(ev)
        self._last_stream = s
        return int(s.cuda_stream)

    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()

    def _scratch(self, attr: str, need: int) -> torch.Tensor:
        """The cached scratch tensor `attr`, grown to `need` bytes (caller
        holds self._lock)."""
        sc = getattr(self, attr)
        if sc is None or sc.numel() < need:
            if sc is not None and self._last_stream is not None:
                sc.record_stream(self._last_stream)  # a call may still be running on it
            sc = torch.empty(max(need, 64), dtype=torch.uint8, device=self.device)
            setattr(self, attr, sc)
        return sc

    @staticmethod
    def _rc_only(rc: int, what: str) -> None:
        """Raise for an entry that reports by return code only (it does not
        set sdk_last_error)."""
        if rc != 0:
            raise SudokuHipError(f"{what} failed ({rc}): " + ("HIP error" if rc == -1 else "bad arguments"))

    # -------------------------------------------------------------- solve
    def solve(self, puzzles, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
              ordered: bool = False, order="gen", stream=None, grid_waves: int = 0, pipelined: bool = False
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Solve every board with the reference walk `order` ("gen":
        gen.py:6-28, "node": node.py:62-74).  Asynchronous on the stream;
        returns (solutions uint8 (n,81), status int32 (n,)).  grid_waves > 0
        caps the lane-per-board kernel's grid at that many waves per SIMD
        (sdk_solve_batch_grid; solve_inflight's co-resident launches).
        pipelined: another launch follows on the device (SDK_GRID_PIPELINED:
        drained waves exit instead of sharing the last boards); results never
        depend on it."""
        p = self._dev(as_boards(puzzles))
        n = p.shape[0]
        if out is None:
            out = torch.empty_like(p)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        if out.shape != p.shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous (n, 81) uint8 tensor")
        if status.shape != (n,) or status.dtype != torch.int32:
            raise ValueError("status must be an (n,) int32 tensor")
        with self._lock, torch.cuda.device(self.device):
            rc = self.lib.sdk_solve_batch_grid(p.data_ptr(), out.data_ptr(), status.data_ptr(), n,
                                               self.workspace.data_ptr(), _lib.order_code(order),
                                               1 if ordered else 0, self._ws_stream(stream),
                                               _grid_arg(grid_waves, pipelined))
        _lib.check(rc, "sdk_solve_batch_grid")
        return out, status

    # -------------------------------------------------------------- count
    def count_solutions(self, puzzles, limit: int = 2, return_first: bool = False, stream=None, max_waves: int = 0):
        """counts[i] = min(limit, completions of board i that are valid Sudoku
        grids) as an int32 (n,) tensor (sdk_count_solutions_batch; library
        extension, no reference counterpart).  1 <= limit <= 1024.  A board
        whose givens repeat a digit in a unit counts 0 -- unlike solve(), whose
        walk never tests the givens; a byte > 9 gives SDK_INVALID (-1).
        return_first: also an (n, 81) tensor with a completion of every board
        that has one (the unique one when the count at limit >= 2 is 1) and
        the input board otherwise.  max_waves > 0 caps the kernel's grid;
        results never depend on it.  Asynchronous on the stream; one cached
        scratch tensor serves every call, ordered like the workspace's."""
        limit = int(limit)
        if not 1 <= limit <= SDK_COUNT_MAX_LIMIT:
            raise ValueError(f"limit must be 1..{SDK_COUNT_MAX_LIMIT}")
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = self._dev(as_boards(puzzles, max_value=255))
        n = p.shape[0]
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        first = torch.empty_like(p) if return_first else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_count_scratch", int(self.lib.sdk_count_scratch_bytes(n, int(max_waves))))
            rc = self.lib.sdk_count_solutions_batch(p.data_ptr(), counts.data_ptr(),
                                                    first.data_ptr() if return_first else None, n, limit,
                                                    sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_count_solutions_batch")
        return (counts, first) if return_first else counts

    # -------------------------------------------------------- exact count
    def count_exact(self, boards, slice=None, max_rounds=None, max_tasks: int = 0, max_waves: int = 0, stream=None,
                    return_status: bool = False, return_stats: bool = False):
        """The exact number of completions of every board as an int64 (n,)
        tensor, without a cap (sdk_count_exact_batch; library extension, no
        reference counterpart).  A board's search tree is cut
        into tasks on the GPU and shared over every lane, so one heavy board
        uses the whole device.  Givens that repeat a digit in a unit count 0.
        The call runs rounds of about `slice` passes a lane (default
        EXACT_SLICE), at most max_rounds of them (default EXACT_MAX_ROUNDS); a
        board still open then is SDK_EXACT_PARTIAL and its count a lower bound
        (not reproducible).  Raises if any board is SDK_EXACT_PARTIAL or
        SDK_FAULT, unless return_status asks for the int32 (n,) statuses: then
        (counts, status) comes back and nothing is raised.  A byte > 9 counts
        0 with status SDK_INVALID.  return_stats adds a dict (rounds, donated, parks,
        max_passes) as the last element.  max_tasks: the capacity of each task
        list (0: four tasks a lane); max_waves > 0 caps the grid; an exact
        count never depends on any of the knobs.  SYNCHRONOUS on the stream;
        one cached scratch tensor serves every call, ordered like the
        workspace's."""
        slice = EXACT_SLICE if slice is None else int(slice)
        max_rounds = EXACT_MAX_ROUNDS if max_rounds is None else int(max_rounds)
        if slice < 1 or max_rounds < 1:
            raise ValueError("slice and max_rounds must be >= 1")
        if int(max_waves) < 0 or int(max_tasks) < 0:
            raise ValueError("max_waves and max_tasks must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        counts = torch.empty(n, dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        st = (ctypes.c_int64 * 4)()
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_exact_scratch",
                               int(self.lib.sdk_count_exact_scratch_bytes(n, int(max_waves), int(max_tasks))))
            rc = self.lib.sdk_count_exact_batch(p.data_ptr(), counts.data_ptr(), status.data_ptr(), n, slice, max_rounds,
                                                int(max_tasks), sc.data_ptr(), sc.numel(), int(max_waves),
                                                self._ws_stream(stream), st)
        self._rc_only(rc, "sdk_count_exact_batch")
        if not return_status and n:
            bad = (status == _lib.SDK_EXACT_PARTIAL) | (status == _lib.SDK_FAULT)
            if bool(bad.any().item()):
                raise SudokuHipError(f"count_exact: {int(bad.sum().item())} of {n} boards without an exact count after "
                                     f"{int(st[0])} rounds (return_status=True gives the statuses and lower bounds)")
        out = (counts, status) if return_status else (counts,)
        if return_stats:
            out += (dict(zip(("rounds", "donated", "parks", "max_passes"), (int(v) for v in st))),)
        return out[0] if len(out) == 1 else out

    # -------------------------------------------------- completion list
    def completions(self, boards, capacity=None, limit: int = 0, sort: bool = True, return_status: bool = False,
                    slice=None, max_rounds=None, max_tasks: int = 0, max_waves: int = 0, stream=None):
        """Every completion of every board (sdk_enumerate_batch; library
        extension, no reference counterpart) in CSR form:
        (grids (m, 81) uint8, offsets (n + 1,) int64), board i's completions
        being grids[offsets[i]:offsets[i + 1]].  A completion is what
        count_solutions counts; the search is count_exact's, shared over the
        whole grid, with the same slice / max_rounds / max_tasks / max_waves.
        sort=True (the default): rows ordered by board, then lexicographically
        by their 81 bytes, so the result is reproducible bit for bit (torch
        sorts on the device); sort=False only groups the rows by board, in an
        order that differs from run to run.  limit > 0: at most `limit`
        completions of a board are listed and the rest of its search is
        dropped (status SDK_ENUM_LIMITED, which of them is unspecified).
        capacity: rows of the list, default n * limit, or 2^20 without a
        limit.  Without return_status an overflow raises SudokuHipError with
        the number of rows needed in its message (retry with that capacity),
        and so does a board left SDK_ENUM_PARTIAL or SDK_FAULT; with it,
        (grids, offsets, count int64 (n,), status int32 (n,), info dict) come
        back, grids holding only the rows actually listed (info["listed"] of
        info["total"]) and rows of SDK_FAULT boards left out.  SYNCHRONOUS on
        the stream; count_exact's cached scratch serves the call."""
        slice = EXACT_SLICE if slice is None else int(slice)
        max_rounds = EXACT_MAX_ROUNDS if max_rounds is None else int(max_rounds)
        limit = int(limit)
        if slice < 1 or max_rounds < 1:
            raise ValueError("slice and max_rounds must be >= 1")
        if int(max_waves) < 0 or int(max_tasks) < 0 or limit < 0:
            raise ValueError("max_waves, max_tasks and limit must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        capacity = (n * limit if limit else 1 << 20) if capacity is None else int(capacity)
        if not 0 <= capacity <= _lib.SDK_ENUM_MAX_ROWS:
            raise ValueError(f"capacity must be 0..{_lib.SDK_ENUM_MAX_ROWS}")
        grids = torch.empty((capacity, 81), dtype=torch.uint8, device=self.device)
        owner = torch.empty(capacity, dtype=torch.int32, device=self.device)
        counts = torch.empty(n, dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        st = (ctypes.c_int64 * 6)()
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_exact_scratch",
                               int(self.lib.sdk_enumerate_scratch_bytes(n, int(max_waves), int(max_tasks))))
            rc = self.lib.sdk_enumerate_batch(p.data_ptr(), n, grids.data_ptr() if capacity else None,
                                              owner.data_ptr() if capacity else None, capacity, limit,
                                              counts.data_ptr(), status.data_ptr(), slice, max_rounds, int(max_tasks),
                                              sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream), st)
        self._rc_only(rc, "sdk_enumerate_batch")
        info = dict(zip(("rounds", "donated", "parks", "max_passes", "total", "listed"), (int(v) for v in st)))
        if not return_status and n:
            if info["listed"] < info["total"]:
                raise SudokuHipError(f"completions: the list overflowed, {info['total']} rows asked for a slot and the "
                                     f"capacity is {capacity} (call again with capacity={info['total']})")
            bad = (status == _lib.SDK_ENUM_PARTIAL) | (status == _lib.SDK_FAULT)
            if bool(bad.any().item()):
                raise SudokuHipError(f"completions: {int(bad.sum().item())} of {n} boards without a complete list "
                                     f"after {info['rounds']} rounds (return_status=True gives the statuses)")
        m = info["listed"]
        with torch.cuda.device(self.device):
            g, o = grids[:m], owner[:m].to(torch.int64)
            if n and m and bool((status == _lib.SDK_FAULT).any().item()):
                keep = status[o] != _lib.SDK_FAULT
                g, o = g[keep], o[keep]
            order = None
            if sort and g.shape[0] > 1:
                # 81 digits of 4 bits in six int64 keys of 15 digits; stable sorts, the last key first
                shifts = torch.arange(14, -1, -1, device=self.device, dtype=torch.int64) * 4
                order = torch.arange(g.shape[0], device=self.device)
                for k in range(5, -1, -1):
                    part = g[:, 15 * k:15 * k + 15].to(torch.int64)
                    key = (part << shifts[:part.shape[1]]).sum(dim=1)
                    order = order[torch.sort(key[order], stable=True)[1]]
            by = torch.sort(o if order is None else o[order], stable=True)[1]
            order = by if order is None else order[by]
            g = g[order].contiguous()
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            if n:
                offsets[1:] = torch.cumsum(torch.bincount(o, minlength=n), dim=0)
        if return_status:
            return g, offsets, counts, status, info
        return g, offsets

    # ---------------------------------------------------------- canonical
    def canonical(self, boards, return_sym: bool = False, return_autos: bool = False, slices: int = 0, stream=None):
        """The canonical (minlex) form of every board under Sudoku's
        symmetries -- transposition, band / stack permutations, row / column
        permutations inside them, digit relabelling -- as an (n, 81) uint8
        tensor (sdk_canonical_batch; library extension, no reference
        counterpart; the definition is in include/sudoku_hip.h).  Two boards
        are the same puzzle under the symmetries exactly when their canonical
        forms are equal.  Any bytes 0..9 count as a board, valid or not.
        return_sym: also an int32 (n,) tensor, the smallest symmetry number
        whose image the form is (gen.apply_symmetry applies it);
        return_autos: also int32 (n,), how many of the 3 359 232 symmetries
        give it.  A board with a byte > 9 comes back as it is with
        SDK_INVALID (-1) in both.  slices cuts each board's search into that
        many workgroups (0: enough for a small batch to fill the device);
        results never depend on it.  Asynchronous on the stream; one cached
        scratch tensor serves every call, ordered like the workspace's."""
        slices = int(slices)
        if not 0 <= slices <= _lib.SDK_CANON_MAX_SLICES:
            raise ValueError(f"slices must be 0 (auto) or 1..{_lib.SDK_CANON_MAX_SLICES}")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        canon = torch.empty_like(p)
        sym = torch.empty(n, dtype=torch.int32, device=self.device)
        autos = torch.empty(n, dtype=torch.int32, device=self.device) if return_autos else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_canon_scratch", int(self.lib.sdk_canonical_scratch_bytes(n, slices)))
            rc = self.lib.sdk_canonical_batch(p.data_ptr(), canon.data_ptr(), sym.data_ptr(),
                                              autos.data_ptr() if return_autos else None, n, slices,
                                              sc.data_ptr(), sc.numel(), self._ws_stream(stream))
        self._rc_only(rc, "sdk_canonical_batch")
        out = (canon,) + ((sym,) if return_sym else ()) + ((autos,) if return_autos else ())
        return out if len(out) > 1 else canon

    # --------------------------------------------------------------- rate
    def rate(self, boards, max_level: int = 4, return_open: bool = False, return_marks: bool = False, stream=None):
        """How much logic every puzzle needs, as an int32 (n,) tensor
        (sdk_rate_batch; library extension, no reference counterpart; the
        definition is in include/sudoku_hip.h and DESIGN.md §14): the lowest
        level whose rules solve the board -- 1 naked singles, 2 with hidden
        singles, 3 with locked candidates, 4 with one level of trial
        eliminations -- 0 when the rules prove that it has no completion,
        max_level + 1 when max_level does not decide it.  The rating does not
        depend on any search order and is the same for every symmetry image
        of a board.  return_open: also an int32 (n, 4) tensor, per level the
        cells left without exactly one candidate (0 from the solving level
        on, -1 where the level's closure is dead, SDK_RATE_NOT_RUN (-2) above
        max_level); return_marks: also an int16 (n, 81) tensor, per cell the
        candidates the deepest closure computed leaves (bit d-1 for digit d;
        the completion as single bits when solved, zero when dead).  A byte
        > 9 gives SDK_INVALID (-1) in the rating and the open counts.
        Asynchronous on the stream; one cached scratch tensor serves every
        call, ordered like the workspace's."""
        max_level = int(max_level)
        if not 1 <= max_level <= _lib.SDK_RATE_MAX_LEVEL:
            raise ValueError(f"max_level must be 1..{_lib.SDK_RATE_MAX_LEVEL}")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        rating = torch.empty(n, dtype=torch.int32, device=self.device)
        opens = torch.empty((n, 4), dtype=torch.int32, device=self.device) if return_open else None
        marks = torch.empty((n, 81), dtype=torch.int16, device=self.device) if return_marks else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_rate_scratch", int(self.lib.sdk_rate_scratch_bytes(n, max_level)))
            rc = self.lib.sdk_rate_batch(p.data_ptr(), rating.data_ptr(), opens.data_ptr() if return_open else None,
                                         marks.data_ptr() if return_marks else None, n, max_level,
                                         sc.data_ptr(), sc.numel(), self._ws_stream(stream))
        self._rc_only(rc, "sdk_rate_batch")
        out = (rating,) + ((opens,) if return_open else ()) + ((marks,) if return_marks else ())
        return out if len(out) > 1 else rating

    # -------------------------------------------------------------- logic
    def logic(self, boards=None, ladder=None, start=None, return_open: bool = False, return_left: bool = False,
              return_marks: bool = False, stream=None):
        """Which named technique every state falls to, as an int32 (n,)
        tensor (sdk_logic_batch; library extension, no reference counterpart;
        the definition is in include/sudoku_hip.h and DESIGN.md §26).  ladder:
        1..8 rule sets (masks of N, H, L, S2, S3, S4, F2, F3, F4 below), each
        with N and a proper superset of the one before; None is
        DEFAULT_LADDER -- singles, hidden singles, locked candidates, pairs,
        triples / quads, X-wing, swordfish / jellyfish.  The answer is the
        first step (1-based) whose rules solve the state, 0 when some step
        proves that it has no completion, len(ladder) + 1 when the ladder
        does not decide it; it depends on no order of the rules and is the
        same for every symmetry image.  start: pencil marks, (n, 81) int16
        masks (bit d-1 for digit d) ANDed into the boards' start states;
        boards None: empty boards under `start`.  return_open / return_left:
        also int32 (n, 8) tensors, per step the cells without exactly one
        candidate and the candidates left in all (0 and 81 from the solving
        step on, -1 from the dead step on, SDK_LOGIC_NOT_RUN (-2) past the
        ladder's end); return_marks: also an int16 (n, 81) tensor, the
        candidates the deepest closure computed leaves (zero when dead).  A
        byte > 9 or a mark above 0x1FF gives SDK_INVALID (-1) in the step
        and the counts.  Asynchronous on the stream; one cached scratch
        tensor serves every call, ordered like the workspace's."""
        lad = [int(m) for m in (DEFAULT_LADDER if ladder is None else ladder)]
        if not 1 <= len(lad) <= _lib.SDK_LOGIC_MAX_STEPS:
            raise ValueError(f"a ladder has 1..{_lib.SDK_LOGIC_MAX_STEPS} steps")
        for prev, m in zip([0] + lad, lad):
            if m & ~0x1FF or not m & N or m == prev or m & prev != prev:
                raise ValueError("every step of a ladder is a mask inside 0x1FF with N and a proper superset of the step before")
        if boards is None and start is None:
            raise ValueError("logic needs boards, start or both")
        p = self._dev(as_boards(boards, max_value=255)) if boards is not None else None
        s = None
        if start is not None:
            s = torch.as_tensor(start)
            if s.dtype not in (torch.int16, torch.uint16):
                s = s.to(torch.int16)
            s = self._dev(s.reshape(-1, 81))
        n = p.shape[0] if p is not None else s.shape[0]
        if p is not None and s is not None and s.shape[0] != n:
            raise ValueError("boards and start differ in length")
        step = torch.empty(n, dtype=torch.int32, device=self.device)
        opens = torch.empty((n, 8), dtype=torch.int32, device=self.device) if return_open else None
        left = torch.empty((n, 8), dtype=torch.int32, device=self.device) if return_left else None
        marks = torch.empty((n, 81), dtype=torch.int16, device=self.device) if return_marks else None
        host_ladder = (ctypes.c_uint32 * len(lad))(*lad)
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_logic_scratch", int(self.lib.sdk_logic_scratch_bytes(n, len(lad))))
            rc = self.lib.sdk_logic_batch(p.data_ptr() if p is not None else None, s.data_ptr() if s is not None else None,
                                          ctypes.addressof(host_ladder), len(lad), step.data_ptr(),
                                          opens.data_ptr() if return_open else None, left.data_ptr() if return_left else None,
                                          marks.data_ptr() if return_marks else None, n, sc.data_ptr(), sc.numel(),
                                          self._ws_stream(stream))
        self._rc_only(rc, "sdk_logic_batch")
        out = (step,) + ((opens,) if return_open else ()) + ((left,) if return_left else ()) + ((marks,) if return_marks else ())
        return out if len(out) > 1 else step

    # ------------------------------------------------------- solving path
    def path(self, boards=None, rules: int = 0x1FF, start=None, max_rounds: int = 0, capacity=None,
             return_marks: bool = False, return_hist: bool = False, stream=None, max_waves: int = 0):
        """Every deduction of every state, round by round (sdk_path_batch;
        library extension, no reference counterpart; the definition is in
        include/sudoku_hip.h and DESIGN.md §27) in CSR form: (events, offsets
        (n + 1,) int64, status (n,) int32), state i's events being
        events[offsets[i]:offsets[i + 1]].  rules: one mask of N .. F4 that
        holds N; its bit indices are the classes 0 N, 1 H, 2 L, 3 S2, 4 S3,
        5 S4, 6 F2, 7 F3, 8 F4.  Every round fires all effective deductions
        of the easiest class that has one, on the round's start state, so the
        path is deterministic, the same for every symmetry image and ends in
        logic's fixpoint of `rules`.  events is an int32 (m, 8) tensor, the
        columns PATH_COLUMNS: round, cls, m, I, u, removed, left,
        contradiction -- (m, I, u) the matrix, the row mask and the union of
        a Hall firing, or m = 72 + dir, I = 1 << (d - 1), u = line | box << 5
        of a locked-candidates firing; removed the candidates the event takes
        away, left those the state keeps after the event's round; a dead
        state ends in one contradiction event (removed 0, left the count
        before).  Events are sorted by (state, round, m, I, u): the result is
        reproducible bit for bit.  status: SDK_PATH_DEAD 0, SDK_PATH_SOLVED 1,
        SDK_PATH_STUCK 2 (no rule of the mask applies), SDK_PATH_LIMITED 3
        (max_rounds > 0 rounds are done), SDK_INVALID for a byte > 9 or a
        mark above 0x1FF (no events).  boards / start: logic's.  capacity:
        rows of the raw list; None counts first and lists at the exact size,
        an explicit one that overflows raises SudokuHipError with the number
        to ask for; capacity=0 is a pure count (no events, all offsets 0).
        return_marks: also the end states, int16 (n, 81), zero when dead;
        return_hist: also int32 (n, 9), the events per class, contradiction
        events not counted.  max_waves > 0 caps the kernel's
        grid; results never depend on it.  SYNCHRONOUS on the stream (the
        list's length comes back to the host); one cached scratch tensor
        serves every call, ordered like the workspace's."""
        rules, max_rounds = int(rules), int(max_rounds)
        if rules & ~0x1FF or not rules & N:
            raise ValueError("rules is a mask inside 0x1FF with N")
        if max_rounds < 0 or int(max_waves) < 0:
            raise ValueError("max_rounds and max_waves must be >= 0")
        if capacity is not None and int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        if boards is None and start is None:
            raise ValueError("path needs boards, start or both")
        p = self._dev(as_boards(boards, max_value=255)) if boards is not None else None
        s = None
        if start is not None:
            s = torch.as_tensor(start)
            if s.dtype not in (torch.int16, torch.uint16):
                s = s.to(torch.int16)
            s = self._dev(s.reshape(-1, 81))
        n = p.shape[0] if p is not None else s.shape[0]
        if p is not None and s is not None and s.shape[0] != n:
            raise ValueError("boards and start differ in length")
        ctx = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        with torch.cuda.device(self.device), ctx():
            count = torch.zeros(n, dtype=torch.int32, device=self.device)
            rounds = torch.zeros(n, dtype=torch.int32, device=self.device)
            status = torch.zeros(n, dtype=torch.int32, device=self.device)
            hist = torch.zeros((n, 9), dtype=torch.int32, device=self.device) if return_hist else None
            marks = torch.zeros((n, 81), dtype=torch.int16, device=self.device) if return_marks else None
            info = torch.zeros(2, dtype=torch.int64, device=self.device)
            cap = 0 if capacity is None else int(capacity)
            listed = 0
            rows = torch.empty((0, 4), dtype=torch.int32, device=self.device)
            for attempt in range(2 if n else 0):
                rows = torch.empty((cap, 4), dtype=torch.int32, device=self.device)
                with self._lock:
                    sc = self._scratch("_path_scratch", int(self.lib.sdk_path_scratch_bytes(n, int(max_waves))))
                    rc = self.lib.sdk_path_batch(p.data_ptr() if p is not None else None,
                                                 s.data_ptr() if s is not None else None, rules, max_rounds, n,
                                                 rows.data_ptr() if cap else None, cap, count.data_ptr(), rounds.data_ptr(),
                                                 status.data_ptr(), hist.data_ptr() if return_hist else None,
                                                 marks.data_ptr() if return_marks else None, info.data_ptr(), sc.data_ptr(),
                                                 sc.numel(), int(max_waves), self._ws_stream(stream))
                self._rc_only(rc, "sdk_path_batch")
                total, listed = (int(v) for v in info.tolist())
                if listed == total:
                    break
                if capacity is not None and cap == 0:
                    break  # a pure count
                if capacity is not None:
                    raise SudokuHipError(f"path: the list overflowed, {total} rows asked for a slot and the capacity is "
                                         f"{cap} (call again with capacity={total})")
                cap = total
            w = rows[:listed].to(torch.int64) & 0xFFFFFFFF
            owner, w1, w2, left = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
            rnd, m, row_mask, union = w1 & 0xFFFF, w2 & 0xFF, (w2 >> 8) & 0x1FF, (w2 >> 17) & 0x7FFF
            if listed:
                order = torch.sort((m << 24) | (row_mask << 15) | union, stable=True)[1]
                order = order[torch.sort(((owner << 16) | rnd)[order], stable=True)[1]]
            else:
                order = torch.zeros(0, dtype=torch.int64, device=self.device)
            events = torch.stack([rnd, (w1 >> 16) & 15, m, row_mask, union, (w1 >> 24) & 0xFF, left, (w1 >> 20) & 1],
                                 dim=1)[order].to(torch.int32)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            if listed:  # (a pure count lists nothing: the offsets stay zero)
                offsets[1:] = torch.cumsum(count.to(torch.int64), dim=0)
        out = (events, offsets, status) + ((marks,) if return_marks else ()) + ((hist,) if return_hist else ())
        return out

    # ---------------------------------------------------- unavoidable sets
    @staticmethod
    def _rev32(x: torch.Tensor) -> torch.Tensor:
        """Bit-reversal of 32-bit values held in int64."""
        x = ((x >> 1) & 0x55555555) | ((x & 0x55555555) << 1)
        x = ((x >> 2) & 0x33333333) | ((x & 0x33333333) << 2)
        x = ((x >> 4) & 0x0F0F0F0F) | ((x & 0x0F0F0F0F) << 4)
        x = ((x >> 8) & 0x00FF00FF) | ((x & 0x00FF00FF) << 8)
        return ((x >> 16) & 0xFFFF) | ((x & 0xFFFF) << 16)

    def unavoidable(self, grids, max_size: int = 12, minimal: bool = True, packed: bool = False, capacity=None,
                    return_status: bool = False, stream=None, max_waves: int = 0):
        """The unavoidable sets of every solution grid (sdk_unavoidable_batch
        and sdk_unavoidable_minimal_batch; library extension, no reference
        counterpart; the definitions are in include/sudoku_hip.h and DESIGN.md
        §24) in CSR form: (sets, offsets (n + 1,) int64), grid i's sets being
        sets[offsets[i]:offsets[i + 1]].  An unavoidable set of a grid g is a
        set of cells inside which some other valid grid differs from g: every
        puzzle with the one solution g has a given in each.  Listed are the
        cell sets of the connected neighbours of at most max_size cells
        (4 <= max_size <= SDK_UA_MAX_SIZE), each once; minimal=True (the
        default) keeps those with no proper subset among them, which are
        exactly the minimal unavoidable sets of at most max_size cells.  sets
        is a uint8 (R, 81) 0/1 tensor, or with packed=True int32 (R, 3), cell
        c bit c & 31 of word c >> 5.  Rows are ordered by grid, then size, then
        their ascending cell lists compared lexicographically: the result is
        reproducible bit for bit (torch sorts on the device).  capacity: rows
        of the raw list; None starts from UA_CAPACITY[max_size] a grid and
        asks once more with the exact number when that overflows, an explicit
        one that overflows raises SudokuHipError with the number to ask for.
        A grid with a byte outside 1..9 (SDK_INVALID) or a digit twice in a
        unit (SDK_UA_NOT_A_GRID) raises, unless return_status asks for the
        int32 (n,) statuses: then (sets, offsets, status) comes back and such
        a grid has no set.  max_waves > 0 caps the kernels' grids; results
        never depend on it.  SYNCHRONOUS on the stream (the list's length
        comes back to the host); one cached scratch tensor serves every call,
        ordered like the workspace's."""
        max_size = int(max_size)
        if not 4 <= max_size <= _lib.SDK_UA_MAX_SIZE:
            raise ValueError(f"max_size must be 4..{_lib.SDK_UA_MAX_SIZE}")
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        if capacity is not None and int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        g = self._dev(as_boards(grids, max_value=255))
        n = g.shape[0]
        ctx = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        cap = n * UA_CAPACITY[max_size] if capacity is None else int(capacity)
        with torch.cuda.device(self.device), ctx():
            count = torch.empty(n, dtype=torch.int32, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            info = torch.zeros(2, dtype=torch.int64, device=self.device)
            for attempt in range(2):
                rows = torch.empty((cap, 4), dtype=torch.int32, device=self.device)
                with self._lock:
                    sc = self._scratch("_ua_scratch", int(self.lib.sdk_unavoidable_scratch_bytes(n, int(max_waves))))
                    rc = self.lib.sdk_unavoidable_batch(g.data_ptr(), n, max_size, rows.data_ptr() if cap else None, cap,
                                                        count.data_ptr(), status.data_ptr(), info.data_ptr(),
                                                        sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream))
                self._rc_only(rc, "sdk_unavoidable_batch")
                total, listed = (int(v) for v in info.tolist())
                if listed == total:
                    break
                if capacity is not None:
                    raise SudokuHipError(f"unavoidable: the list overflowed, {total} rows asked for a slot and the "
                                         f"capacity is {cap} (call again with capacity={total})")
                cap = total
            if not return_status and n and bool((status != _lib.SDK_UA_DONE).any().item()):
                raise SudokuHipError(f"unavoidable: {int((status != _lib.SDK_UA_DONE).sum().item())} of {n} inputs are "
                                     f"no valid grids (return_status=True gives the statuses)")
            # one sort for order and duplicates: rows of (grid, size, the three words bit-reversed and negated, so
            # that the set holding the lowest cell two sets differ in comes first) compared lexicographically
            w = rows[:listed].to(torch.int64) & 0xFFFFFFFF
            size = torch.zeros(listed, dtype=torch.int64, device=self.device)
            for k in range(3):
                x = w[:, k]
                x = x - ((x >> 1) & 0x55555555)
                x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
                x = (x + (x >> 4)) & 0x0F0F0F0F
                size += (x * 0x01010101 >> 24) & 0xFF
            keys = torch.stack([w[:, 3], size] + [0xFFFFFFFF - self._rev32(w[:, k]) for k in range(3)], dim=1)
            if listed:
                keys = torch.unique(keys, dim=0)
            owner = keys[:, 0]
            words = torch.stack([self._rev32(0xFFFFFFFF - keys[:, 2 + k]) for k in range(3)], dim=1)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            if n:
                offsets[1:] = torch.cumsum(torch.bincount(owner, minlength=n), dim=0)
            if minimal and keys.shape[0]:
                raw = torch.cat([words, owner[:, None]], dim=1).to(torch.int32).contiguous()
                keep = torch.empty(raw.shape[0], dtype=torch.uint8, device=self.device)
                rc = self.lib.sdk_unavoidable_minimal_batch(raw.data_ptr(), offsets.data_ptr(), n, keep.data_ptr(),
                                                            int(max_waves), self._stream(stream))
                self._rc_only(rc, "sdk_unavoidable_minimal_batch")
                keep = keep.bool()
                words, owner = words[keep], owner[keep]
                offsets[1:] = torch.cumsum(torch.bincount(owner, minlength=n), dim=0)
            if packed:
                sets = words.to(torch.int32).contiguous()
            else:
                cells = torch.arange(81, device=self.device)
                sets = ((words[:, cells >> 5] >> (cells & 31)) & 1).to(torch.uint8)
        return (sets, offsets, status) if return_status else (sets, offsets)

    # -------------------------------------------------------- hitting sets
    def _cell_masks(self, x, n: int, what: str, default: int) -> torch.Tensor:
        """An allowed / required argument as the C ABI's (n, 4) int32 words:
        None (every family `default`, an 81-bit int), one mask for all or one
        a family, as (81,) / (n, 81) 0/1 values or packed (3 or 4 words)."""
        if x is None:
            x = torch.tensor([default & 0xFFFFFFFF, (default >> 32) & 0xFFFFFFFF, default >> 64], dtype=torch.int64)
        x = self._dev(torch.as_tensor(x))
        if x.dim() == 1:
            x = x.unsqueeze(0).expand(n, -1)
        if x.dim() != 2 or x.shape[0] != n or x.shape[1] not in (81, 3, 4):
            raise ValueError(f"{what} must be (n, 81) cells or packed (n, 3) words, or one row for every family")
        if x.shape[1] == 81:
            cells = torch.arange(81, device=self.device)
            bits = (x != 0).to(torch.int64) << (cells & 31)
            x = torch.stack([bits[:, (cells >> 5) == w].sum(dim=1) for w in range(3)], dim=1)
        x = x.to(torch.int64) & 0xFFFFFFFF
        out = torch.zeros((n, 4), dtype=torch.int64, device=self.device)
        out[:, :3] = x[:, :3]
        return (out - ((out >> 31) << 32)).to(torch.int32).contiguous()

    def hitting_sets(self, sets, offsets, k: int, allowed=None, required=None, limit: int = 0, packed: bool = False,
                     capacity=None, return_status: bool = False, return_count: bool = False, stream=None,
                     max_waves: int = 0):
        """The k-cell hitting sets of every family of cell sets
        (sdk_hitting_sets_batch; library extension, no reference counterpart;
        the definitions are in include/sudoku_hip.h and DESIGN.md §25) in CSR
        form: (rows, offsets (n + 1,) int64).  Family i is
        sets[offsets[i]:offsets[i + 1]] -- (S, 81) 0/1 or packed (S, 3) / (S,
        4) words, both forms BatchSolver.unavoidable returns -- with allowed[i]
        (None: all 81 cells) and required[i] (None: no cell), each (n, 81),
        packed (n, 3), or one row for all families.  A row is a set S of
        exactly k cells (0 <= k <= SDK_HIT_MAX_CLUES) with required <= S <=
        allowed that meets every set of the family; each is listed once,
        whatever the order of the sets or their repeats.  rows is a uint8 (R,
        81) 0/1 tensor, or with packed=True int32 (R, 3); ordered by family,
        then by their ascending cell lists compared lexicographically.
        limit > 0 stops a family after that many rows (which ones is
        unspecified).  capacity: rows of the raw list; None starts from
        HIT_CAPACITY and asks once more with the exact number when that
        overflows, an explicit one that overflows raises SudokuHipError with
        the number to ask for, except capacity=0, which lists nothing: with
        return_count -- the int64 (n,) rows of every family as a further value
        -- and limit=0 that is a pure count, which never walks free fillings.
        A family whose masks have a bit at or above 81, or required outside
        allowed (SDK_INVALID), raises, unless return_status asks for the int32
        (n,) statuses (SDK_HIT_DONE, SDK_HIT_LIMITED, SDK_INVALID) as a third
        value.  max_waves > 0 caps
        the kernels' grids; results never depend on it.  SYNCHRONOUS on the
        stream; one cached scratch tensor serves every call."""
        k, limit = int(k), int(limit)
        if not 0 <= k <= _lib.SDK_HIT_MAX_CLUES:
            raise ValueError(f"k must be 0..{_lib.SDK_HIT_MAX_CLUES}")
        if limit < 0 or int(max_waves) < 0:
            raise ValueError("limit and max_waves must be >= 0")
        if capacity is not None and int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        ctx = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        with torch.cuda.device(self.device), ctx():
            offsets = self._dev(torch.as_tensor(offsets)).to(torch.int64).contiguous()
            if offsets.dim() != 1 or offsets.shape[0] < 1:
                raise ValueError("offsets must hold one entry per family and one more")
            n = offsets.shape[0] - 1
            s = self._dev(torch.as_tensor(sets))
            if s.dim() != 2 or s.shape[1] not in (81, 3, 4):
                raise ValueError("sets must be (S, 81) cells or packed (S, 3) words")
            s = self._cell_masks(s, s.shape[0], "sets", 0) if s.shape[0] else torch.zeros((0, 4), dtype=torch.int32,
                                                                                          device=self.device)
            if n and (int(offsets[0].item()) != 0 or int(offsets[-1].item()) != s.shape[0]):
                raise ValueError("offsets must start at 0 and end at the number of sets")
            A = self._cell_masks(allowed, n, "allowed", (1 << 81) - 1)
            R = self._cell_masks(required, n, "required", 0)
            count = torch.zeros(n, dtype=torch.int64, device=self.device)
            status = torch.zeros(n, dtype=torch.int32, device=self.device)
            info = torch.zeros(2, dtype=torch.int64, device=self.device)
            cap = HIT_CAPACITY if capacity is None else int(capacity)
            for attempt in range(2):
                rows = torch.empty((cap, 4), dtype=torch.int32, device=self.device)
                with self._lock:
                    sc = self._scratch("_hit_scratch", int(self.lib.sdk_hitting_sets_scratch_bytes(n, int(max_waves))))
                    rc = self.lib.sdk_hitting_sets_batch(s.data_ptr() if s.shape[0] else None, offsets.data_ptr(),
                                                         A.data_ptr(), R.data_ptr(), n, k, limit,
                                                         rows.data_ptr() if cap else None, cap, count.data_ptr(),
                                                         status.data_ptr(), info.data_ptr(), sc.data_ptr(), sc.numel(),
                                                         int(max_waves), self._ws_stream(stream))
                self._rc_only(rc, "sdk_hitting_sets_batch")
                total, listed = (int(v) for v in info.tolist())
                if listed == total or cap == 0:
                    break
                if capacity is not None:
                    raise SudokuHipError(f"hitting_sets: the list overflowed, {total} rows asked for a slot and the "
                                         f"capacity is {cap} (call again with capacity={total})")
                cap = total
            if not return_status and n and bool((status == SDK_INVALID).any().item()):
                raise SudokuHipError(f"hitting_sets: {int((status == SDK_INVALID).sum().item())} of {n} families have "
                                     f"masks that are no cell sets (return_status=True gives the statuses)")
            # one sort for the order: rows of (family, the three words bit-reversed and negated, so that the set holding
            # the lowest cell two sets differ in comes first) compared lexicographically
            w = rows[:listed].to(torch.int64) & 0xFFFFFFFF
            keys = torch.stack([w[:, 3]] + [0xFFFFFFFF - self._rev32(w[:, j]) for j in range(3)], dim=1)
            if listed:
                keys = torch.unique(keys, dim=0)
            owner = keys[:, 0]
            words = torch.stack([self._rev32(0xFFFFFFFF - keys[:, 1 + j]) for j in range(3)], dim=1)
            out_offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            if n:
                out_offsets[1:] = torch.cumsum(torch.bincount(owner, minlength=n), dim=0)
            if packed:
                out = (words - ((words >> 31) << 32)).to(torch.int32).contiguous()
            else:
                cells = torch.arange(81, device=self.device)
                out = ((words[:, cells >> 5] >> (cells & 31)) & 1).to(torch.uint8)
        return (out, out_offsets) + ((status,) if return_status else ()) + ((count,) if return_count else ())

    def sub_puzzles(self, grids, k: int, allowed=None, required=None, max_size: int = 12, sets=None, chunk: int = 1 << 18,
                    stream=None, max_waves: int = 0):
        """Every proper puzzle of exactly k clues whose solution is grid i,
        with required[i] <= its clue cells <= allowed[i] (masks as in
        hitting_sets), as (puzzles (R, 81) uint8, offsets (n + 1,) int64),
        ordered by grid and then by ascending clue cells.  A proper puzzle has
        a clue in every unavoidable set of its grid, so the candidates are the
        k-cell hitting sets of the grid's minimal unavoidable sets of at most
        max_size cells (BatchSolver.unavoidable, or `sets` = (sets, offsets)
        already computed for these grids); each candidate becomes a board by
        tensor operations and is kept where count_solutions(limit=2) is 1.
        The answer is exact for every max_size -- the sets only prune.  The
        grids are counted first and listed in groups of at most `chunk`
        candidates (a grid with more has a group to itself), and boards are
        built and verified `chunk` at a time, so memory stays bounded by the
        largest grid's packed candidates; a grid with more than
        SUB_PUZZLES_MAX_ROWS of them raises SudokuHipError."""
        g = self._dev(as_boards(grids, max_value=255))
        n = g.shape[0]
        ctx = (lambda: torch.cuda.stream(stream)) if stream is not None else contextlib.nullcontext
        with torch.cuda.device(self.device), ctx():
            if sets is None:
                sets = self.unavoidable(g, max_size=max_size, packed=True, stream=stream, max_waves=max_waves)
            usets, uoff = self._dev(sets[0]), self._dev(sets[1]).to(torch.int64)
            A = self._cell_masks(allowed, n, "allowed", (1 << 81) - 1)
            R = self._cell_masks(required, n, "required", 0)
            kw = dict(stream=stream, max_waves=max_waves)
            count = self.hitting_sets(usets, uoff, k, allowed=A, required=R, capacity=0, return_count=True, **kw)[2].tolist()
            if count and max(count) > SUB_PUZZLES_MAX_ROWS:
                raise SudokuHipError(f"sub_puzzles: grid {count.index(max(count))} has {max(count)} candidates of {k} cells, more "
                                     f"than {SUB_PUZZLES_MAX_ROWS} (16 bytes each in one list): narrow allowed, widen required "
                                     f"or raise max_size")
            cells = torch.arange(81, device=self.device)
            found, per = [], torch.zeros(n, dtype=torch.int64, device=self.device)
            lo = 0
            while lo < n:
                hi, rows = lo + 1, count[lo]
                while hi < n and rows + count[hi] <= chunk:
                    rows += count[hi]
                    hi += 1
                if rows:
                    part, poff = self.hitting_sets(usets[uoff[lo]:uoff[hi]], uoff[lo:hi + 1] - uoff[lo], k, allowed=A[lo:hi],
                                                   required=R[lo:hi], packed=True, capacity=rows, **kw)
                    owner = torch.repeat_interleave(torch.arange(lo, hi, device=self.device), poff[1:] - poff[:-1])
                    for at in range(0, part.shape[0], chunk):
                        w = part[at:at + chunk].to(torch.int64) & 0xFFFFFFFF
                        own = owner[at:at + chunk]
                        boards = g[own] * ((w[:, cells >> 5] >> (cells & 31)) & 1).to(torch.uint8)
                        good = self.count_solutions(boards, limit=2, **kw) == 1
                        found.append(boards[good])
                        per.index_add_(0, own[good], torch.ones_like(own[good]))
                lo = hi
            puzzles = torch.cat(found) if found else torch.zeros((0, 81), dtype=torch.uint8, device=self.device)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
            offsets[1:] = torch.cumsum(per, dim=0)
        return puzzles, offsets

    # ---------------------------------------------------------- backdoors
    def backdoors(self, boards, level: int = 2, max_size: int = 3, solutions=None, return_count: bool = False,
                  return_first: bool = False, return_cover: bool = False, stream=None, max_waves: int = 0):
        """The size of every puzzle's smallest backdoor, as an int32 (n,)
        tensor (sdk_backdoor_batch; library extension, no reference
        counterpart; the definition is in include/sudoku_hip.h and DESIGN.md
        §23): the fewest cells which, filled with their digits of the
        board's completion, let rate()'s rules of `level` (1 naked singles, 2
        with hidden singles, 3 with locked candidates) finish the board; 0
        exactly when rate(board, max_level=level) is 1..level; max_size + 1
        when no set of at most max_size cells does (1 <= max_size <= 4).  It
        grades the boards rate() leaves undecided and says where a board is
        hard.  solutions: an (n, 81) tensor with the completion of every
        board; a byte > 9 in a board or outside 1..9 in its completion gives
        SDK_INVALID (-1), a completion that is no valid grid or does not keep
        the givens SDK_BACKDOOR_MISMATCH (-2).  solutions=None: every board's
        first completion from count_solutions(limit=2, return_first=True); a
        board with no completion comes back as SDK_BACKDOOR_MISMATCH, and for
        a board with several completions the backdoors are those to that
        first one (the sets that pin it).  return_count: also an int32 (n,)
        tensor, how many backdoors have that size (1 for size 0, 0 for
        max_size + 1 and the negative codes); return_first: also a uint8
        (n, 4) tensor, the lexicographically smallest of them, cells
        ascending, 255 in unused places (deterministic, but not the image
        under a symmetry); return_cover: also a uint8 (n, 81) tensor, 1 where
        a cell lies in at least one of them.  Size, count and cover depend on
        no search order, grid or batch.  max_waves > 0 caps the kernels'
        grids; results never depend on it.  Asynchronous on the stream; one
        cached scratch tensor serves every call, ordered like the
        workspace's."""
        level, max_size = int(level), int(max_size)
        if not 1 <= level <= _lib.SDK_BACKDOOR_MAX_LEVEL:
            raise ValueError(f"level must be 1..{_lib.SDK_BACKDOOR_MAX_LEVEL}")
        if not 1 <= max_size <= _lib.SDK_BACKDOOR_MAX_SIZE:
            raise ValueError(f"max_size must be 1..{_lib.SDK_BACKDOOR_MAX_SIZE}")
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        none = None  # the boards without a completion (solutions=None)
        if solutions is None:
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                counts, g = self.count_solutions(p, limit=2, return_first=True, stream=stream, max_waves=max_waves)
                none = counts == 0
        else:
            g = self._dev(as_boards(solutions, max_value=255))
            if g.shape != p.shape:
                raise ValueError("solutions must hold one grid per board")
        size = torch.empty(n, dtype=torch.int32, device=self.device)
        count = torch.empty(n, dtype=torch.int32, device=self.device) if return_count else None
        first = torch.empty((n, 4), dtype=torch.uint8, device=self.device) if return_first else None
        cover = torch.empty((n, 81), dtype=torch.uint8, device=self.device) if return_cover else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_backdoor_scratch", int(self.lib.sdk_backdoor_scratch_bytes(n, max_size, int(max_waves))))
            rc = self.lib.sdk_backdoor_batch(p.data_ptr(), g.data_ptr(), size.data_ptr(),
                                             count.data_ptr() if return_count else None,
                                             first.data_ptr() if return_first else None,
                                             cover.data_ptr() if return_cover else None, n, level, max_size,
                                             sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_backdoor_batch")
        if none is not None:
            # (the board itself stood in for the missing completion: whatever the kernels made of it)
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                size.masked_fill_(none, _lib.SDK_BACKDOOR_MISMATCH)
                if return_count:
                    count.masked_fill_(none, 0)
                if return_first:
                    first.masked_fill_(none[:, None], 255)
                if return_cover:
                    cover.masked_fill_(none[:, None], 0)
        out = ((size,) + ((count,) if return_count else ()) + ((first,) if return_first else ())
               + ((cover,) if return_cover else ()))
        return out if len(out) > 1 else size

    # --------------------------------------------------------- candidates
    def candidates(self, boards, return_count: bool = False, stream=None, max_waves: int = 0):
        """The exact candidates of every board, as an int16 (n, 81) tensor
        (sdk_candidates_batch; library extension, no reference counterpart;
        DESIGN.md §15): bit d-1 of marks[i, c] is set exactly when at least
        one completion of board i -- a valid Sudoku grid that keeps the givens
        -- puts digit d into cell c (rate()'s marks format; those marks are a
        superset of these).  A cell with one bit is forced (a given shows its
        own bit), a cell with several is where the board stays open, and a
        board with no completion has all marks zero.  There is no cap and no
        truncated case; the answer depends on no search order and the marks
        of a symmetry image of a board are the image of its marks.
        return_count: also an int32 (n,) tensor, min(2, completions): 0 for
        zero marks, 1 when every cell has one bit, 2 otherwise; SDK_INVALID
        (-1, with zero marks) for a byte > 9.  Givens that repeat a digit in a
        unit have no completion.  max_waves > 0 caps the kernel's grid;
        results never depend on it.  Asynchronous on the stream; one cached
        scratch tensor serves every call, ordered like the workspace's."""
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        marks = torch.empty((n, 81), dtype=torch.int16, device=self.device)
        count = torch.empty(n, dtype=torch.int32, device=self.device) if return_count else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_cand_scratch", int(self.lib.sdk_candidates_scratch_bytes(n, int(max_waves))))
            rc = self.lib.sdk_candidates_batch(p.data_ptr(), marks.data_ptr(), count.data_ptr() if return_count else None,
                                               n, sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_candidates_batch")
        return (marks, count) if return_count else marks

    # -------------------------------------------------- unique candidates
    def unique_candidates(self, boards, return_marks: bool = False, return_count: bool = False, stream=None,
                          max_waves: int = 0):
        """The candidates that exactly one completion holds, as an int16
        (n, 81) tensor (sdk_unique_candidates_batch; library extension, no
        reference counterpart): bit d-1 of once[i, c] is set
        exactly when exactly ONE completion of board i -- a valid Sudoku grid
        that keeps the givens -- puts digit d into cell c.  For an empty cell
        that is: board i with the clue (c, d) added is a proper puzzle.  A
        given's own bit is set exactly when the board itself has exactly one
        completion.  There is no cap and no truncated case; the answer depends
        on no search order and the answer of a symmetry image of a board is
        the image of its answer.
        return_marks: also the int16 (n, 81) tensor candidates() returns, bit
        for bit (at least one completion; once is a subset of it);
        return_count: also an int32 (n,) tensor, min(2, completions), as
        candidates() gives it; SDK_INVALID (-1, with zero arrays) for a byte
        > 9.  Givens that repeat a digit in a unit have no completion.  The
        optional outputs follow once in this order.  max_waves > 0 caps the
        kernel's grid; results never depend on it.  Asynchronous on the
        stream; one cached scratch tensor serves every call, ordered like the
        workspace's."""
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        once = torch.empty((n, 81), dtype=torch.int16, device=self.device)
        marks = torch.empty((n, 81), dtype=torch.int16, device=self.device) if return_marks else None
        count = torch.empty(n, dtype=torch.int32, device=self.device) if return_count else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_uniq_scratch", int(self.lib.sdk_unique_candidates_scratch_bytes(n, int(max_waves))))
            rc = self.lib.sdk_unique_candidates_batch(p.data_ptr(), once.data_ptr(),
                                                      marks.data_ptr() if return_marks else None,
                                                      count.data_ptr() if return_count else None, n, sc.data_ptr(),
                                                      sc.numel(), int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_unique_candidates_batch")
        out = (once,) + ((marks,) if return_marks else ()) + ((count,) if return_count else ())
        return out if len(out) > 1 else once

    # ----------------------------------------------------------- minimize
    def minimize(self, boards, order=None, max_empty: int = 81, probe: bool = False, return_removed: bool = False,
                 stream=None, max_waves: int = 0):
        """Redundant givens (sdk_minimize_batch; library extension, no
        reference counterpart): (puzzles uint8 (n, 81), status
        int32 (n,)), plus removed int32 (n,) with return_removed.  status[i] =
        min(2, completions of board i): 0 also for givens that repeat a digit
        in a unit, SDK_INVALID (-1) for a byte > 9.  Only a board with exactly
        one completion is changed; every other row comes back as it is, with
        removed 0.
        Greedy (the default): the board's givens are erased turn by turn --
        turn t takes cell order[i, t] (an (n, 81) tensor of cell numbers; a
        value above 80, a repeat or an empty cell skips the turn), or cell t
        when order is None -- while the puzzle keeps its one completion, until
        it has max_empty (0..81) empty cells, the input's own included.  With
        max_empty=81 and an order that names every given the result is a
        minimal proper puzzle.
        probe=True: order and max_empty are not read; every given is tested
        alone against the input board and the row returned has every
        individually redundant given erased (in general not a proper puzzle);
        a puzzle is minimal exactly when removed is 0.
        max_waves > 0 caps the kernel's grid; results never depend on it.
        Asynchronous on the stream; one cached scratch tensor serves every
        call, ordered like the workspace's."""
        max_empty = int(max_empty)
        if not 0 <= max_empty <= 81:
            raise ValueError("max_empty must be 0..81")
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = self._dev(as_boards(boards, max_value=255))
        n = p.shape[0]
        if order is not None:
            order = torch.as_tensor(order)
            if tuple(order.shape) != (n, 81):
                raise ValueError("order must have shape (n, 81)")
            if order.dtype != torch.uint8:  # a number that is no cell skips its turn
                order = torch.where((order < 0) | (order > 80), 255, order).to(torch.uint8)
            order = self._dev(order)
        out = torch.empty_like(p)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        removed = torch.empty(n, dtype=torch.int32, device=self.device) if return_removed else None
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_min_scratch", int(self.lib.sdk_minimize_scratch_bytes(n, int(max_waves))))
            rc = self.lib.sdk_minimize_batch(p.data_ptr(), order.data_ptr() if order is not None else None,
                                             out.data_ptr(), status.data_ptr(),
                                             removed.data_ptr() if return_removed else None, n,
                                             _lib.SDK_MIN_PROBE if probe else _lib.SDK_MIN_GREEDY, max_empty,
                                             sc.data_ptr(), sc.numel(), int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_minimize_batch")
        return (out, status, removed) if return_removed else (out, status)

    # ------------------------------------------------------------- sample
    def sample(self, boards, seed: int = 0, per_board: int = 1, first_key: int = 0, stream=None, max_waves: int = 0):
        """A random completion of every item (sdk_sample_batch; library
        extension, no reference counterpart): (grids uint8
        (n * per_board, 81), status int32 (n * per_board,)).  Item q samples
        board q // per_board under key first_key + q; its answer depends on the
        board, seed and key alone, so sample(boards[k:], first_key=k *
        per_board) is the tail of sample(boards).  status 1: the row is a valid
        grid that keeps the givens; 0: the board has no completion (givens that
        repeat a digit in a unit included); SDK_INVALID (-1): a byte > 9; for
        every status but 1 the row is the input board.  boards=None with
        per_board items samples the empty board (random_grids).
        Every branch of the search picks uniformly among the digits left in
        its cell (the rule is in include/sudoku_hip.h), so every completion of
        a board can come out, but they are NOT equally likely: this is a
        randomised search, not a uniform sampler.  seed and first_key are taken
        mod 2^64.  max_waves > 0 caps the kernel's grid; results never depend
        on it.  Asynchronous on the stream; one cached scratch tensor serves
        every call, ordered like the workspace's."""
        per_board = int(per_board)
        if per_board < 1:
            raise ValueError("per_board must be >= 1")
        if int(max_waves) < 0:
            raise ValueError("max_waves must be >= 0")
        p = None if boards is None else self._dev(as_boards(boards, max_value=255))
        n = 1 if p is None else p.shape[0]
        items = n * per_board
        if items > 2 ** 31 - 1:
            raise ValueError("at most 2**31 - 1 items")
        out = torch.empty((items, 81), dtype=torch.uint8, device=self.device)
        status = torch.empty(items, dtype=torch.int32, device=self.device)
        mask = (1 << 64) - 1
        with self._lock, torch.cuda.device(self.device):
            sc = self._scratch("_sample_scratch", int(self.lib.sdk_sample_scratch_bytes(items, int(max_waves))))
            rc = self.lib.sdk_sample_batch(None if p is None else p.data_ptr(), out.data_ptr(), status.data_ptr(), n,
                                           per_board, int(seed) & mask, int(first_key) & mask, sc.data_ptr(), sc.numel(),
                                           int(max_waves), self._ws_stream(stream))
        self._rc_only(rc, "sdk_sample_batch")
        return out, status

    def random_grids(self, n: int, seed: int = 0, first_key: int = 0, stream=None, max_waves: int = 0) -> torch.Tensor:
        """n random full grids as an (n, 81) uint8 tensor: sample() of the
        empty board under keys first_key .. first_key + n - 1, with no board
        bytes read (NULL boards).  Grid k is a function of seed and first_key
        + k alone.  Raises if an item reports anything but a completion (the
        call then waits for the kernel)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        if n == 0:
            return torch.empty((0, 81), dtype=torch.uint8, device=self.device)
        grids, status = self.sample(None, seed, per_board=n, first_key=first_key, stream=stream, max_waves=max_waves)
        if not bool((status == 1).all().item()):
            raise SudokuHipError("a random grid of the empty board was not reported as a completion")
        return grids

    def solve_batches(self, batches, outs, statuses, order="gen", stream=None, grid_waves: int = 0,
                      pipelined: bool = False):
        """Several device batches solved by ONE launch sequence
        (sdk_solve_batches): the lane-per-board kernel's queue runs over the
        batches laid end to end and drains once, so batches too small to fill
        the GPU on their own (a multi-GPU shard of one step) keep every lane
        busy.  Each batch's outputs are exactly solve()'s.  At most
        SDK_MAX_BATCHES (32) batches; unordered only."""
        if not (len(batches) == len(outs) == len(statuses)) or not 1 <= len(batches) <= _lib.SDK_MAX_BATCHES:
            raise ValueError(f"1..{_lib.SDK_MAX_BATCHES} batches, one out and one status tensor each")
        ps = [self._dev(as_boards(b)) for b in batches]
        for p, o, st in zip(ps, outs, statuses):
            if o.shape != p.shape or o.dtype != torch.uint8 or not o.is_contiguous() or o.device != self.device:
                raise ValueError("each out must be a contiguous (n, 81) uint8 tensor on the solver's device")
            if st.shape != (p.shape[0],) or st.dtype != torch.int32 or st.device != self.device:
                raise ValueError("each status must be an (n,) int32 tensor on the solver's device")
        k = len(ps)
        arr = ctypes.c_void_p * k
        ins = arr(*[p.data_ptr() for p in ps])
        out_p = arr(*[o.data_ptr() for o in outs])
        st_p = arr(*[st.data_ptr() for st in statuses])
        ns = (ctypes.c_int64 * k)(*[p.shape[0] for p in ps])
        with self._lock, torch.cuda.device(self.device):
            rc = self.lib.sdk_solve_batches(ins, out_p, st_p, ns, k, self.workspace.data_ptr(), _lib.order_code(order),
                                            self._ws_stream(stream), _grid_arg(grid_waves, pipelined))
        _lib.check(rc, "sdk_solve_batches")
        return list(zip(outs, statuses))

    def _stream_pool(self, k: int):
        """The solver's own streams, created once and shared by solve_host
        (compute, copy-in) and solve_inflight (one per slot): a process has
        few hardware queues (4), and streams past them share a queue and
        serialise."""
        with self._pool_lock:
            if self._pool is None:
                self._pool = []
            while len(self._pool) < k:
                self._pool.append(torch.cuda.Stream(self.device))
            return self._pool[:k]

    def _slot_solvers(self, inflight: int):
        """[self] + inflight - 1 more solvers on this device, each with its
        own workspace (~1.1 GB: per-lane stacks) and its own stream."""
        streams = self._stream_pool(inflight)
        with self._pool_lock:
            if self._slots is None:
                self._slots = [(self, streams[0])]
            while len(self._slots) < inflight:
                self._slots.append((BatchSolver(self.device), streams[len(self._slots)]))
            return self._slots[:inflight]

    def solve_inflight(self, batches, outs, statuses, inflight: Optional[int] = None, order="gen",
                       ordered: bool = False, launch_events=None, grid_waves: Optional[int] = None, group: int = 1,
                       pool_last: Optional[int] = None):
        """Solve a sequence of device batches with up to `inflight` launches
        in flight on this GPU: batch i runs on slot i % inflight (its own
        workspace and stream), so a launch's end -- its last boards draining
        while most lanes idle -- overlaps the next launches instead of
        idling the GPU.  inflight / grid_waves (waves per SIMD in each
        launch's grid; 0 = a full grid): default_inflight() -- six launches
        at 1 wave per SIMD with >= 8 hardware queues, else three at 2.  Each
        launch is a whole sdk_solve_batch_grid; results are those of solve().  outs[i] / statuses[i] receive batch i (buffers of
        batches that may be in flight together must not alias).  The
        caller's current stream waits for every batch; nothing synchronises
        the host.  launch_events: optional list that receives a (start, end)
        timing-event pair per launch, recorded on its slot's stream.
        group > 1: each launch solves `group` consecutive batches at once
        (solve_batches, one queue over them; unordered only) -- the
        strong-scaling steps, where one GPU's share of a step is too small to
        fill the GPU alone.  The last `pool_last` launches run unpipelined
        -- little is queued behind them, so their drained waves share the last
        boards through the XCD tail pool; every earlier launch is pipelined
        (its drained waves leave their slots to the launches on the other
        streams).  Default: half the launches in flight, rounded up (three of
        six: +1.3 % over six and over none at 20 steps, equal at 100; the
        N = 8 rank's 20 steps +12 %); with one launch in flight
        nothing can use the slots, so every launch shares its tail."""
        if inflight is None:
            inflight, gw = default_inflight()
            grid_waves = gw if grid_waves is None else grid_waves
        if inflight < 1:
            raise ValueError("inflight must be >= 1")
        if not 1 <= group <= _lib.SDK_MAX_BATCHES or (group > 1 and ordered):
            raise ValueError(f"group must be 1..{_lib.SDK_MAX_BATCHES} (and 1 in ordered mode)")
        if not (len(batches) == len(outs) == len(statuses)):
            raise ValueError("one out and one status tensor per batch")
        if grid_waves is None:
            grid_waves = GRID_WAVES_INFLIGHT if inflight > 1 else 0
        slots = self._slot_solvers(inflight)
        caller = torch.cuda.current_stream(self.device)
        # every batch in its final form (contiguous uint8 on this device)
        # BEFORE `ready` is recorded: a conversion enqueued on the caller
        # stream after it would race the slot stream's kernel
        batches = [self._dev(as_boards(b)) for b in batches]
        ready = torch.cuda.Event()
        ready.record(caller)
        for _, s in slots:
            s.wait_event(ready)
        pipes = pipelined_launches((len(batches) + group - 1) // group, inflight, pool_last)
        for i, lo in enumerate(range(0, len(batches), group)):
            solver, s = slots[i % inflight]
            pipe = pipes[i]
            bs, os_, sts = batches[lo:lo + group], outs[lo:lo + group], statuses[lo:lo + group]
            if launch_events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
            if group == 1:
                solver.solve(bs[0], out=os_[0], status=sts[0], order=order, ordered=ordered, stream=s,
                             grid_waves=grid_waves, pipelined=pipe)
            else:
                solver.solve_batches(bs, os_, sts, order=order, stream=s, grid_waves=grid_waves, pipelined=pipe)
            if launch_events is not None:
                e1.record(s)
                launch_events.append((e0, e1))
            for t in (*bs, *os_, *sts):  # caller-stream allocations used on the slot's stream
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(s)
        for _, s in slots:
            caller.wait_stream(s)
        return list(zip(outs, statuses))

    def inflight_stats(self, reset: bool = False) -> dict:
        """stats() summed over the solve_inflight slots' workspaces."""
        tot = None
        for solver, s in (self._slots or [(self, None)]):
            st = solver.stats(reset=reset, stream=s)
            tot = st if tot is None else {k: (tot[k] + v if k != "best" else min(tot[k], v)) for k, v in st.items()}
        return tot

    def solve_host(self, puzzles: torch.Tensor, order="gen", chunk: int = 1 << 18,
                   out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Host boards in, host solutions and statuses out (the serving
        path), pipelined: chunk i+1 is copied in on one stream and chunk i-1
        copied out on another while chunk i is solved, so both PCIe
        directions overlap the kernel.  Give pinned host tensors (`out` /
        `status` are allocated pinned when omitted); pageable input is copied
        synchronously.  Same results as solve(); returns when all is back."""
        p = as_boards(puzzles)
        if p.device.type != "cpu":
            raise ValueError("solve_host takes host boards; use solve() for device tensors")
        n = p.shape[0]
        if out is None:
            out = torch.empty((n, 81), dtype=torch.uint8).pin_memory()
        if status is None:
            status = torch.empty(n, dtype=torch.int32).pin_memory()
        if out.shape != (n, 81) or out.dtype != torch.uint8 or out.device.type != "cpu":
            raise ValueError("out must be a host (n, 81) uint8 tensor")
        if status.shape != (n,) or status.dtype != torch.int32 or status.device.type != "cpu":
            raise ValueError("status must be a host (n,) int32 tensor")
        if n == 0:
            return out, status
        d_in = torch.empty((n, 81), dtype=torch.uint8, device=self.device)
        d_out = torch.empty_like(d_in)
        d_st = torch.empty(n, dtype=torch.int32, device=self.device)
        caller = torch.cuda.current_stream(self.device)
        # three streams in all: the solver's two (shared with solve_inflight's
        # slots, created once) and the caller's for the copies out.  A
        # process has few hardware queues (4); past them streams share one,
        # and a copy queued behind a solve serialises the pipeline.
        compute, h2d = self._stream_pool(2)
        d2h = caller
        compute.wait_stream(caller)
        h2d.wait_stream(caller)  # the device buffers are caller-stream allocations
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            with torch.cuda.stream(h2d):
                d_in[lo:hi].copy_(p[lo:hi], non_blocking=True)
            compute.wait_stream(h2d)
            self.solve(d_in[lo:hi], out=d_out[lo:hi], status=d_st[lo:hi], order=order, stream=compute)
            d2h.wait_stream(compute)
            with torch.cuda.stream(d2h):
                out[lo:hi].copy_(d_out[lo:hi], non_blocking=True)
                status[lo:hi].copy_(d_st[lo:hi], non_blocking=True)
        for t in (d_in, d_out, d_st):
            t.record_stream(h2d)
            t.record_stream(compute)
        d2h.synchronize()
        return out, status

    def check(self, grids, mode: int = 0, stream=None) -> torch.Tensor:
        """mode 0: Sudoku.check (sudoku.py:119-140); mode 1: node.py:82-116."""
        g = self._dev(as_boards(grids, max_value=255))
        ok = torch.empty(g.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdk_check_batch(g.data_ptr(), ok.data_ptr(), g.shape[0], mode, self._stream(stream))
        _lib.check(rc, "sdk_check_batch")
        return ok

    def first_candidate(self, grids, cells, stream=None) -> torch.Tensor:
        """node.py:76-80 per (board, cell) task; 0 means None."""
        g = self._dev(as_boards(grids, max_value=255))
        c = self._dev(torch.as_tensor(cells, dtype=torch.int32).reshape(-1))
        if c.shape[0] != g.shape[0]:
            raise ValueError("one cell index per board")
        num = torch.empty(g.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdk_first_candidate_batch(g.data_ptr(), c.data_ptr(), num.data_ptr(), g.shape[0],
                                                    self._stream(stream))
        _lib.check(rc, "sdk_first_candidate_batch")
        return num

    def peer_solve(self, boards, stream=None):
        """node.py:534-557 P2PNode.peer_sudoku_solve (the reference's HTTP
        /solve greedy loop) per board: (boards it leaves (n,81), status (n,),
        validations (n,)); status SDK_SOLVED / SDK_UNSOLVABLE (check passed /
        failed) or SDK_NO_RETURN (node.py never returns on that board)."""
        g = self._dev(as_boards(boards))
        n = g.shape[0]
        out = torch.empty_like(g)
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        val = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdk_peer_solve_batch(g.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                               self._stream(stream))
        _lib.check(rc, "sdk_peer_solve_batch")
        return out, st, val

    def new_peer_state(self) -> torch.Tensor:
        """A new P2PNode's persistent /solve state (partial_solution and
        tried_numbers_by_position, node.py:149, 167) for peer_solve_seq."""
        return torch.zeros(_lib.SDK_PEER_STATE_BYTES, dtype=torch.uint8, device=self.device)

    def peer_solve_seq(self, boards, state: torch.Tensor, stream=None):
        """The same /solve loop on ONE node serving the boards as requests in
        order (sdk_peer_solve_seq): each request starts from the node state
        the previous one left; `state` (new_peer_state()) is updated in place.
        Returns (boards left, status, validations per request)."""
        g = self._dev(as_boards(boards))
        if state.device != self.device or state.dtype != torch.uint8 or state.numel() != _lib.SDK_PEER_STATE_BYTES:
            raise ValueError("state must be a new_peer_state() tensor on this device")
        n = g.shape[0]
        out = torch.empty_like(g)
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        val = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdk_peer_solve_seq(g.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                             state.data_ptr(), self._stream(stream))
        _lib.check(rc, "sdk_peer_solve_seq")
        return out, st, val

    def expand(self, nodes, order="gen", stream=None) -> torch.Tensor:
        """One frontier level (sdk_expand_frontier); synchronises to size it."""
        nd = self._dev(as_boards(nodes))
        n = nd.shape[0]
        tmp = torch.empty_like(nd)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        cap = 9 * n
        children = torch.empty((max(cap, 1), 81), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sdk_expand_frontier(nd.data_ptr(), n, tmp.data_ptr(), offsets.data_ptr(),
                                              children.data_ptr(), cap, _lib.order_code(order),
                                              self._stream(stream))
        _lib.check(rc, "sdk_expand_frontier")
        total = int(offsets[n].item()) if n else 0
        if total > cap:
            raise SudokuHipError(f"frontier overflow: {total} > {cap}")
        return children[:total]

    def stats(self, reset: bool = False, stream=None) -> dict:
        out = (ctypes.c_int64 * 6)()
        with self._lock, torch.cuda.device(self.device):
            rc = self.lib.sdk_read_stats(self.workspace.data_ptr(), out, 1 if reset else 0, self._ws_stream(stream))
        _lib.check(rc, "sdk_read_stats")
        return {"finished": out[0], "solved": out[1], "guesses": out[2], "sweeps": out[3], "best": out[4],
                "deferred": out[5]}

    def verify(self, stream=None) -> dict:
        """Every board handed to this workspace's solve kernels since the last
        stats(reset=True) has its answer, and no kernel reported an error
        (sdk_verify_workspace; synchronises the stream).  Returns {"assigned",
        "finished", "error"}; raises SudokuHipError otherwise -- a board a
        kernel took but could not finish (a tail-pool record never published,
        DESIGN.md §3) is never a silent stale output."""
        out = (ctypes.c_int64 * 4)()
        with self._lock, torch.cuda.device(self.device):
            rc = self.lib.sdk_verify_workspace(self.workspace.data_ptr(), out, self._ws_stream(stream))
        if rc == -3:
            raise SudokuHipError(self.lib.sdk_last_error().decode(errors="replace"))
        _lib.check(rc, "sdk_verify_workspace")
        return {"assigned": out[0], "finished": out[1], "error": out[2]}

    def verify_inflight(self) -> dict:
        """verify() over the solve_inflight slots' workspaces (summed)."""
        tot = {"assigned": 0, "finished": 0, "error": 0}
        for solver, s in (self._slots or [(self, None)]):
            for k, v in solver.verify(stream=s).items():
                tot[k] += v
        return tot

    def stats_snapshot(self, stream=None) -> torch.Tensor:
        """The counters of stats() as a device int64 (6,) tensor, copied
        asynchronously in stream order with this workspace's solves
        (sdk_snapshot_stats): the difference of two snapshots around a solve
        is that solve's own work, with no host synchronisation."""
        out = torch.empty(6, dtype=torch.int64, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            rc = self.lib.sdk_snapshot_stats(self.workspace.data_ptr(), out.data_ptr(), self._ws_stream(stream))
        _lib.check(rc, "sdk_snapshot_stats")
        return out

    # ------------------------------------------------------ frontier split
    def frontier(self, board, target: int = 4096, max_levels: int = 81, order="gen") -> torch.Tensor:
        """Expand one board's search tree level by level (in the walk's
        order) until the frontier holds >= target nodes, or the next level
        would be narrower (dead branches outnumber new ones), or nothing is
        left to split.  Returns the frontier, in walk order."""
        nodes = self._dev(as_boards(board))
        for _ in range(max_levels):
            if nodes.shape[0] >= target or nodes.shape[0] == 0:
                break
            children = self.expand(nodes, order=order)
            if children.shape[0] == nodes.shape[0] and torch.equal(children, nodes):
                break  # every node already solved: nothing left to split
            if 0 < children.shape[0] < nodes.shape[0]:
                break  # narrowing: keep the wider level
            nodes = children
        return nodes

    def solve_one_split(self, board, target: int = 4096, order="gen") -> Tuple[bool, torch.Tensor]:
        """Single hard board: frontier split over all waves of this GPU, then
        an ordered solve; returns (solved, grid81)."""
        root = self._dev(as_boards(board))
        if root.shape[0] != 1:
            raise ValueError("solve_one_split takes exactly one board")
        nodes = self.frontier(root, target, order=order)
        if nodes.shape[0] == 0:
            return False, root[0].clone()
        sols, st = self.solve(nodes, ordered=True, order=order)
        hit = torch.nonzero(st == SDK_SOLVED)
        if hit.numel() == 0:
            return False, root[0].clone()
        return True, sols[int(hit[0, 0].item())].clone()


_SOLVERS = {}
_SOLVERS_LOCK = threading.Lock()


def get_solver(device=None) -> BatchSolver:
    dev = _require_gpu(device)
    with _SOLVERS_LOCK:
        s = _SOLVERS.get(dev.index)
        if s is None:
            s = _SOLVERS[dev.index] = BatchSolver(dev)
        return s
