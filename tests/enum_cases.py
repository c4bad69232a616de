"""What the completion-list tests share (test_enum_host.py on the CPU,
test_gpu_enum.py on the GPU): the host model's entry
(tests/native/enum_host.cpp), the check that a list IS a board's completion
set, and exact_cases.py's boards, knobs and counts, reused as they are.

No fixture: a list is the completion set of a board exactly when every row is
a valid grid, every row keeps the board's givens, the rows are pairwise
distinct and their number is the board's exact count -- known from
tests/golden/exact_cases.json or the oracle's counter.
"""
import ctypes

import numpy as np

import native_build
from exact_cases import (DONE, FAULT, H1_COUNT, INVALID, KNOBS, LEVELS, MANY, PARTIAL, RUN_MAX, TINY,  # noqa: F401
                         check_path, light, load_fixture, mixed, placed, placements, pool, pool_sets)

LIMITED = 3  # SDK_ENUM_LIMITED
INFO = ("rounds", "donated", "parks", "max_passes", "total", "listed")

_vp, _i64, _int, _i32, _u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32
native_build.PROTOS.setdefault("enum_host", {
    # in, n, grids, owner, capacity, limit, count, status, waves, slice, max_rounds, max_tasks, max_depth,
    # info (6 x int64, NULL ok) -> 0 / -2
    "enum_host_batch": ([_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _int, _i32, _int, _i64, _u32, _vp], _int)})

_UNITS = np.array([[9 * r + c for c in range(9)] for r in range(9)] +
                  [[9 * r + c for r in range(9)] for c in range(9)] +
                  [[9 * (3 * (b // 3) + r) + 3 * (b % 3) + c for r in range(3) for c in range(3)] for b in range(9)])


def host_enum(lib, boards, capacity, limit=0, waves=1, slice=4096, max_rounds=MANY, max_tasks=0, max_depth=LEVELS):
    """The host model's answer: (grids (capacity, 81) among 0xA5 bytes, owner
    (capacity,) among -7, count (n,) int64, status (n,) int32, info dict)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    grids = np.full((capacity, 81), 0xA5, dtype=np.uint8)
    owner = np.full(capacity, -7, dtype=np.int32)
    count = np.full(len(boards), -12345, dtype=np.int64)
    status = np.full(len(boards), 12345, dtype=np.int32)
    info = np.zeros(6, dtype=np.int64)
    rc = lib.enum_host_batch(boards.ctypes.data, len(boards), grids.ctypes.data if capacity else None,
                             owner.ctypes.data if capacity else None, capacity, limit, count.ctypes.data,
                             status.ctypes.data, waves, slice, max_rounds, max_tasks, max_depth, info.ctypes.data)
    assert rc == 0, rc
    return grids, owner, count, status, dict(zip(INFO, (int(v) for v in info)))


def valid_grids(rows):
    """(m,) bool: row k is a grid whose every row, column and box holds 1..9
    once -- numpy alone, nothing of the library."""
    rows = np.asarray(rows).reshape(-1, 81)
    bits = np.where((rows >= 1) & (rows <= 9), 1 << rows.astype(np.int64), 0)
    return (np.bitwise_or.reduce(bits[:, _UNITS], axis=2) == 0x3FE).all(axis=1)


def row_keys(rows):
    """Every row as one 81-byte string scalar: equal rows, equal keys, and
    the keys sort as the rows do lexicographically."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 81)
    return rows.view("S81").ravel() if len(rows) else np.zeros(0, dtype="S81")


def sorted_rows(rows):
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 81)
    return rows[np.argsort(row_keys(rows), kind="stable")]


def check_listed(boards, grids, owner, listed):
    """What holds for rows [0, listed) whatever the capacity, limit or
    budget: owners in range, rows valid, givens kept, no row twice within a
    board; nothing at or beyond `listed` written.  Returns rows per board."""
    boards = np.asarray(boards).reshape(-1, 81)
    g, o = grids[:listed], owner[:listed]
    assert (grids[listed:] == 0xA5).all() and (owner[listed:] == -7).all()
    assert ((o >= 0) & (o < len(boards))).all()
    assert valid_grids(g).all()
    given = boards[o]
    assert ((given == 0) | (given == g)).all()
    both = np.concatenate([o.astype(">i4").view(np.uint8).reshape(-1, 4), g], axis=1)
    assert len(np.unique(np.ascontiguousarray(both).view("S85").ravel())) == listed
    return np.bincount(o, minlength=len(boards))


def check_complete(boards, grids, owner, listed, want):
    """The list holds the completion set of every board: check_listed and
    want[i] rows of board i."""
    per = check_listed(boards, grids, owner, listed)
    bad = np.nonzero(per != np.asarray(want))[0]
    assert len(bad) == 0, [(int(i), int(per[i]), int(want[i])) for i in bad[:10]]


def by_board(grids, owner, listed, n):
    """The public form of a raw list: rows ordered by board, then
    lexicographically; (rows, offsets)."""
    g, o = grids[:listed], owner[:listed]
    order = np.argsort(row_keys(g), kind="stable")
    order = order[np.argsort(o[order], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(o, minlength=n))])
    return g[order], off
