"""The boards and recorded answers the exact-candidates tests share
(test_cand_host.py on the CPU, test_gpu_cand.py on the GPU), and the oracle's
restatement of the definition:

    marks[c] bit d-1  <=>  some valid completion of the board puts d into c

tests/golden/make_cand_cases.py records oracle_marks() of its boards in
tests/golden/cand_cases.json; load_fixture() reads them back.  Loaded once per
process and shared, never modified.
"""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "cand_cases.json")
INVALID = -1  # SDK_INVALID
FAULT = -3    # SDK_FAULT
ALL = 0x1FF
# boards taken from count_cases.sets(), by position in their set, and from
# rate_cases.json (the first RATE5 boards with rating 5).  Set b: its first 15
# and HEAVY_B, the board of the 256 that costs the host build of plane_cand.h
# the most (22 012 passes, 17 times the set's mean: a wave waits for it)
HEAVY_B = 177
TAKE = (("a", tuple(range(32))), ("b", tuple(range(15)) + (HEAVY_B,)), ("c", tuple(range(64))),
        ("d", tuple(range(64))), ("e", tuple(range(16))), ("f", tuple(range(5))))
RATE5 = 8


def board_text(board):
    """81 values as 81 hex digits (a byte of 10 is 'a')."""
    return "".join("%x" % int(v) for v in board)


def board_from_text(s):
    return np.array([int(ch, 16) for ch in s], dtype=np.uint8)


def marks_text(marks):
    """81 candidate masks as 243 hex digits (three per cell)."""
    return "".join("%03x" % int(m) for m in marks)


def marks_from_text(s):
    return [int(s[3 * i:3 * i + 3], 16) for i in range(81)]


def count_of(marks):
    """The count the marks imply: 0 for none, 1 when every cell has one bit, 2 otherwise."""
    m = np.asarray(marks, dtype=np.int64)
    if not m.any():
        return 0
    return 1 if ((m != 0) & (m & (m - 1) == 0)).all() else 2


def _peers():
    units = [[9 * r + c for c in range(9)] for r in range(9)] + [[9 * r + c for r in range(9)] for c in range(9)] + \
            [[9 * (3 * (b // 3) + i) + 3 * (b % 3) + j for i in range(3) for j in range(3)] for b in range(9)]
    return [sorted({x for u in units if c in u for x in u} - {c}) for c in range(81)]


PEERS = _peers()


def oracle_marks(board):
    """(marks[81], count) of one board from the oracle's counter alone: per
    empty cell and digit that repeats no digit of the cell's units,
    O.count_solutions(board with the cell set, 1) >= 1; a given's own bit when
    the board has a completion.  A byte > 9: zeros and INVALID; clashing
    givens: zeros and 0."""
    from oracle import oracle as O
    import count_cases as C
    board = np.asarray(board, dtype=np.uint8).reshape(81)
    if (board > 9).any():
        return [0] * 81, INVALID
    if C.givens_clash(board) or O.count_solutions(board, 1) == 0:
        return [0] * 81, 0
    marks = [0] * 81
    for c in range(81):
        if board[c]:
            marks[c] = 1 << (int(board[c]) - 1)
            continue
        seen = {int(board[p]) for p in PEERS[c]}
        for d in range(1, 10):
            if d in seen:
                continue
            trial = board.copy()
            trial[c] = d
            if O.count_solutions(trial, 1) >= 1:
                marks[c] |= 1 << (d - 1)
    return marks, count_of(marks)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/cand_cases.json as (names, boards (n, 81) uint8, marks
    (n, 81) uint16, count (n,) int32), read-only."""
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    names = [c["name"] for c in cases]
    boards = np.array([board_from_text(c["board"]) for c in cases], dtype=np.uint8)
    marks = np.array([marks_from_text(c["marks"]) for c in cases], dtype=np.uint16)
    count = np.array([c["count"] for c in cases], dtype=np.int32)
    for v in (boards, marks, count):
        v.setflags(write=False)
    return names, boards, marks, count
