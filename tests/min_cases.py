"""The boards and recorded answers the minimisation tests share
(test_min_host.py on the CPU, test_gpu_min.py on the GPU), and the oracle's
restatement of sdk_minimize_batch's definition (include/sudoku_hip.h) as the
plain loop over O.count_solutions(trial, 2).

tests/golden/make_min_cases.py records oracle_minimize() of its cases in
tests/golden/min_cases.json; load_fixture() reads them back.  Loaded once per
process and shared, never modified.
"""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "min_cases.json")
INVALID = -1  # SDK_INVALID
FAULT = -3    # SDK_FAULT
GREEDY, PROBE = 0, 1  # SDK_MIN_GREEDY, SDK_MIN_PROBE
MIN_LEVELS = 82       # plane::MIN_LEVELS: a lane's stack lines
SEED = 20261


def board_text(board):
    """81 values as 81 hex digits (a byte of 10 is 'a')."""
    return "".join("%x" % int(v) for v in board)


def board_from_text(s):
    return np.array([int(ch, 16) for ch in s], dtype=np.uint8)


def order_text(order):
    """81 turn bytes as 162 hex digits (two per turn)."""
    return "".join("%02x" % int(v) for v in order)


def order_from_text(s):
    return np.array([int(s[2 * i:2 * i + 2], 16) for i in range(81)], dtype=np.uint8)


def oracle_minimize(board, order, mode, max_empty):
    """(out[81], status, removed) of one board from the oracle's counter
    alone.  order: 81 turn bytes or None (turn t takes cell t)."""
    from oracle import oracle as O
    import count_cases as C
    board = np.asarray(board, dtype=np.uint8).reshape(81)
    if (board > 9).any():
        return board.copy(), INVALID, 0
    status = 0 if C.givens_clash(board) else O.count_solutions(board, 2)
    if status != 1:
        return board.copy(), status, 0
    p, removed = board.copy(), 0
    if mode == PROBE:
        for c in np.nonzero(board)[0]:
            trial = board.copy()
            trial[c] = 0
            if O.count_solutions(trial, 2) == 1:
                p[c] = 0
                removed += 1
        return p, 1, removed
    for t in range(81):
        c = t if order is None else int(order[t])
        if c > 80 or p[c] == 0:
            continue
        if int((p == 0).sum()) >= max_empty:
            break
        trial = p.copy()
        trial[c] = 0
        if O.count_solutions(trial, 2) == 1:
            p, removed = trial, removed + 1
    return p, 1, removed


def names_every_given(board, order):
    """Does the turn order (None: every cell) name every given of the board?"""
    return order is None or set(np.nonzero(board)[0].tolist()) <= set(int(c) for c in order)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/min_cases.json as a dict of read-only arrays, one row a
    case: names (list), boards (n, 81) uint8, order (n, 81) uint8 and
    has_order (n,) bool (False: the case's order is NULL; its row is 0..80),
    mode, max_empty, status, removed (n,) int32, out (n, 81) uint8."""
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    fx = {"names": [c["name"] for c in cases],
          "boards": np.array([board_from_text(c["board"]) for c in cases], dtype=np.uint8),
          "has_order": np.array([c["order"] is not None for c in cases]),
          "order": np.array([np.arange(81, dtype=np.uint8) if c["order"] is None else order_from_text(c["order"])
                             for c in cases], dtype=np.uint8),
          "out": np.array([board_from_text(c["board"] if c["out"] is None else c["out"]) for c in cases],
                          dtype=np.uint8)}
    for k in ("mode", "max_empty", "status", "removed"):
        fx[k] = np.array([c[k] for c in cases], dtype=np.int32)
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx
