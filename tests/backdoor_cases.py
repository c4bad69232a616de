"""The backdoor tests' shared cases: the loader of
tests/golden/backdoor_cases.json (written by tests/golden/make_backdoor_cases.py
from rate_host_batch alone: every k-subset of the empty cells, no pruning) and
the definition of DESIGN.md §23 in plain Python on rate_cases.closure, cheap
enough to run live only at sizes 0 and 1.

    names, boards, grids, runs = load_fixture()
    runs[(level, max_size)] = (idx, size, count, first, cover)

idx: the cases the run covers (indices into names); the arrays are aligned to
it.  A board or grid byte is one hexadecimal digit in the file, so that the
invalid bytes have a place.
"""
import json
import os

import numpy as np

import rate_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1    # SDK_INVALID
MISMATCH = -2   # SDK_BACKDOOR_MISMATCH
MAX_SIZE = 4    # SDK_BACKDOOR_MAX_SIZE
NONE4 = [255, 255, 255, 255]


def hexbytes(s):
    return np.array([int(c, 16) for c in s], dtype=np.uint8)


def hextext(a):
    return "".join("%x" % int(v) for v in a)


def cover_text(cover):
    """81 flags as 21 hex digits (cell c = bit c)."""
    return "%021x" % sum(1 << c for c in range(81) if cover[c])


def cover_from_text(s):
    v = int(s, 16)
    return [(v >> c) & 1 for c in range(81)]


def load_fixture():
    with open(os.path.join(HERE, "golden", "backdoor_cases.json")) as f:
        doc = json.load(f)
    cases = doc["cases"]
    names = [c["name"] for c in cases]
    boards = np.array([hexbytes(c["board"]) for c in cases], dtype=np.uint8)
    grids = np.array([hexbytes(c["grid"]) for c in cases], dtype=np.uint8)
    runs = {}
    for i, c in enumerate(cases):
        for r in c["runs"]:
            runs.setdefault((r["level"], r["max_size"]), []).append((i, r))
    out = {}
    for key, rows in runs.items():
        out[key] = (np.array([i for i, _ in rows]),
                    np.array([r["size"] for _, r in rows], dtype=np.int32),
                    np.array([r["count"] for _, r in rows], dtype=np.int32),
                    np.array([r["first"] for _, r in rows], dtype=np.uint8).reshape(-1, 4),
                    np.array([cover_from_text(r["cover"]) for _, r in rows], dtype=np.uint8).reshape(-1, 81))
    return names, boards, grids, out


def check_pair(board, grid):
    """0, INVALID or MISMATCH for (board, grid), by the text of the definition."""
    board, grid = [int(v) for v in board], [int(v) for v in grid]
    if any(v > 9 for v in board) or any(not 1 <= v <= 9 for v in grid):
        return INVALID
    if any(sorted(grid[c] for c in unit) != list(range(1, 10)) for unit in R.UNITS):
        return MISMATCH
    if any(b and b != g for b, g in zip(board, grid)):
        return MISMATCH
    return 0


def is_backdoor(board, grid, cells, level):
    cand = R.start([grid[c] if c in cells else board[c] for c in range(81)])
    return not R.closure(cand, level) and R.solved(cand)


def backdoors(board, grid, level, max_size):
    """(size, count, first[4], cover[81]) by the definition: every subset of
    ALL 81 cells, smallest size first."""
    from itertools import combinations
    code = check_pair(board, grid)
    if code:
        return code, 0, NONE4, [0] * 81
    board, grid = [int(v) for v in board], [int(v) for v in grid]
    if is_backdoor(board, grid, (), level):
        return 0, 1, NONE4, [0] * 81
    for k in range(1, max_size + 1):
        hits = [s for s in combinations(range(81), k) if is_backdoor(board, grid, s, level)]
        if hits:
            cover = [int(any(c in s for s in hits)) for c in range(81)]
            return k, len(hits), list(hits[0]) + [255] * (4 - k), cover
    return max_size + 1, 0, NONE4, [0] * 81
