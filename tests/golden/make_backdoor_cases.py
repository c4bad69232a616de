"""Write tests/golden/backdoor_cases.json: boards, grids and their smallest
backdoors (size, count, first, cover) at the runs the tests use.

    python tests/golden/make_backdoor_cases.py

Every answer comes from rate_host_batch (tests/native/rate_host.cpp, pinned by
tests/test_rate_host.py) on the board with the subset's cells filled from the
grid: EVERY k-subset of the board's EMPTY cells, in lexicographic order, no
pruning, k = 0, 1, ... until a size has a backdoor.  csrc/backdoor.h is not
involved.  (The definition speaks of all 81 cells; a given in S changes
nothing, so a set with one is never minimum unless it is one without it.)
About a minute on 16 cores.  The boards:

  the 80 class_* and the first 40 seed_* boards of rate_cases.json, the grid
    from their level-4 marks; 12 puzzles_30_* of rating 1 likewise;
  proper_undecided with its one completion and undecided_trials_removed with
    each of its two (count_host_batch's first completion; the other by fixing
    one cell to another digit);
  a full grid as its own board; the empty board with a grid;
  a board with one given changed against its grid, and a grid with two equal
    digits in a row at cells the board leaves empty (MISMATCH);
  a byte 10 in the board and a byte 0 in the grid (INVALID).

Runs: levels 1, 2, 3 at max_size 3 and level 2 at max_size 1 for all; level 1
at max_size 4 for class_2 .. class_5 and the empty board.
"""
import ctypes
import json
import os
import sys
from collections import Counter
from itertools import combinations

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import backdoor_cases as B  # noqa: E402
import native_build  # noqa: E402
import rate_cases as R  # noqa: E402

OUT = os.path.join(HERE, "backdoor_cases.json")
CHUNK = 1 << 18
_vp = ctypes.c_void_p
native_build.PROTOS.setdefault("rate_host", {"rate_host_batch": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int], None)})

# what the issue's tables list: run -> {size: boards} over the class_* and seed_* cases
TALLIES = {
    ("class_", 1, 3): {3: 31, 4: 49}, ("class_", 2, 3): {0: 34, 1: 44, 2: 2}, ("class_", 3, 3): {0: 54, 1: 26},
    ("seed_", 1, 3): {1: 4, 2: 31, 3: 5}, ("seed_", 2, 3): {1: 40}, ("seed_", 3, 3): {0: 8, 1: 32},
}
TRIPLES = {
    ("proper_undecided", 1, 3): (3, 12, [3, 23, 73, 255]),
    ("proper_undecided", 2, 3): (3, 566, [1, 3, 66, 255]),
    ("proper_undecided", 3, 3): (3, 862, [1, 3, 66, 255]),
    ("class_2", 1, 4): (4, 27, [0, 3, 28, 41]),
    ("class_3", 1, 4): (4, 95, [0, 27, 35, 70]),
    ("class_4", 1, 4): (4, 4, [5, 9, 47, 59]),
    ("class_5", 1, 4): (4, 34, [0, 15, 28, 48]),
}


def ratings(lib, boards, level):
    r = np.empty(len(boards), dtype=np.int32)
    lib.rate_host_batch(boards.ctypes.data, r.ctypes.data, None, None, len(boards), level)
    return r


def answer(lib, board, grid, level, max_size):
    code = B.check_pair(board, grid)
    if code:
        return code, 0, B.NONE4, [0] * 81
    empty = [c for c in range(81) if board[c] == 0]
    for k in range(0, max_size + 1):
        sets = list(combinations(empty, k))
        sets = np.array(sets, dtype=np.int64).reshape(len(sets), k)
        hits = []
        for at in range(0, len(sets), CHUNK):
            part = sets[at:at + CHUNK]
            trial = np.repeat(board[None, :], len(part), axis=0)
            if k:
                trial[np.arange(len(part))[:, None], part] = grid[part]
            r = ratings(lib, np.ascontiguousarray(trial), level)
            hits.append(part[(r >= 1) & (r <= level)])
        hits = np.concatenate(hits)
        if len(hits):
            cover = np.zeros(81, dtype=np.uint8)
            cover[np.unique(hits)] = 1
            return k, len(hits), [int(v) for v in hits[0]] + [255] * (4 - k), cover.tolist()
    return max_size + 1, 0, B.NONE4, [0] * 81


def completions(board):
    """Up to two completions of a board with at most two (count_host_batch)."""
    lib = native_build.host_lib("count_host")

    def first(b):
        b = np.ascontiguousarray(b, dtype=np.uint8)
        cnt, out = np.zeros(1, dtype=np.int32), np.zeros(81, dtype=np.uint8)
        p, d = ctypes.c_uint64(0), ctypes.c_uint32(0)
        lib.count_host_batch(b.ctypes.data, cnt.ctypes.data, out.ctypes.data, 1, 3, 81, ctypes.byref(p), ctypes.byref(d))
        return int(cnt[0]), out
    n, g = first(board)
    if n == 1:
        return [g]
    assert n == 2, n
    for c in range(81):
        if board[c]:
            continue
        for d in range(1, 10):
            if d != g[c]:
                b = board.copy()
                b[c] = d
                m, h = first(b)
                if m:
                    return [g, h]
    raise AssertionError("no second completion")


def main():
    lib = native_build.host_lib("rate_host", openmp=True)
    names, boards, rating, _, marks = R.load_fixture()
    at = {n: k for k, n in enumerate(names)}
    grid_of = lambda i: np.array([int(m).bit_length() for m in marks[i]], dtype=np.uint8)
    cases = []  # (name, board, grid)
    for k in range(80):
        cases.append((f"class_{k}", boards[at[f"class_{k}"]], grid_of(at[f"class_{k}"])))
    for k in range(40):
        cases.append((f"seed_{k}", boards[at[f"seed_{k}"]], grid_of(at[f"seed_{k}"])))
    p30 = [n for n in names if n.startswith("puzzles_30_") and rating[at[n]] == 1][:12]
    assert len(p30) == 12
    cases += [(n, boards[at[n]], grid_of(at[n])) for n in p30]
    pu = boards[at["proper_undecided"]]
    (g,) = completions(pu)
    cases.append(("proper_undecided", pu, g))
    ut = boards[at["undecided_trials_removed"]]
    ga, gb = completions(ut)
    cases += [("undecided_trials_removed_a", ut, ga), ("undecided_trials_removed_b", ut, gb)]
    g0, b1 = grid_of(at["class_0"]), boards[at["class_1"]].copy()
    cases.append(("full_grid", g0.copy(), g0.copy()))
    cases.append(("empty", np.zeros(81, dtype=np.uint8), g0.copy()))
    g1 = grid_of(at["class_1"])
    cell = int(np.nonzero(b1)[0][0])
    changed = b1.copy()
    changed[cell] = b1[cell] % 9 + 1
    cases.append(("given_changed", changed, g1.copy()))
    free = [c for c in range(9) if b1[c] == 0][:2]
    rep = g1.copy()
    rep[free[1]] = rep[free[0]]
    cases.append(("grid_row_repeat", b1.copy(), rep))
    ten = b1.copy()
    ten[40] = 10
    cases.append(("board_byte_10", ten, g1.copy()))
    zero = g1.copy()
    zero[80] = 0
    cases.append(("grid_byte_0", b1.copy(), zero))

    deep = {"class_2", "class_3", "class_4", "class_5", "empty"}
    docs = []
    for name, b, g in cases:
        runs = [(1, 3), (2, 3), (3, 3), (2, 1)] + ([(1, 4)] if name in deep else [])
        rows = []
        for level, max_size in runs:
            size, count, first, cover = answer(lib, b, g, level, max_size)
            rows.append({"level": level, "max_size": max_size, "size": size, "count": count, "first": first,
                         "cover": B.cover_text(cover)})
        docs.append({"name": name, "board": B.hextext(b), "grid": B.hextext(g), "runs": rows})
        print(name, [(r["level"], r["max_size"], r["size"], r["count"]) for r in rows], flush=True)

    def run_of(doc, level, max_size):
        (r,) = [r for r in doc["runs"] if (r["level"], r["max_size"]) == (level, max_size)]
        return r
    for (prefix, level, max_size), want in TALLIES.items():
        got = Counter(run_of(d, level, max_size)["size"] for d in docs if d["name"].startswith(prefix))
        assert dict(got) == want, (prefix, level, max_size, dict(got))
    for (name, level, max_size), want in TRIPLES.items():
        (d,) = [d for d in docs if d["name"] == name]
        r = run_of(d, level, max_size)
        assert (r["size"], r["count"], r["first"]) == want, (name, level, r)
    doc = {"source": "rate_host_batch on every k-subset of the empty cells (make_backdoor_cases.py); a board or grid "
                     "byte is one hex digit; cover: 21 hex digits, cell c = bit c",
           "cases": docs}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(docs)} cases -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
