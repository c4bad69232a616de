"""The solving path's definition in plain Python, and the
states the path tests share.  Independent of csrc/path.h: per-cell candidate
masks (bit d-1 = digit d); the units, dead and solved are rate_cases.py's, the
rule masks and the start state logic_cases.py's; firings, their classes and
the schedule are written out below as the text states them.

    events, status, rounds, hist, marks = path(board, start, rules, max_rounds)

An event is the tuple (round, cls, m, I, u, removed, left, contradiction), the
columns of BatchSolver.path; a board's events are sorted.

tests/golden/make_path_cases.py records path(...) in tests/golden/
path_cases.json (names, masks, facts) and path_cases.npz (events); the tests
compare the host build of path.h and the GPU against that file.
"""
import json
import os
from itertools import combinations

import numpy as np

import logic_cases as G
import rate_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
DEAD, SOLVED, STUCK, LIMITED, INVALID = 0, 1, 2, 3, -1
ALL = G.ALL
CLASS_NAMES = ("N", "H", "L", "S2", "S3", "S4", "F2", "F3", "F4")
CLASS_SIZE = (1, 1, 0, 2, 3, 4, 2, 3, 4)
MASKS = (ALL, G.N | G.H | G.L, G.N | G.S4 | G.F4, G.N | G.L)   # the fixture's rule masks
POP = G.POP
LINES = R.ROWS + R.COLS
COLUMNS = ("round", "cls", "m", "I", "u", "removed", "left", "contradiction")


def class_matrices(c):
    """The matrices the Hall class c runs on."""
    return range(45, 72) if c == 0 else range(18, 45) if c == 1 else range(18, 72) if c < 6 else range(0, 18)


def places(m, i, j):
    """(cell, digit 0..8) of element j of row i of matrix m."""
    kind, idx = divmod(m, 9)
    if kind == 0:
        return 9 * i + j, idx
    if kind == 1:
        return 9 * j + i, idx
    if kind < 5:
        return R.UNITS[9 * (kind - 2) + idx][j], i
    return R.UNITS[9 * (kind - 5) + idx][i], j


def matrix(cand, m):
    return [sum((cand[c] >> d & 1) << j for j in range(9) for c, d in (places(m, i, j),)) for i in range(9)]


def hall_removals(m, I, u):
    """The (cell, digit) pairs the firing's action names: u in every row outside I."""
    return [places(m, i, j) for i in range(9) if not I >> i & 1 for j in range(9) if u >> j & 1]


def l_removals(dir_, d, line, box):
    meet = set(LINES[line]) & set(R.BOXES[box])
    rest = (set(LINES[line]) if dir_ == 0 else set(R.BOXES[box])) - meet
    return [(c, d) for c in sorted(rest)]


def event_removals(ev):
    """The (cell, digit) pairs an event's action names; it needs the event alone."""
    _, _, m, I, u, _, _, contradiction = ev
    if contradiction:
        return []
    if m >= 72:
        return l_removals(m - 72, I.bit_length() - 1, u & 31, u >> 5)
    return hall_removals(m, I, u)


def count_removed(cand, pairs):
    return sum(cand[c] >> d & 1 for c, d in pairs)


def hall_firings(cand, c):
    """(firings [(m, I, u, removed)], violations [(m, I, u)]) of the Hall class c."""
    k = CLASS_SIZE[c]
    fire, bad = [], []
    for m in class_matrices(c):
        rows = matrix(cand, m)
        # (a row larger than k lies in no subset whose union has k elements or fewer)
        for sub in combinations([i for i in range(9) if POP[rows[i]] <= k], k):
            u = 0
            for i in sub:
                u |= rows[i]
            I = sum(1 << i for i in sub)
            if POP[u] < k:
                bad.append((m, I, u))
            elif POP[u] == k:
                n = count_removed(cand, hall_removals(m, I, u))
                if n:
                    fire.append((m, I, u, n))
    return fire, bad


def l_firings(cand):
    fire = []
    for d in range(9):
        for box in range(9):
            for line in range(18):
                meet = set(LINES[line]) & set(R.BOXES[box])
                if len(meet) != 3 or not any(cand[c] >> d & 1 for c in meet):
                    continue
                for dir_, here in ((0, R.BOXES[box]), (1, LINES[line])):
                    if not any(cand[c] >> d & 1 for c in here if c not in meet):
                        n = count_removed(cand, l_removals(dir_, d, line, box))
                        if n:
                            fire.append((72 + dir_, 1 << d, line | box << 5, n))
    return fire


def path(board=None, start=None, rules=ALL, max_rounds=0):
    """(events, status, rounds, hist[9], marks[81]) of one state, by the text."""
    assert rules & G.N and not rules & ~ALL and (board is not None or start is not None)
    if (board is not None and any(int(v) > 9 for v in board)) or (start is not None and any(int(s) & ~ALL for s in start)):
        return [], INVALID, 0, [0] * 9, [0] * 81
    cand = G.start_state(board, start)
    events, hist, r = [], [0] * 9, 0
    while True:
        left = sum(POP[m] for m in cand)
        if R.dead(cand):
            m, I = min((m, 1 << i) for m in range(18, 72) for i, row in enumerate(matrix(cand, m)) if row == 0)
            events.append((r + 1, 0, m, I, 0, 0, left, 1))
            return sorted(events), DEAD, r, hist, [0] * 81
        if R.solved(cand):
            return sorted(events), SOLVED, r, hist, cand
        if max_rounds > 0 and r == max_rounds:
            return sorted(events), LIMITED, r, hist, cand
        fired = None
        for c in range(9):
            if not rules >> c & 1:
                continue
            if c == 2:
                fire = l_firings(cand)
            else:
                fire, bad = hall_firings(cand, c)
                if bad and c >= 3:
                    m, I, u = min(bad)
                    events.append((r + 1, c, m, I, u, 0, left, 1))
                    return sorted(events), DEAD, r, hist, [0] * 81
            if fire:
                fired = c
                break
        if fired is None:
            return sorted(events), STUCK, r, hist, cand
        r += 1
        new = list(cand)
        for m, I, u, n in fire:
            for c, d in event_removals((r, fired, m, I, u, n, 0, 0)):
                new[c] &= ~(1 << d)
        cand = new
        left = sum(POP[m] for m in cand)
        events += [(r, fired, m, I, u, n, left, 0) for m, I, u, n in fire]
        hist[fired] += len(fire)


def replay(marks, events):
    """`marks` after the actions of `events`, by the events alone."""
    out = [int(m) for m in marks]
    for ev in events:
        for c, d in event_removals(tuple(int(v) for v in ev)):
            out[c] &= ~(1 << d)
    return out


def start_marks(board, start):
    return G.start_state(board, start)


# ------------------------------------------------------------------ fixture
def load_fixture():
    """tests/golden/path_cases.json and path_cases.npz as a dict: names,
    boards (n, 81) uint8, start (n, 81) uint16, has_board / has_start (n,)
    bool, and runs: a list of dicts with rules, max_rounds, idx (the states
    run), status, rounds, hist (k, 9), marks (k, 81), offsets (k + 1,),
    events (E, 8) int32 sorted per state."""
    with open(os.path.join(HERE, "golden", "path_cases.json")) as f:
        doc = json.load(f)
    z = np.load(os.path.join(HERE, "golden", "path_cases.npz"))
    out = {
        "names": doc["names"],
        "boards": np.array(z["boards"], dtype=np.uint8),
        "start": np.array(z["start"], dtype=np.uint16),
        "has_board": np.array(z["has_board"], dtype=bool),
        "has_start": np.array(z["has_start"], dtype=bool),
        "facts": doc["facts"],
        "runs": [],
    }
    for k, run in enumerate(doc["runs"]):
        out["runs"].append({
            "rules": run["rules"], "max_rounds": run["max_rounds"],
            "idx": np.array(z[f"idx_{k}"], dtype=np.int64),
            "status": np.array(z[f"status_{k}"], dtype=np.int32),
            "rounds": np.array(z[f"rounds_{k}"], dtype=np.int32),
            "hist": np.array(z[f"hist_{k}"], dtype=np.int32),
            "marks": np.array(z[f"marks_{k}"], dtype=np.uint16),
            "offsets": np.array(z[f"offsets_{k}"], dtype=np.int64),
            "events": np.array(z[f"events_{k}"], dtype=np.int32),
        })
    for v in list(out.values()) + [a for run in out["runs"] for a in run.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def inputs(fx, idx):
    """(boards, start) of the fixture's states `idx`, None where no state has one."""
    idx = np.asarray(idx)
    return fx["boards"][idx], fx["start"][idx]
