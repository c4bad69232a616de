"""The puzzle rating's definition in plain Python, and the boards the rating
tests share.  Independent of csrc/rate.h: per-cell candidate masks (bit d-1 =
digit d), every rule as the text of DESIGN.md §14 states it, applied until
nothing changes.  The fixpoint of a rule set is unique (every rule is
monotone), so the order below is one of many that give the same answer.

    rating, open, marks = rate(board, max_level)

tests/golden/make_rate_cases.py records rate(board, 4) for its boards
in tests/golden/rate_cases.json; the tests compare the host build of rate.h
and the GPU against that file.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1   # SDK_INVALID
NOT_RUN = -2   # SDK_RATE_NOT_RUN
ALL = 0x1FF

ROWS = [[9 * r + c for c in range(9)] for r in range(9)]
COLS = [[9 * r + c for r in range(9)] for c in range(9)]
BOXES = [[9 * (3 * (b // 3) + i) + 3 * (b % 3) + j for i in range(3) for j in range(3)] for b in range(9)]
UNITS = ROWS + COLS + BOXES
PEERS = [sorted({x for u in UNITS if c in u for x in u} - {c}) for c in range(81)]
# (box, line) pairs that meet in three cells: I, box \ I, line \ I
LOCKED = []
for _box in BOXES:
    for _line in ROWS + COLS:
        _meet = [c for c in _box if c in _line]
        if len(_meet) == 3:
            LOCKED.append((_meet, [c for c in _box if c not in _meet], [c for c in _line if c not in _meet]))


def start(board):
    return [1 << (int(v) - 1) if v else ALL for v in board]


def dead(cand):
    if any(m == 0 for m in cand):
        return True
    for unit in UNITS:
        seen = 0
        for c in unit:
            seen |= cand[c]
        if seen != ALL:
            return True
    return False


def single(m):
    return m != 0 and m & (m - 1) == 0


def solved(cand):
    return all(single(m) for m in cand) and not dead(cand)


def rule_n(cand):
    changed = False
    for c in range(81):
        m = cand[c]
        if single(m):
            for p in PEERS[c]:
                if cand[p] & m:
                    cand[p] &= ~m
                    changed = True
    return changed


def rule_h(cand):
    changed = False
    for unit in UNITS:
        for d in range(9):
            cells = [c for c in unit if cand[c] >> d & 1]
            if len(cells) == 1 and cand[cells[0]] != 1 << d:
                cand[cells[0]] = 1 << d
                changed = True
    return changed


def rule_l(cand):
    changed = False
    for meet, box_rest, line_rest in LOCKED:
        for d in range(9):
            bit = 1 << d
            if not any(cand[c] & bit for c in meet):
                continue
            for here, there in ((box_rest, line_rest), (line_rest, box_rest)):
                if not any(cand[c] & bit for c in here):
                    for c in there:
                        if cand[c] & bit:
                            cand[c] &= ~bit
                            changed = True
    return changed


def rule_t(cand):
    changed = False
    for c in range(81):
        for d in range(9):
            m = cand[c]
            if m >> d & 1 and m != 1 << d:  # two or more candidates, d among them
                trial = list(cand)
                trial[c] = 1 << d
                if closure(trial, 3):
                    cand[c] &= ~(1 << d)
                    changed = True
    return changed


RULES = {1: (rule_n,), 2: (rule_n, rule_h), 3: (rule_n, rule_h, rule_l), 4: (rule_n, rule_h, rule_l, rule_t)}


def closure(cand, level):
    """The level's rules on `cand` in place until nothing changes or the state
    is dead.  Returns dead(cand)."""
    while True:
        if dead(cand):
            return True
        changed = False
        for rule in RULES[level]:
            # (a trial is only worth its cost on a state the cheaper rules are done with)
            if rule is rule_t and changed:
                break
            if rule(cand):
                changed = True
                if dead(cand):
                    return True
        if not changed:
            return False


def rate(board, max_level=4):
    """(rating, open[4], marks[81]) of one board of 81 values, by the text."""
    board = [int(v) for v in board]
    if any(v > 9 for v in board):
        return INVALID, [INVALID] * 4, [0] * 81
    opens = [NOT_RUN] * 4
    rating, marks = max_level + 1, None
    for level in range(1, max_level + 1):
        cand = start(board)
        if closure(cand, level):
            rating, marks = 0, [0] * 81
            for k in range(level, max_level + 1):
                opens[k - 1] = -1
            break
        opens[level - 1] = sum(not single(m) for m in cand)
        marks = cand
        if solved(cand):
            rating = level
            for k in range(level, max_level + 1):
                opens[k - 1] = 0
            break
    return rating, opens, marks


# ------------------------------------------------------------------ boards
def digits(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


# name -> (board, rating, open) at max_level 4: the facts DESIGN.md §14 lists
NAMED = {
    "empty": ("0" * 81, 5, [81, 81, 81, 81]),
    "proper_undecided": ("1.......2.9.4...5...6...7...5.9.3.......7.......85..4.7.....6...3...9.8...2.....1".replace(".", "0"),
                         5, [60, 60, 60, 60]),
    "two_ones_in_a_row": ("11" + "0" * 79, 0, [-1, -1, -1, -1]),
    "row_without_a_place": ("123456780" + "000000009" + "0" * 63, 0, [-1, -1, -1, -1]),
    "one_given_of_a_seed_changed": ("000600040210030004037040810800000000900050200000074005080703009000000000150000000",
                               0, [-1, -1, -1, -1]),
    "dead_at_level_3": ("004030002200071005000002060091000000507090300002004000085000200070000009000006040",
                        0, [56, 54, -1, -1]),
    "dead_at_level_2": ("000400320010000007000060008007086000080500009001000600400000003070300005206009070",
                        0, [57, -1, -1, -1]),
    "undecided_trials_removed": ("074006000000000230800005009590070002700800300060000000080400510300000000000090043",
                                 5, [57, 52, 52, 30]),
}


def corpus(name):
    """The boards of a data file of the package (hard17_classes.txt,
    hard_search_seeds.txt), read here so that this module needs no torch."""
    path = os.path.join(os.path.dirname(HERE), "sudoku_solver_distributed_amd", "data", name)
    with open(path) as f:
        return [ln.split()[0] for ln in f if ln.strip() and not ln.startswith("#")]


def puzzles_30(n=60):
    z = np.load(os.path.join(HERE, "golden", "random_generated.npz"))
    return ["".join(str(int(v)) for v in b) for b in z["puzzles_30"][:n]]


def load_fixture():
    """tests/golden/rate_cases.json as (names, boards (n, 81) uint8, rating (n,),
    open (n, 4), marks (n, 81) uint16)."""
    with open(os.path.join(HERE, "golden", "rate_cases.json")) as f:
        doc = json.load(f)
    cases = doc["cases"]
    return ([c["name"] for c in cases],
            np.array([digits(c["board"]) for c in cases], dtype=np.uint8),
            np.array([c["rating"] for c in cases], dtype=np.int32),
            np.array([c["open"] for c in cases], dtype=np.int32),
            np.array([marks_from_text(c["marks"]) for c in cases], dtype=np.uint16))


def marks_text(marks):
    """81 candidate masks as 243 hex digits (three per cell)."""
    return "".join("%03x" % m for m in marks)


def marks_from_text(s):
    return [int(s[3 * i:3 * i + 3], 16) for i in range(81)]


def at_level(rating, opens, m):
    """What the definition makes of a board's max_level-4 answer at max_level
    m: (rating, open, marks_known).  marks_known is False where the marks are
    those of closure_m, which the max_level-4 answer does not hold."""
    rating, opens = int(rating), [int(v) for v in opens]
    if rating == INVALID:
        return rating, opens, True
    o = opens[:m] + [NOT_RUN] * (4 - m)
    if 1 <= rating <= m:
        return rating, o, True
    if -1 in opens[:m]:
        return 0, o, True
    return m + 1, o, m == 4
