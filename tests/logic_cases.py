"""The named techniques' definition in plain Python, and the
states the logic tests share.  Independent of csrc/logic.h: per-cell candidate
masks (bit d-1 = digit d); N, H, L, dead and the units are rate_cases.py's, the
Hall step is written out below as the text states it.

    step, open, left, marks = logic(board, start, ladder)

A ladder step's closure is computed on the closure of the step before: every
rule is monotone and every step's rule set holds the one before, so that is
the fixpoint the start state would reach as well.

tests/golden/make_logic_cases.py records logic(...) at the default ladder in
tests/golden/logic_cases.json (names and steps) and logic_cases.npz (open,
left, start, marks); the tests compare the host build of logic.h and
the GPU against that file.
"""
import json
import os
from itertools import combinations

import numpy as np

import rate_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1   # SDK_INVALID
NOT_RUN = -2   # SDK_LOGIC_NOT_RUN
MAX_STEPS = 8
ALL = 0x1FF
N, H, L, S2, S3, S4, F2, F3, F4 = 1, 2, 4, 8, 16, 32, 64, 128, 256
NHL = N | H | L
DEFAULT_LADDER = [N, N | H, NHL, NHL | S2, NHL | S2 | S3 | S4, NHL | S2 | S3 | S4 | F2, ALL]
# the other ladders the tests run
LADDERS = ([NHL | F2 | F3 | F4], [N, N | S4, N | S4 | F4], [N | H, ALL])
GRADE_NAMES = ["dead", "singles", "hidden singles", "locked candidates", "pairs", "triples / quads", "X-wing",
               "swordfish / jellyfish", "beyond"]
POP = [bin(v).count("1") for v in range(512)]


def ladder_ok(ladder):
    """1..8 masks inside 0x1FF, each with N, each a proper superset of the one before."""
    if not 1 <= len(ladder) <= MAX_STEPS:
        return False
    prev = 0
    for m in ladder:
        if m & ~ALL or not m & N or m == prev or m & prev != prev:
            return False
        prev = m
    return True


def hall(rows, k):
    """The Hall step of size k on nine row sets: (dead, clear[9]), clear[i] the
    elements that leave row i.  (A row larger than k lies in no subset whose
    union has k elements or fewer: only the others are combined.)"""
    clear = [0] * 9
    small = [i for i in range(9) if POP[rows[i]] <= k]
    for I in combinations(small, k):
        u = 0
        for i in I:
            u |= rows[i]
        if POP[u] < k:
            return True, clear
        if POP[u] == k:
            for i in range(9):
                if i not in I:
                    clear[i] |= u
    return False, clear


def rule_s(cand, k):
    """Subsets of size k: naked (cells x digits) and hidden (digits x cells) in
    every unit.  Returns (dead, changed)."""
    changed = False
    for unit in R.UNITS:
        dead, clear = hall([cand[c] for c in unit], k)
        if dead:
            return True, changed
        for i, c in enumerate(unit):
            if cand[c] & clear[i]:
                cand[c] &= ~clear[i]
                changed = True
        dead, clear = hall([sum((cand[c] >> d & 1) << j for j, c in enumerate(unit)) for d in range(9)], k)
        if dead:
            return True, changed
        for d in range(9):
            for j, c in enumerate(unit):
                if clear[d] >> j & 1 and cand[c] >> d & 1:
                    cand[c] &= ~(1 << d)
                    changed = True
    return False, changed


def rule_f(cand, k):
    """Fish of size k: per digit, rows x columns and columns x rows."""
    changed = False
    for d in range(9):
        for lines in (R.ROWS, R.COLS):
            dead, clear = hall([sum((cand[c] >> d & 1) << j for j, c in enumerate(line)) for line in lines], k)
            if dead:
                return True, changed
            for i, line in enumerate(lines):
                for j, c in enumerate(line):
                    if clear[i] >> j & 1 and cand[c] >> d & 1:
                        cand[c] &= ~(1 << d)
                        changed = True
    return False, changed


HALL_RULES = ((S2, rule_s, 2), (S3, rule_s, 3), (S4, rule_s, 4), (F2, rule_f, 2), (F3, rule_f, 3), (F4, rule_f, 4))


def closure(cand, rules):
    """The rules of the mask `rules` on `cand` in place until nothing changes
    or the state is dead.  Returns dead."""
    while True:
        if R.dead(cand):
            return True
        changed = False
        for bit, rule in ((N, R.rule_n), (H, R.rule_h), (L, R.rule_l)):
            if rules & bit and rule(cand):
                changed = True
                if R.dead(cand):
                    return True
        if changed:
            continue  # (the Hall steps are only worth their cost on a state the cheaper rules are done with)
        for bit, rule, k in HALL_RULES:
            if rules & bit:
                dead, ch = rule(cand, k)
                if dead:
                    return True
                if ch:
                    changed = True
                    break
        if not changed:
            return False


def start_state(board, start):
    """A board's own start state ANDed with the pencil marks; None for either."""
    cand = R.start(board) if board is not None else [ALL] * 81
    if start is not None:
        cand = [m & int(s) for m, s in zip(cand, start)]
    return cand


def logic(board=None, start=None, ladder=DEFAULT_LADDER):
    """(step, open[8], left[8], marks[81]) of one state, by the text."""
    assert ladder_ok(ladder) and (board is not None or start is not None)
    if (board is not None and any(int(v) > 9 for v in board)) or (start is not None and any(int(s) & ~ALL for s in start)):
        return INVALID, [INVALID] * 8, [INVALID] * 8, [0] * 81
    steps = len(ladder)
    opens, left = [NOT_RUN] * 8, [NOT_RUN] * 8
    cand = start_state(board, start)
    for j, rules in enumerate(ladder):
        if closure(cand, rules):
            for k in range(j, steps):
                opens[k] = left[k] = -1
            return 0, opens, left, [0] * 81
        if R.solved(cand):
            for k in range(j, steps):
                opens[k], left[k] = 0, 81
            return j + 1, opens, left, cand
        opens[j] = sum(not R.single(m) for m in cand)
        left[j] = sum(POP[m] for m in cand)
    return steps + 1, opens, left, cand


def first_change(start_left, left):
    """The first step (1-based) whose `left` differs from the step before (the
    start state's count before step 1); None when none does."""
    prev = start_left
    for j, v in enumerate(left):
        if v == NOT_RUN:
            break
        if v != prev:
            return j + 1
        prev = v
    return None


# ------------------------------------------------------------ planted states
KINDS = ("naked", "hidden", "row_fish", "col_fish")


def pattern_step(kind, k):
    """The default ladder's step that holds the pattern's rule."""
    return (4 if k == 2 else 5) if kind in ("naked", "hidden") else (6 if k == 2 else 7)


def solution_grid(rng):
    """A shuffled solution grid: the band pattern under a random symmetry."""
    import symmetry_cases as S
    base = np.array([(3 * (r % 3) + r // 3 + c) % 9 + 1 for r in range(9) for c in range(9)], dtype=np.uint8)
    return S.image_board(base, S.random_symmetry(rng))


def planted(kind, k, seed):
    """An (empty board, start) pair around a shuffled solution grid: every cell
    keeps its solution digit and every other digit with probability 0.8, and
    one pattern of `kind` and size k is planted.  Returns start[81]."""
    rng = np.random.default_rng([seed, KINDS.index(kind), k])
    g = solution_grid(rng)
    start = [(1 << (int(v) - 1)) | sum(1 << d for d in range(9) if rng.random() < 0.8) for v in g]
    if kind in ("naked", "hidden"):
        unit = R.UNITS[int(rng.integers(27))]
        cells = [unit[i] for i in sorted(rng.choice(9, k, replace=False))]
        digits = sum(1 << (int(g[c]) - 1) for c in cells)
        for c in unit:
            if kind == "naked" and c in cells:
                start[c] = digits            # k cells, the same k digits
            elif kind == "hidden" and c not in cells:
                start[c] &= ~digits          # k digits, places in k cells only
    else:
        d = int(rng.integers(9))
        lines, cross = (R.ROWS, R.COLS) if kind == "row_fish" else (R.COLS, R.ROWS)
        chosen = sorted(rng.choice(9, k, replace=False))
        keep = {c for i in chosen for c in lines[i] if g[c] == d + 1}   # the solution's own places
        keep_cross = {j for j in range(9) if keep & set(cross[j])}
        for i in chosen:
            for j, c in enumerate(lines[i]):
                if j not in keep_cross:
                    start[c] &= ~(1 << d)
    return [int(m) for m in start]


# ------------------------------------------------------------ Hall violations
def _full():
    return [ALL] * 81


def violations():
    """name -> (start[81], ladders): states with a pigeonhole violation that N,
    H and L do not see, and the ladders they are run under (the last one holds
    the rule that sees it)."""
    out = {}
    s = _full()
    s[0], s[1], s[2], s[3] = 0b011, 0b110, 0b101, 0b111   # four cells of row 0 share three digits
    out["four_cells_three_digits_row"] = (s, ([NHL], [N, N | S2], [N, N | S4]))
    s = _full()
    s[0], s[9], s[27], s[54] = 0b011, 0b110, 0b101, 0b111  # ... of column 0
    out["four_cells_three_digits_column"] = (s, ([NHL], [N, N | S2], [N, N | S4]))
    s = _full()
    for c in R.BOXES[4]:
        if c not in (30, 50):
            s[c] &= ~0b111000                              # digits 4, 5, 6 have two places in box 4
    out["three_digits_two_places_box"] = (s, ([NHL], [N, N | S2], [N | H, N | H | S3]))
    s = _full()
    for r in (0, 3, 6):
        for c in range(9):
            if c not in (0, 4):
                s[9 * r + c] &= ~(1 << 6)                  # digit 7 in rows 0, 3, 6: columns 0 and 4 only
    out["three_rows_two_columns_fish"] = (s, ([NHL], [NHL | S2 | S3 | S4], [NHL, NHL | F3]))
    s = _full()
    s[0] = s[1] = 0b1                                      # two cells of a row with the one digit: N sees it
    out["two_cells_one_digit"] = (s, ([N], [N | S2]))
    return out


# ------------------------------------------------------------------ fixture
def marks_text(marks):
    return R.marks_text(marks)


def load_fixture():
    """tests/golden/logic_cases.json and logic_cases.npz as a dict: names, boards (n, 81) uint8,
    start (n, 81) uint16, has_board / has_start (n,) bool, kind (n,) of str
    ("" for the rate fixture's boards), k (n,), step (n,), open (n, 8), left
    (n, 8), marks (n, 81) uint16 at the default ladder; and violations: a list
    of (name, start (81,) uint16, ladder, step, open, left, marks)."""
    with open(os.path.join(HERE, "golden", "logic_cases.json")) as f:
        doc = json.load(f)
    cases = doc["cases"]
    assert doc["ladder"] == DEFAULT_LADDER
    z = np.load(os.path.join(HERE, "golden", "logic_cases.npz"))
    assert len(z["start"]) == len(z["marks"]) == len(z["open"]) == len(z["left"]) == len(cases)
    rate_names, rate_boards = R.load_fixture()[:2]
    board_of = dict(zip(rate_names, rate_boards))  # a state without pencil marks is a board of rate_cases.json
    out = {
        "names": [c["name"] for c in cases],
        "boards": np.array([np.zeros(81, np.uint8) if "kind" in c else board_of[c["name"]] for c in cases], dtype=np.uint8),
        "start": np.array(z["start"], dtype=np.uint16),
        "has_board": np.array(["kind" not in c for c in cases]),
        "has_start": np.array(["kind" in c for c in cases]),
        "kind": np.array([c.get("kind", "") for c in cases]),
        "k": np.array([c.get("k", 0) for c in cases]),
        "step": np.array([c["step"] for c in cases], dtype=np.int32),
        "open": np.array(z["open"], dtype=np.int32),
        "left": np.array(z["left"], dtype=np.int32),
        "marks": np.array(z["marks"], dtype=np.uint16),
        "violations": [(v["name"], np.array(R.marks_from_text(v["start"]), dtype=np.uint16), run["ladder"], run["step"],
                        run["open"], run["left"], np.array(R.marks_from_text(run["marks"]), dtype=np.uint16))
                       for v in doc["violations"] for run in v["runs"]],
    }
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
