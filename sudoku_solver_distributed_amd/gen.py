"""Drop-in for the reference's ``gen.py`` plus the batch workloads.

* ``solve_sudoku(board)``      -- gen.py:6-28: same signature and result (the
  board is filled in place with the walk's first solution, True/False
  returned); the walk itself runs in the HIP kernel.
* ``generate_sudoku(empty)``   -- gen.py:31-52: same random-call sequence on
  the ``random`` module, so under the same ``random.seed`` it returns the same
  puzzle as the reference.
* ``generate_batch(n, empty, seed)`` -- n calls of generate_sudoku under one
  seed, with every fill solved in ONE GPU batch (identical boards).
* ``hard17_batch(n, seed)``    -- the benchmark's hard set: 17-clue boards with
  a unique solution, made by validity-preserving symmetries (digit relabeling,
  row/column permutations inside bands/stacks, band/stack permutations,
  transposition) of the 80 certified isomorphism classes in
  data/hard17_classes.txt (scripts/make_hard17.py).
* ``hard_search_batch(n, seed)`` -- the search-heavy set: the same symmetries
  applied to 256 minimal puzzles that need real search (data/).
* ``unique_batch(n, empty_boxes, seed)`` -- proper puzzles: boards with exactly
  one solution (minimal ones by default), certified removal by removal by the
  GPU's completion count, or by one BatchSolver.minimize call with fused=True
  (library extension; the reference's generate_sudoku erases cells blindly and
  its 55-empty boards are almost never unique).
* ``random_grids(n, seed)`` -- n random full grids from the GPU's seeded
  randomised search (BatchSolver.random_grids; library extension), with no
  host loop; ``unique_batch(..., grids="random")`` builds its puzzles on them.
* ``make_unique(boards)`` -- boards with several completions repaired into
  proper puzzles: givens added where the GPU's exact candidates
  (BatchSolver.candidates; library extension) leave a cell open.
* ``exchange(puzzles)`` / ``exchange_search(seeds, target)`` -- the {-1, +1}
  clue-exchange neighbours of proper puzzles, and the breadth-first search
  over isomorphism classes built on them, by the GPU's unique candidates
  (BatchSolver.unique_candidates; library extension).
* ``apply_symmetry(boards, sym)`` / ``class_ids(boards)`` -- the symmetry
  group in numbers and the isomorphism class of every board, by the GPU's
  canonical form (BatchSolver.canonical; library extension).
* ``min_hitting_clues(grids)`` / ``smallest_sub_puzzles(puzzles)`` /
  ``neighbourhood(puzzles, d)`` -- the hitting number of a grid's unavoidable
  sets, the smallest proper puzzles inside a puzzle and the {-d, +d}
  neighbours, by the GPU's hitting sets (BatchSolver.hitting_sets /
  sub_puzzles; library extension).
* ``hint(boards)`` / ``explain(events)`` / ``apply_events(marks, events)`` /
  ``technique_counts(boards)`` -- the easiest deductions available now, one
  English line an event, the replay of events on pencil marks and the events
  per technique, by the GPU's solving path (BatchSolver.path; library
  extension).
"""
from __future__ import annotations

import os
import random as _random
import sys
from typing import List, Optional

import numpy as np
import torch

from ._lib import SudokuHipError
from .solver import SDK_SOLVED, as_boards, get_solver
from .sudoku import Sudoku

# 17-clue boards with exactly one solution (certified by
# tests/test_oracle.py::test_seeds_unique with the oracle's counter); the last
# one is the "brute-force resistant" board whose solution's first row is
# 987654321 -- a worst case for the walk.  Through round 3 hard17_batch made
# every benchmark board from these six (six isomorphism classes); they now
# seed the corpus search (scripts/make_hard17.py -> data/hard17_classes.txt),
# and bench.py also reports a search-heavy side set (hard_search_batch).
SEEDS_17 = (
    "000000010400000000020000000000050407008000300001090000300400200050100000000806000",
    "000000010400000000020000000000050604008000300001090000300400200050100000000807000",
    "000000012000035000000600070700000300000400800100000000000120000080000040050000600",
    "000000012003600000000007000410020000000500300700000600280000040000300500000000000",
    "000000012008030000000000040120500000000004700060000000507000300000620000000100000",
    "000000000000003085001020000000507000004000100090000000500000073002010000000040009",
)
PATHOLOGICAL = SEEDS_17[5]
# a 21-clue unique board that naked + hidden singles cannot finish: needs
# real search under either walk order (frontier-split tests / latency bench)
SEARCH_HEAVY = "800000000003600000070090200050007000000045700000100030001000068008500010090000400"


def _board_from_flat(flat) -> List[List[int]]:
    flat = list(flat)
    return [flat[r * 9:(r + 1) * 9] for r in range(9)]


def solve_sudoku(board) -> bool:
    """gen.py:6-28 on the GPU: fills `board` (9x9 list of lists) in place."""
    sols, st = get_solver().solve(as_boards(board))
    if int(st[0].item()) != SDK_SOLVED:
        return False
    flat = sols[0].cpu().tolist()
    for r in range(9):
        board[r][:] = flat[r * 9:(r + 1) * 9]
    return True


def _draw_diagonal(rng) -> List[List[int]]:
    # gen.py:33-40
    board = [[0] * 9 for _ in range(9)]
    for n in range(0, 9, 3):
        nums = rng.sample(range(1, 10), 9)
        for i in range(3):
            for j in range(3):
                board[n + i][n + j] = nums.pop()
    return board


def _draw_removals(rng, empty_boxes, full_mask) -> List[int]:
    # gen.py:46-50, on the zero pattern only (the walk fills every cell of a
    # diagonal-seeded board, so the pattern does not depend on the digits)
    zero = [not f for f in full_mask]
    out = []
    for _ in range(empty_boxes):
        row, col = rng.randint(0, 8), rng.randint(0, 8)
        while zero[row * 9 + col]:
            row, col = rng.randint(0, 8), rng.randint(0, 8)
        zero[row * 9 + col] = True
        out.append(row * 9 + col)
    return out


def generate_sudoku(empty_boxes=0, rng=None) -> Sudoku:
    """gen.py:31-52 (uses the global `random` module unless rng is given)."""
    rng = rng if rng is not None else _random
    board = _draw_diagonal(rng)
    solve_sudoku(board)
    full = [v != 0 for row in board for v in row]
    for cell in _draw_removals(rng, empty_boxes, full):
        board[cell // 9][cell % 9] = 0
    return Sudoku(board)


def generate_batch(n: int, empty_boxes: int, seed: Optional[int] = None, device=None,
                   return_solutions: bool = False):
    """Exactly [generate_sudoku(empty_boxes) for _ in range(n)] after
    random.seed(seed), with the n fills solved as one GPU batch.
    Returns a (n, 81) uint8 tensor on the device (and the full grids)."""
    rng = _random.Random(seed)
    # The reference interleaves per board: 3 samples, solve, removals.  The
    # removal draws depend only on the zero pattern, so drawing board by board
    # here yields the same sequence as long as every fill succeeds (checked).
    diag = np.zeros((n, 81), dtype=np.uint8)
    removals = []
    for k in range(n):
        b = _draw_diagonal(rng)
        diag[k] = np.asarray(b, dtype=np.uint8).reshape(81)
        removals.append(_draw_removals(rng, empty_boxes, [True] * 81))
    solver = get_solver(device)
    full, st = solver.solve(torch.from_numpy(diag))
    if not bool((st == SDK_SOLVED).all().item()):
        raise RuntimeError("a diagonal-seeded board had no completion; "
                           "generate these boards one by one with generate_sudoku")
    puzzles = full.clone()
    if empty_boxes:
        idx = torch.as_tensor(np.asarray(removals, dtype=np.int64).reshape(n, empty_boxes),
                              device=puzzles.device)
        puzzles.scatter_(1, idx, 0)
    return (puzzles, full) if return_solutions else puzzles


def random_grids(n: int, seed: Optional[int] = None, device=None) -> torch.Tensor:
    """n random full grids as a (n, 81) uint8 device tensor: the GPU's seeded
    randomised search on the empty board (BatchSolver.random_grids, keys
    0..n-1; library extension, no reference counterpart -- the reference's
    generate_sudoku is still generate_batch).  Every valid grid can come out;
    they are not equally likely.  seed=None draws a seed from `random`."""
    if seed is None:
        seed = _random.getrandbits(64)
    return get_solver(device).random_grids(n, seed)


def _full_grids(n: int, seed: Optional[int], device, grids: str) -> torch.Tensor:
    if grids == "walk":
        return generate_batch(n, 0, seed, device=device)
    if grids == "random":
        return random_grids(n, seed, device=device)
    raise ValueError('grids must be "walk" or "random"')


def unique_batch(n: int, empty_boxes: int = 81, seed: Optional[int] = None, device=None,
                 return_solutions: bool = False, distinct: bool = False, fused: bool = False, grids: str = "walk"):
    """n puzzles with exactly ONE solution, as a (n, 81) uint8 device tensor
    (and their full grids).  Library extension, no reference counterpart.

    1. full = generate_batch(n, 0, seed): the full grids.
    2. order = argsort(default_rng(seed).random((n, 81)), axis=1): each
       board's own random order of its 81 cells.
    3. puzzle = full; for round t = 0..80, every board that still has fewer
       than `empty_boxes` empties tries its puzzle with cell order[i, t]
       erased; ONE count_solutions(trials, limit=2) call certifies the whole
       batch, and a removal is kept where the count is 1.

    Every board has one completion (its full grid) and at most `empty_boxes`
    empties.  With empty_boxes=81 every puzzle is minimal: each cell was tried
    once, and a removal that loses uniqueness loses it under any further
    removals too.

    distinct=True keeps only the first puzzle of every isomorphism class
    (class_ids), in the batch's order, and the matching rows of the full
    grids: fewer than n boards when two puzzles are symmetry images of each
    other.

    fused=True: step 3's 81 rounds as ONE BatchSolver.minimize(full, order,
    max_empty=empty_boxes) call (library extension): the same
    full grids and orders, and bit for bit the same puzzles.

    grids="random": step 1 takes full = random_grids(n, seed) instead, random
    full grids made on the GPU without a host loop; every
    later step is the same.  "walk" is generate_batch's grids, as before."""
    solver = get_solver(device)
    full = _full_grids(n, seed, device, grids)
    order = np.argsort(np.random.default_rng(seed).random((n, 81)), axis=1)
    if fused:
        puzzle = full.clone()
        if n and empty_boxes > 0:
            turns = torch.as_tensor(order.astype(np.uint8), device=full.device)
            puzzle, status = solver.minimize(full, turns, max_empty=min(int(empty_boxes), 81))
            if not bool((status == 1).all().item()):
                raise RuntimeError("a full grid was not reported as its own one completion")
        if distinct and n:
            first = torch.sort(class_ids(puzzle, device=device)[2]).values
            puzzle, full = puzzle[first], full[first]
        return (puzzle, full) if return_solutions else puzzle
    order = torch.as_tensor(order, dtype=torch.int64, device=full.device)
    puzzle = full.clone()
    empties = torch.zeros(n, dtype=torch.int64, device=full.device)
    zero = torch.zeros((), dtype=torch.uint8, device=full.device)
    for t in range(81 if n and empty_boxes > 0 else 0):
        cell = order[:, t:t + 1]
        live = (empties < empty_boxes).unsqueeze(1)
        trial = puzzle.scatter(1, cell, torch.where(live, zero, puzzle.gather(1, cell)))
        keep = live & (solver.count_solutions(trial, limit=2) == 1).unsqueeze(1)
        puzzle = torch.where(keep, trial, puzzle)
        empties += keep.squeeze(1)
    if distinct and n:
        first = torch.sort(class_ids(puzzle, device=device)[2]).values
        puzzle, full = puzzle[first], full[first]
    return (puzzle, full) if return_solutions else puzzle


def rated_batch(n: int, seed: Optional[int] = None, ratings=None, device=None, return_solutions: bool = False,
                grids: str = "walk"):
    """unique_batch(n, seed=seed) with every puzzle's rating
    (BatchSolver.rate, max_level 4: 1 naked singles .. 4 trial eliminations,
    5 not decided by them; never 0, every puzzle has a completion):
    (puzzles (k, 81) uint8, ratings (k,) int32[, full grids (k, 81)]), device
    tensors.  ratings: keep only the puzzles whose rating is in this
    collection, in the batch's order (k <= n); None keeps all n.  grids:
    unique_batch's.  Library extension, no reference counterpart."""
    puzzles, full = unique_batch(n, seed=seed, device=device, return_solutions=True, grids=grids)
    rating = get_solver(device).rate(puzzles)
    if ratings is not None:
        keep = torch.isin(rating, torch.as_tensor(sorted(int(r) for r in ratings), dtype=torch.int32, device=rating.device))
        puzzles, full, rating = puzzles[keep], full[keep], rating[keep]
    return (puzzles, rating, full) if return_solutions else (puzzles, rating)


# what BatchSolver.logic's step says at the default ladder: GRADE_NAMES[step]
GRADE_NAMES = ("dead", "singles", "hidden singles", "locked candidates", "pairs", "triples / quads", "X-wing",
               "swordfish / jellyfish", "beyond")


def grade(boards, device=None) -> torch.Tensor:
    """The first step of the default ladder that solves every board
    (BatchSolver.logic): 1 singles .. 7 swordfish / jellyfish, 8 beyond them,
    0 no completion, as an int32 (n,) device tensor; grade_names() gives the
    names.  Library extension, no reference counterpart."""
    return get_solver(device).logic(boards)


def grade_names(steps) -> List[str]:
    """GRADE_NAMES for grade()'s steps ("invalid" for SDK_INVALID)."""
    return [GRADE_NAMES[s] if 0 <= s < len(GRADE_NAMES) else "invalid" for s in torch.as_tensor(steps).cpu().tolist()]


# ---- the solving path (BatchSolver.path)
# what an event's class says: PATH_CLASS_NAMES[cls]
PATH_CLASS_NAMES = ("naked single", "hidden single", "locked candidates", "pair", "triple", "quad", "X-wing", "swordfish",
                    "jellyfish")
_UNIT_KINDS = ("row", "column", "box")


def path_class_names(classes) -> List[str]:
    """PATH_CLASS_NAMES for the class column of BatchSolver.path's events."""
    return [PATH_CLASS_NAMES[c] for c in torch.as_tensor(classes).cpu().tolist()]


def hint(boards, start=None, rules: int = 0x1FF, device=None):
    """The easiest deductions available now on every state: BatchSolver.path
    with max_rounds=1, (events, offsets, status).  Every event of a state is
    of one class, the lowest of `rules` that removes a candidate; a solved,
    stuck or dead state has none (a dead one its contradiction event).
    Library extension, no reference counterpart."""
    return get_solver(device).path(boards, rules=rules, start=start, max_rounds=1)


def technique_counts(boards, start=None, rules: int = 0x1FF, device=None) -> torch.Tensor:
    """How many events of every class the solving path of every state holds:
    an int32 (n, 9) device tensor (BatchSolver.path as a pure count), the
    columns PATH_CLASS_NAMES.  Library extension, no reference counterpart."""
    return get_solver(device).path(boards, rules=rules, start=start, capacity=0, return_hist=True)[-1]


def _unit_cells(t: int, u: int) -> List[int]:
    if t == 0:
        return [9 * u + k for k in range(9)]
    if t == 1:
        return [9 * k + u for k in range(9)]
    return [9 * (3 * (u // 3) + k // 3) + 3 * (u % 3) + k % 3 for k in range(9)]


def _path_tables():
    """(cell, digit) of element j of row i of matrix m, as two (72, 9, 9)
    arrays, and the cells an L firing clears as a (2, 18, 9, 81) 0/1 array."""
    cell = np.zeros((72, 9, 9), dtype=np.int64)
    digit = np.zeros((72, 9, 9), dtype=np.int64)
    for m in range(72):
        kind, idx = divmod(m, 9)
        for i in range(9):
            for j in range(9):
                if kind == 0:
                    cell[m, i, j], digit[m, i, j] = 9 * i + j, idx
                elif kind == 1:
                    cell[m, i, j], digit[m, i, j] = 9 * j + i, idx
                elif kind < 5:
                    cell[m, i, j], digit[m, i, j] = _unit_cells(kind - 2, idx)[j], i
                else:
                    cell[m, i, j], digit[m, i, j] = _unit_cells(kind - 5, idx)[i], j
    locked = np.zeros((2, 18, 9, 81), dtype=bool)
    for line in range(18):
        lc = set(_unit_cells(line // 9, line % 9))
        for box in range(9):
            bc = set(_unit_cells(2, box))
            if len(lc & bc) == 3:
                locked[0, line, box, sorted(lc - bc)] = True
                locked[1, line, box, sorted(bc - lc)] = True
    return cell, digit, locked


_PATH_TABLES = None


def apply_events(marks, events, offsets=None):
    """Replay the actions of path events on pencil marks: a Hall event takes u
    out of every row of its matrix outside I, an L event takes its digit out
    of the rest of the line (pointing) or of the box (claiming); a
    contradiction event does nothing.  The events alone say what leaves, not
    the state they were found on.  marks: (81,) masks with the events of that
    one state, or (n, 81) with the CSR offsets of BatchSolver.path.  Returns
    the new marks, a tensor for a tensor and an array for an array; the
    arithmetic is NumPy's, on the host."""
    global _PATH_TABLES
    if _PATH_TABLES is None:
        _PATH_TABLES = _path_tables()
    cell, digit, locked = _PATH_TABLES
    as_tensor = isinstance(marks, torch.Tensor)
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    mk = to_np(marks)
    out = mk.astype(np.int64).reshape(-1, 81) & 0xFFFF
    ev = to_np(events).astype(np.int64).reshape(-1, 8)
    if offsets is None:
        owner = np.zeros(len(ev), dtype=np.int64)
    else:
        owner = np.repeat(np.arange(out.shape[0]), np.diff(to_np(offsets).astype(np.int64)))
    live = ev[:, 7] == 0
    ev, owner = ev[live], owner[live]
    clear = np.zeros_like(out)
    hall = ev[:, 2] < 72
    h, ho = ev[hall], owner[hall]
    bits = 1 << np.arange(9)
    sel = (((h[:, 3, None] & bits) == 0)[:, :, None] & ((h[:, 4, None] & bits) != 0)[:, None, :])
    e, i, j = np.nonzero(sel)
    np.bitwise_or.at(clear, (ho[e], cell[h[e, 2], i, j]), 1 << digit[h[e, 2], i, j])
    lk, lo = ev[~hall], owner[~hall]
    where = locked[lk[:, 2] - 72, lk[:, 4] & 31, lk[:, 4] >> 5]  # (events, 81)
    e, c = np.nonzero(where)
    np.bitwise_or.at(clear, (lo[e], c), lk[e, 3])
    out = (out & ~clear).astype(mk.dtype if mk.dtype.kind in "iu" else np.int64).reshape(mk.shape)
    return torch.as_tensor(out, device=marks.device) if as_tensor else out


def _digits_text(mask: int) -> str:
    return "{" + ",".join(str(d + 1) for d in range(9) if mask >> d & 1) + "}"


def _join(names) -> str:
    names = [str(x) for x in names]
    return names[0] if len(names) == 1 else ", ".join(names[:-1]) + " and " + names[-1]


def _cells_text(t: int, u: int, mask: int) -> str:
    """The cells `mask` of unit u of kind t, as the UI would name them."""
    ks = [k for k in range(9) if mask >> k & 1]
    if t == 0:
        return ("columns " if len(ks) > 1 else "column ") + _join(k + 1 for k in ks)
    if t == 1:
        return ("rows " if len(ks) > 1 else "row ") + _join(k + 1 for k in ks)
    return _join("r%dc%d" % (c // 9 + 1, c % 9 + 1) for c in (_unit_cells(2, u)[k] for k in ks))


def explain(events) -> List[str]:
    """One English line per event of BatchSolver.path, for example "naked
    pair {3,7} in row 4, columns 2 and 5: 3 candidates leave"."""
    lines = []
    for rnd, cls, m, I, u, removed, left, contra in (
            events.detach().cpu().numpy() if isinstance(events, torch.Tensor) else np.asarray(events)).reshape(-1, 8).tolist():
        tail = ": %d candidate%s leave%s" % (removed, "" if removed == 1 else "s", "s" if removed == 1 else "")
        if m >= 72:
            d, line, box = I.bit_length(), u & 31, u >> 5
            lname = "%s %d" % (_UNIT_KINDS[line // 9], line % 9 + 1)
            if m == 72:
                lines.append("pointing: %d in box %d lies in %s only%s %s" % (d, box + 1, lname, tail, lname))
            else:
                lines.append("claiming: %d in %s lies in box %d only%s box %d" % (d, lname, box + 1, tail, box + 1))
            continue
        kind, idx = divmod(m, 9)
        size = bin(I).count("1")
        if kind < 2:
            lines_, cross = ("rows", "columns") if kind == 0 else ("columns", "rows")
            what = "%s on %d in %s %s, %s %s" % (PATH_CLASS_NAMES[min(cls, 8)] if cls >= 6 else "fish", idx + 1, lines_,
                                                 _join(k + 1 for k in range(9) if I >> k & 1), cross,
                                                 _join(k + 1 for k in range(9) if u >> k & 1) if u else "none")
        else:
            t = (kind - 2) % 3
            unit = "%s %d" % (_UNIT_KINDS[t], idx + 1)
            hidden = kind < 5
            digits, cells = (I, u) if hidden else (u, I)
            where = _cells_text(t, idx, cells) if cells else "no cell"
            if size == 1 and not contra:
                what = "%s single %s in %s, %s" % ("hidden" if hidden else "naked", _digits_text(digits)[1:-1], unit, where)
            else:
                what = "%s %s %s in %s, %s" % ("hidden" if hidden else "naked", PATH_CLASS_NAMES[3 + min(size, 4) - 2] if size > 1
                                               else "single", _digits_text(digits), unit, where)
        if contra:
            if size == 1 and kind >= 5:
                lines.append("contradiction: %s, %s has no candidate" % (unit, where))
            elif size == 1:
                lines.append("contradiction: %s has no place for %s" % (unit, _digits_text(I)[1:-1]))
            else:
                lines.append("contradiction: %s -- %d rows share %d" % (what, size, bin(u).count("1")))
        else:
            lines.append(what + tail)
    return lines


def make_unique(boards, device=None):
    """Boards with several completions turned into proper puzzles by adding
    givens: (puzzles (n, 81) uint8, added (n,) int32), device tensors.  Library
    extension, no reference counterpart.

    Each round takes marks = BatchSolver.candidates(board), the digits some
    completion puts into each cell.  A board with a cell of two or more
    candidates gets the cell with the MOST candidates (ties: the lowest
    index) set to its LOWEST candidate; the loop ends when a round changes
    nothing.  Every choice is a true candidate, so a board never loses its
    last completion, and it ends with exactly one.  Boards with one
    completion, with none, or with a byte > 9 come back unchanged (added 0).
    The givens are kept; added[i] is the number of new ones."""
    solver = get_solver(device)
    p = solver._dev(as_boards(boards, max_value=255)).clone()
    n = p.shape[0]
    added = torch.zeros(n, dtype=torch.int32, device=p.device)
    live = torch.arange(n, dtype=torch.int64, device=p.device)
    bit = torch.arange(9, dtype=torch.int32, device=p.device)
    rank = 80 - torch.arange(81, dtype=torch.int32, device=p.device)  # ties: the lowest index first
    while live.numel():
        marks = solver.candidates(p[live]).to(torch.int32)
        width = ((marks.unsqueeze(2) >> bit) & 1).sum(2, dtype=torch.int32)  # candidates per cell
        cell = (width * 128 + rank).argmax(1, keepdim=True)
        still = width.gather(1, cell).squeeze(1) >= 2
        live, cell = live[still], cell[still]
        if not live.numel():
            break
        m = marks[still].gather(1, cell)
        low = m & -m
        digit = (((low - 1).unsqueeze(2) >> bit) & 1).sum(2) + 1  # the lowest candidate: 1 + its bit number
        p[live, cell.squeeze(1)] = digit.squeeze(1).to(torch.uint8)
        added[live] += 1
    return p, added


# ------------------------------------------------------------- clue exchange
# Q boards per BatchSolver.unique_candidates call inside exchange(): the bit
# expansion of a chunk's answer holds 81 x 9 int32 per board beside the boards
# and the int16 answer, about 200 MB for 2^16 boards
EXCHANGE_CHUNK = 1 << 16


def exchange(puzzles, device=None):
    """The {-1, +1} neighbours of proper puzzles: every proper puzzle that
    comes from one of `puzzles` by erasing one clue and adding one.  Library
    extension, no reference counterpart; the GPU counterpart of
    scripts/hard17/hard17_search.c, with no cap.

    For every puzzle i with exactly one completion and every given cell a, let
    Q be the puzzle without a.  Every empty cell b of Q (a included) and digit
    v that exactly one completion of Q puts there
    (BatchSolver.unique_candidates) gives the neighbour Q + (b, v) -- except
    (a, the erased digit), which is puzzle i itself.  Every neighbour has
    exactly one completion and as many clues as its parent.

    Returns (neighbours (m, 81) uint8, parent (m,) int64, removed (m,) int32,
    added_cell (m,) int32, added_digit (m,) int32), device tensors, sorted by
    (parent, removed cell a, added cell b, added digit v).  Puzzles with no
    completion or several, or with a byte > 9, contribute nothing.  The Q
    boards of the whole batch are built with tensor operations and answered
    EXCHANGE_CHUNK at a time; there is no loop over boards."""
    solver = get_solver(device)
    p = solver._dev(as_boards(puzzles, max_value=255))
    dev = p.device
    proper = solver.count_solutions(p, limit=2) == 1
    parent, removed = torch.nonzero(proper.unsqueeze(1) & (p != 0), as_tuple=True)  # sorted by (parent, a)
    q = p[parent]
    rows = torch.arange(q.shape[0], dtype=torch.int64, device=dev)
    erased = q[rows, removed].to(torch.int64)
    q[rows, removed] = 0
    bit = torch.arange(9, dtype=torch.int32, device=dev)
    found = []
    for lo in range(0, q.shape[0], EXCHANGE_CHUNK):
        qc = q[lo:lo + EXCHANGE_CHUNK]
        once = solver.unique_candidates(qc).to(torch.int32)
        hit = (((once.unsqueeze(2) >> bit) & 1) != 0) & (qc == 0).unsqueeze(2)
        k = rows[:qc.shape[0]]
        hit[k, removed[lo:lo + EXCHANGE_CHUNK], erased[lo:lo + EXCHANGE_CHUNK] - 1] = False  # the parent itself
        r, b, v = torch.nonzero(hit, as_tuple=True)  # sorted by (row, b, v)
        found.append((r + lo, b, v))
    if found:
        r, b, v = (torch.cat(x) for x in zip(*found))
    else:
        r = b = v = torch.zeros(0, dtype=torch.int64, device=dev)
    neighbours = q[r]
    neighbours[torch.arange(r.shape[0], dtype=torch.int64, device=dev), b] = (v + 1).to(torch.uint8)
    return neighbours, parent[r], removed[r].to(torch.int32), b.to(torch.int32), (v + 1).to(torch.int32)


def _first_unique(boards, known: int):
    """Indices (ascending) of the rows of `boards` from row `known` on that
    equal no earlier row: the new classes in order of first appearance."""
    n = boards.shape[0]
    if not n:
        return torch.zeros(0, dtype=torch.int64, device=boards.device)
    uniq, ids = torch.unique(boards, dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), n, dtype=torch.int64, device=boards.device)
    first.scatter_reduce_(0, ids, torch.arange(n, dtype=torch.int64, device=boards.device), reduce="amin")
    first = torch.sort(first).values
    return first[first >= known]


def exchange_search(seeds, target: int, max_rounds: Optional[int] = None, device=None):
    """Breadth-first search over isomorphism classes by clue exchange: the
    canonical boards (BatchSolver.canonical) of the classes found, as a
    (k, 81) uint8 device tensor -- the seeds' classes first, in the seeds'
    order, then every new class in the order in which it first appears.
    Library extension; what scripts/make_hard17.py does on the CPU.

    Round 0's frontier is the seeds' classes (their canonical boards).  Each
    round takes exchange(frontier), the canonical forms of its neighbours, and
    keeps the classes not seen before, in order of first appearance; they are
    the next frontier.  The search stops when `target` classes are known (the
    round that reaches it is cut there, so k <= target unless the seeds alone
    are more), when a frontier is empty, or after max_rounds rounds (None: no
    limit).  Deterministic: the same seeds give the same tensor."""
    solver = get_solver(device)
    canon = solver.canonical(solver._dev(as_boards(seeds, max_value=255)))
    classes = canon[_first_unique(canon, 0)]
    frontier, rounds = classes, 0
    while classes.shape[0] < target and frontier.shape[0] and (max_rounds is None or rounds < max_rounds):
        neighbours = exchange(frontier, device=device)[0]
        if not neighbours.shape[0]:
            break
        known = classes.shape[0]
        both = torch.cat([classes, solver.canonical(neighbours)])
        frontier = both[_first_unique(both, known)][:max(0, int(target) - known)]
        classes = torch.cat([classes, frontier])
        rounds += 1
    return classes


# ------------------------------------------------------------ symmetry classes
_PERM3 =((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
CANON_SYMMETRIES = 2 * 1296 * 1296


def line_perms() -> np.ndarray:
    """The 1296 line permutations as a (1296, 9) array: number
    p = ((bp*6 + a)*6 + b)*6 + d is perm[k] = 3*PERM3[bp][k//3] +
    PERM3[(a, b, d)[k//3]][k%3] (include/sudoku_hip.h, sdk_canonical_batch)."""
    out = np.empty((1296, 9), dtype=np.int64)
    for p in range(1296):
        bp, inner = p // 216, ((p // 36) % 6, (p // 6) % 6, p % 6)
        out[p] = [3 * _PERM3[bp][k // 3] + _PERM3[inner[k // 3]][k % 3] for k in range(9)]
    return out


def apply_symmetry(boards, sym):
    """The image of every board under its symmetry number, straight from the
    definition (pure numpy, independent of the kernel): sym = (t*1296 + ri)*1296
    + ci; image cell (i, j) = g[R[i]][C[j]], or g[C[j]][R[i]] when t == 1; then
    the non-zero digits relabelled 1, 2, ... in order of first appearance.
    boards: (n, 81) with bytes 0..9; sym: n numbers in [0, 3359232) (or one
    for all).  Returns (images (n, 81) uint8, digit_maps (n, 10) uint8) with
    digit_maps[i, x] = the label digit x of board i got (0: x is 0 or absent)
    -- tensors on the boards' device if `boards` is a tensor, else arrays."""
    as_tensor = isinstance(boards, torch.Tensor)
    b = (boards.cpu().numpy() if as_tensor else np.asarray(boards)).astype(np.uint8).reshape(-1, 81)
    s = sym.cpu().numpy() if isinstance(sym, torch.Tensor) else np.asarray(sym)
    s = np.broadcast_to(s.astype(np.int64).reshape(-1), (len(b),))
    if b.size and b.max() > 9:
        raise ValueError("board cells must be 0..9")
    if len(s) and (s.min() < 0 or s.max() >= CANON_SYMMETRIES):
        raise ValueError(f"sym must be in [0, {CANON_SYMMETRIES})")
    perms = line_perms()
    t, R, C = s // (1296 * 1296), perms[(s // 1296) % 1296], perms[s % 1296]
    r, c = R[:, :, None], C[:, None, :]
    src = np.where(t[:, None, None] == 1, c * 9 + r, r * 9 + c).reshape(-1, 81)
    img = np.take_along_axis(b, src, axis=1)
    # the first position of every digit (81: absent) ranks the digits
    first = np.stack([np.where((img == x).any(1), (img == x).argmax(1), 81) for x in range(1, 10)], axis=1)
    label = 1 + (first[:, None, :] < first[:, :, None]).sum(2)
    maps = np.zeros((len(b), 10), dtype=np.uint8)
    maps[:, 1:] = np.where(first < 81, label, 0)
    out = np.take_along_axis(maps, img.astype(np.int64), axis=1)
    if as_tensor:
        return torch.from_numpy(out).to(boards.device), torch.from_numpy(maps).to(boards.device)
    return out, maps


def class_ids(boards, device=None):
    """The isomorphism class of every board: (canon, ids, first_index) --
    canon (n, 81) uint8, the canonical forms (BatchSolver.canonical); ids
    (n,) int64, a dense class number per board (classes numbered in the
    lexicographic order of their canonical forms); first_index (classes,)
    int64, the index of each class's first member.  Device tensors."""
    canon = get_solver(device).canonical(boards)
    n = canon.shape[0]
    uniq, ids = torch.unique(canon, dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), n, dtype=torch.int64, device=canon.device)
    first.scatter_reduce_(0, ids, torch.arange(n, dtype=torch.int64, device=canon.device), reduce="amin")
    return canon, ids, first


# ------------------------------------------------------- completion lists
_M64 = (1 << 64) - 1


def _mix(x: int) -> int:
    """sdk_sample_batch's mix (include/sudoku_hip.h), mod 2^64."""
    x &= _M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _M64
    return x ^ (x >> 31)


def uniform_completions(boards, seed: int = 0, per_board: int = 1, first_key: int = 0, limit: int = 1 << 16,
                        device=None):
    """Uniform random completions: (grids (n * per_board, 81) uint8, status
    (n * per_board,) int32), item q = i * per_board + j being a completion of
    board i.  UNIFORM over the board's completions, where BatchSolver.sample
    is explicitly not: the board's completions are listed
    (BatchSolver.completions, sorted) and item q takes row
    ((r >> 32) * count_i) >> 32 of board i's list, r = mix(mix(seed) +
    first_key + q) mod 2^64 with sdk_sample_batch's mix -- a function of the
    board, seed and key alone.  Only for boards whose completions fit the
    list: a board with `limit` completions or more (SDK_ENUM_LIMITED) or one
    left SDK_ENUM_PARTIAL raises SudokuHipError.  A board without a completion
    gives status 0 and its own row, like sample; every other item status 1."""
    solver = get_solver(device)
    p = solver._dev(as_boards(boards, max_value=255))
    n, per_board, limit = p.shape[0], int(per_board), int(limit)
    if per_board < 1 or limit < 1:
        raise ValueError("per_board and limit must be >= 1")
    grids, offsets, count, status, info = solver.completions(p, limit=limit, return_status=True)
    if info["listed"] < info["total"] or bool((status != 1).any().item()):
        bad = int((status != 1).sum().item())
        raise SudokuHipError(f"uniform_completions: {bad} of {n} boards without a complete list below "
                                  f"limit={limit} (statuses {sorted(set(status.tolist()))})")
    cnt, off = count.tolist(), offsets.tolist()
    base = _mix(seed)
    rows, st = [], []
    for q in range(n * per_board):
        i = q // per_board
        r = _mix(base + int(first_key) + q)
        st.append(1 if cnt[i] else 0)
        rows.append(off[i] + (((r >> 32) * cnt[i]) >> 32) if cnt[i] else -1)
    rows = torch.tensor(rows, dtype=torch.int64, device=p.device)
    st = torch.tensor(st, dtype=torch.int32, device=p.device)
    out = p.repeat_interleave(per_board, dim=0)
    has = rows >= 0
    out[has] = grids[rows[has]]
    return out, st


def completion_classes(board, limit: int = 0, capacity=None, device=None):
    """How many essentially different grids a pattern of givens has:
    (representatives (k, 81) uint8, multiplicities (k,) int64) -- the
    canonical forms (BatchSolver.canonical) of the board's completions, each
    once, in lexicographic order, and how many completions have each.
    limit / capacity as in BatchSolver.completions, whose errors apply."""
    solver = get_solver(device)
    p = solver._dev(as_boards(board, max_value=255))
    if p.shape[0] != 1:
        raise ValueError("completion_classes takes one board")
    grids, _ = solver.completions(p, limit=limit, capacity=capacity, sort=False)
    if grids.shape[0] == 0:
        return grids, torch.zeros(0, dtype=torch.int64, device=grids.device)
    return torch.unique(solver.canonical(grids), dim=0, return_counts=True)


# ------------------------------------------------------------ unavoidable sets
def _set_cells(sets: torch.Tensor) -> torch.Tensor:
    """BatchSolver.unavoidable's sets, packed or not, as a bool (R, 81) tensor."""
    if sets.dim() == 2 and sets.shape[1] == 3:
        cells = torch.arange(81, device=sets.device)
        return ((sets.to(torch.int64)[:, cells >> 5] >> (cells & 31)) & 1).bool()
    if sets.dim() != 2 or sets.shape[1] != 81:
        raise ValueError("sets must be (R, 81) or packed (R, 3)")
    return sets.bool()


def clue_lower_bound(grids, max_size: int = 12, device=None) -> torch.Tensor:
    """A lower bound on the clues of every puzzle whose one solution is the
    grid, as an int64 (n,) tensor: the size of a family of pairwise disjoint
    minimal unavoidable sets of at most max_size cells
    (BatchSolver.unavoidable) -- a puzzle needs a given in
    each.  The family is GREEDY: the sets are taken in the listed order (by
    size, then cell list), each one that meets none taken before.  Any
    disjoint family is a valid bound; this is not the largest one (the clique
    number of the disjointness graph), only a cheap one."""
    solver = get_solver(device)
    return _greedy_bound(*solver.unavoidable(grids, max_size=max_size, minimal=True, packed=True))


def _greedy_bound(sets: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """clue_lower_bound on packed sets already listed."""
    n = offsets.shape[0] - 1
    words = sets.to(torch.int64) & 0xFFFFFFFF
    counts = offsets[1:] - offsets[:-1]
    used = torch.zeros((n, 3), dtype=torch.int64, device=sets.device)
    bound = torch.zeros(n, dtype=torch.int64, device=sets.device)
    for r in range(int(counts.max().item()) if n else 0):
        live = torch.nonzero(counts > r)[:, 0]
        s = words[offsets[live] + r]
        free = ((s & used[live]) == 0).all(dim=1)
        live, s = live[free], s[free]
        used[live] |= s
        bound[live] += 1
    return bound


def hits_unavoidable(puzzles, sets, offsets, device=None) -> torch.Tensor:
    """Per puzzle, whether its givens meet every listed unavoidable set of
    its grid, as a bool (n,) tensor: (sets, offsets) as BatchSolver.unavoidable
    returns them for the puzzles' solution grids, packed or not.  A puzzle
    that misses one has a second completion -- the cheap necessary test before
    any solver; with no set listed the answer is True."""
    solver = get_solver(device)
    p = solver._dev(as_boards(puzzles, max_value=255))
    n = p.shape[0]
    offsets = offsets.to(p.device)
    if offsets.shape != (n + 1,):
        raise ValueError("offsets must hold one entry per puzzle and one more")
    cells = _set_cells(sets.to(p.device))
    owner = torch.repeat_interleave(torch.arange(n, device=p.device), offsets[1:] - offsets[:-1])
    missed = ~(cells & (p != 0)[owner]).any(dim=1)
    return torch.zeros(n, dtype=torch.int64, device=p.device).index_add_(0, owner, missed.to(torch.int64)) == 0


# ---------------------------------------------------------------- hitting sets
def _take_families(sets: torch.Tensor, offsets: torch.Tensor, idx: torch.Tensor):
    """The CSR lists of the families `idx` (with repeats, in that order)."""
    lens = (offsets[1:] - offsets[:-1])[idx]
    out = torch.zeros(idx.shape[0] + 1, dtype=torch.int64, device=offsets.device)
    out[1:] = torch.cumsum(lens, dim=0)
    rows = torch.repeat_interleave(offsets[idx] - out[:-1], lens) + torch.arange(int(out[-1].item()), device=offsets.device)
    return sets[rows], out


def min_hitting_clues(grids, max_size: int = 12, allowed=None, sets=None, device=None) -> torch.Tensor:
    """SLOW on whole grids at the default max_size: every k below the answer
    is searched to the end, which on all 81 cells with sets of 12 cells takes
    one MI355X 51 s for a hard17 grid; max_size
    8 or `allowed` cells make it milliseconds.

    A PROVEN lower bound on the clues of every puzzle whose one solution is
    the grid, as an int64 (n,) tensor: the least k for which some k cells meet
    every minimal unavoidable set of at most max_size cells
    (BatchSolver.unavoidable, BatchSolver.hitting_sets with limit=1; DESIGN.md
    §25) -- the hitting number of that family.  The search runs upward from
    clue_lower_bound's greedy packing, which it is never below: k clues cannot
    meet more than k disjoint sets.  allowed (masks as in hitting_sets): the
    bound for the puzzles whose clues lie inside those cells, never below the
    unrestricted one and far cheaper to find.  sets: (sets, offsets) as
    BatchSolver.unavoidable(grids, max_size, packed=True) returns them, when
    the caller has them already."""
    solver = get_solver(device)
    sets, offsets = sets if sets is not None else solver.unavoidable(grids, max_size=max_size, minimal=True, packed=True)
    if allowed is not None:
        allowed = solver._cell_masks(allowed, offsets.shape[0] - 1, "allowed", 0)
    n = offsets.shape[0] - 1
    k_of = _greedy_bound(sets, offsets)
    done = torch.zeros(n, dtype=torch.bool, device=sets.device)
    k = int(k_of.min().item()) if n else 0
    while n and not bool(done.all().item()):
        if k > _lib_hit_max():
            raise SudokuHipError(f"min_hitting_clues: no hitting set of {_lib_hit_max()} cells")
        idx = torch.nonzero(~done & (k_of <= k))[:, 0]
        if idx.shape[0]:
            s, o = _take_families(sets, offsets, idx)
            count = solver.hitting_sets(s, o, k, allowed=None if allowed is None else allowed[idx], limit=1, capacity=0,
                                        return_count=True)[2]
            done[idx[count > 0]] = True
            k_of[idx[count == 0]] = k + 1
        k += 1
    return k_of


def _lib_hit_max() -> int:
    from ._lib import SDK_HIT_MAX_CLUES
    return SDK_HIT_MAX_CLUES


def smallest_sub_puzzles(puzzles, max_size: int = 12, device=None):
    """The smallest proper puzzles inside proper puzzles: per puzzle the
    least k at which some k of its givens still have one completion, and every
    such sub-puzzle, as (k int64 (n,), sub-puzzles (R, 81) uint8, offsets
    (n + 1,) int64).  The search runs upward from min_hitting_clues of the
    solution grid inside the givens (below it no k givens meet the grid's
    unavoidable sets) with BatchSolver.sub_puzzles(grid, k, allowed=givens).  A puzzle without
    exactly one completion raises."""
    solver = get_solver(device)
    p = solver._dev(as_boards(puzzles))
    n = p.shape[0]
    counts, grids = solver.count_solutions(p, limit=2, return_first=True)
    if n and bool((counts != 1).any().item()):
        raise SudokuHipError(f"smallest_sub_puzzles: {int((counts != 1).sum().item())} of {n} puzzles are not proper")
    sets = solver.unavoidable(grids, max_size=max_size, packed=True)
    given = (p != 0).to(torch.uint8)
    k_of = min_hitting_clues(grids, max_size=max_size, allowed=given, sets=sets, device=device)
    clues = given.sum(dim=1).tolist()
    done = torch.zeros(n, dtype=torch.bool, device=p.device)
    found = [None] * n
    k = int(k_of.min().item()) if n else 0
    while n and not bool(done.all().item()):
        idx = torch.nonzero(~done & (k_of <= k))[:, 0]
        if idx.shape[0]:
            if k > _lib_hit_max():
                raise SudokuHipError(f"smallest_sub_puzzles: no sub-puzzle of {_lib_hit_max()} clues or fewer")
            sub, off = solver.sub_puzzles(grids[idx], k, allowed=given[idx], sets=_take_families(sets[0], sets[1], idx))
            off = off.tolist()
            for j, i in enumerate(idx.tolist()):
                if off[j + 1] > off[j] or k >= clues[i]:
                    found[i] = sub[off[j]:off[j + 1]]
                    done[i] = True
                else:
                    k_of[i] = k + 1
        k += 1
    per = torch.tensor([f.shape[0] for f in found], dtype=torch.int64, device=p.device)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=p.device)
    offsets[1:] = torch.cumsum(per, dim=0)
    subs = torch.cat(found) if n else torch.zeros((0, 81), dtype=torch.uint8, device=p.device)
    return k_of, subs, offsets


def neighbourhood(puzzles, d: int = 1, max_size: int = 12, device=None):
    """The {-d, +d} neighbours of proper puzzles, d = 1..3: every proper
    puzzle other than puzzle i itself that comes from it by erasing d clues
    and adding d (a clue erased may come back, so the nearer neighbours are
    among them), as (neighbours (m, 81) uint8, parent (m,) int64), each once a
    parent, sorted by parent and then by ascending clue cells.  Every
    neighbour has its parent's SOLUTION and number of clues: d = 1 gives the
    boards of exchange() that complete to the parent's grid (exchange also
    lists neighbours that complete to another grid; the unavoidable sets of
    the parent's grid say nothing about those).  For every d-subset of the givens the rest is
    `required` of one BatchSolver.sub_puzzles family of the solution grid at
    k = the puzzle's clues.  Puzzles with no completion or several, or with a
    byte > 9, contribute nothing.  One unavoidable call serves the batch; the
    families are then built puzzle by puzzle, each d-subset with a copy of its
    grid's sets (the CSR form has no way to share one list between families)."""
    import itertools
    if d not in (1, 2, 3):
        raise ValueError("d must be 1, 2 or 3")
    solver = get_solver(device)
    p = solver._dev(as_boards(puzzles, max_value=255))
    dev = p.device
    counts, grids = solver.count_solutions(p, limit=2, return_first=True)
    clues = (p != 0).sum(dim=1)
    ok = (counts == 1) & (clues >= d) & (clues <= _lib_hit_max())
    out, parents = [], []
    live = torch.nonzero(ok)[:, 0]
    usets, uoff = solver.unavoidable(grids[live], max_size=max_size, packed=True) if live.shape[0] else (None, None)
    for at, i in enumerate(live.tolist()):
        cells = torch.nonzero(p[i])[:, 0]
        combos = torch.tensor(list(itertools.combinations(range(cells.shape[0]), d)), dtype=torch.int64, device=dev)
        req = (p[i] != 0).to(torch.uint8).repeat(combos.shape[0], 1)
        req[torch.arange(combos.shape[0], device=dev).unsqueeze(1), cells[combos]] = 0
        fam = _take_families(usets, uoff, torch.full((combos.shape[0],), at, dtype=torch.int64, device=dev))
        sub, _ = solver.sub_puzzles(grids[i:i + 1].expand(combos.shape[0], -1), int(clues[i]), required=req, sets=fam)
        sub = torch.unique(sub, dim=0) if sub.shape[0] else sub
        sub = sub[(sub != p[i]).any(dim=1)]
        # torch.unique orders boards by digits; the public order is by clue cells: the board with a clue in the first
        # cell two differ in comes first (three keys of 27 cells, cell 0 the highest bit, each descending)
        weight = 1 << (26 - torch.arange(81, device=dev) % 27)
        for j in (2, 1, 0):
            key = ((sub[:, 27 * j:27 * j + 27] != 0) * weight[27 * j:27 * j + 27]).sum(dim=1)
            sub = sub[torch.sort(key, descending=True, stable=True)[1]]
        out.append(sub)
        parents.append(torch.full((sub.shape[0],), i, dtype=torch.int64, device=dev))
    if not out:
        return torch.zeros((0, 81), dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    return torch.cat(out), torch.cat(parents)


# ------------------------------------------------------------ hard 17-clue set
def _perms(rng: np.random.Generator, shape, k: int) -> np.ndarray:
    """Uniform random permutations of range(k), vectorised over `shape`."""
    return np.argsort(rng.random(tuple(shape) + (k,)), axis=-1)


def _symmetry_images(base: np.ndarray, n: int, seed: int) -> np.ndarray:
    """n random validity-preserving images of the (k, 81) boards `base`:
    digit relabeling, row / column permutations inside bands / stacks,
    band / stack permutations, transposition.  Clue count, number of
    completions and logical difficulty are invariants; the walk's cell
    order sees a different board each time."""
    rng = np.random.default_rng(seed)
    base = base.reshape(-1, 9, 9)
    which = rng.integers(len(base), size=n)
    relabel = np.zeros((n, 10), dtype=np.uint8)
    relabel[:, 1:] = _perms(rng, (n,), 9) + 1
    rows = (_perms(rng, (n,), 3)[:, :, None] * 3 + _perms(rng, (n, 3), 3)).reshape(n, 9)
    cols = (_perms(rng, (n,), 3)[:, :, None] * 3 + _perms(rng, (n, 3), 3)).reshape(n, 9)
    trans = rng.integers(2, size=n).astype(bool)
    # one flat source cell per output cell, then 1-D takes in blocks (the same
    # draws and bytes as transposing and gathering rows, columns and digits
    # in turn, in a third of the time): out(r, c) = base(rows[r], cols[c]), or
    # base(cols[c], rows[r]) when transposed
    out = np.empty((n, 81), dtype=np.uint8)
    flat = base.reshape(len(base), 81)
    for lo in range(0, n, 1 << 16):
        sl = slice(lo, min(n, lo + (1 << 16)))
        m = sl.stop - lo
        r, c = rows[sl, :, None].astype(np.int32), cols[sl, None, :].astype(np.int32)
        src = np.where(trans[sl, None, None], c * 9 + r, r * 9 + c).reshape(m, 81)
        cell = np.take(flat, which[sl, None].astype(np.int64) * 81 + src)
        out[sl] = np.take(relabel[sl].ravel(), np.arange(m, dtype=np.int64)[:, None] * 10 + cell)
    return out


_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def hard17_classes() -> List[str]:
    """The hard 17-clue corpus: one board per isomorphism class (minlex
    form), each certified 17 clues + one completion (data/hard17_classes.txt,
    made by scripts/make_hard17.py from SEEDS_17 by clue exchanges)."""
    with open(os.path.join(_DATA, "hard17_classes.txt")) as f:
        return [ln.split()[0] for ln in f if ln.strip() and not ln.startswith("#")]


def hard17_batch(n: int, seed: int = 0, seeds=None, device=None) -> torch.Tensor:
    """n 17-clue unique-solution boards (symmetry images of `seeds`, default
    the hard17_classes() corpus), as a (n, 81) uint8 tensor on `device`
    (host if device is None)."""
    seeds = hard17_classes() if seeds is None else seeds
    base = np.array([[int(c) for c in s] for s in seeds], dtype=np.uint8)
    t = torch.from_numpy(np.ascontiguousarray(_symmetry_images(base, n, seed)))
    return t.to(device) if device is not None else t


_HARD_SEARCH = os.path.join(_DATA, "hard_search_seeds.txt")


def hard_search_seeds() -> List[str]:
    """The search-heavy seed boards (data/hard_search_seeds.txt, made by
    scripts/make_hard_search.py): minimal unique puzzles from gen.py-style
    grids that naked + hidden singles cannot finish (>= 2 guesses)."""
    with open(_HARD_SEARCH) as f:
        return [ln.split()[0] for ln in f if ln.strip() and not ln.startswith("#")]


def hard_search_batch(n: int, seed: int = 0, device=None) -> torch.Tensor:
    """n search-heavy unique-solution boards (symmetry images of
    hard_search_seeds()), as a (n, 81) uint8 tensor."""
    base = np.array([[int(c) for c in s] for s in hard_search_seeds()], dtype=np.uint8)
    t = torch.from_numpy(np.ascontiguousarray(_symmetry_images(base, n, seed)))
    return t.to(device) if device is not None else t


if __name__ == "__main__":  # gen.py:55-66
    empty_boxes = int(sys.argv[1])
    new_puzzle = generate_sudoku(empty_boxes)
    print(new_puzzle)
    print(
        "curl http://localhost:8001/solve -X POST -H 'Content-Type: application/json' -d '{\"sudoku\": %s}'"
        % (new_puzzle.grid)
    )
