"""The boards and recorded answers the unique-candidates tests share
(test_uniq_host.py on the CPU, test_gpu_uniq.py on the GPU), and the oracle's
restatement of the definition:

    marks[c] bit d-1  <=>  at least one valid completion of the board puts d into c
    once[c]  bit d-1  <=>  exactly one does

tests/golden/make_uniq_cases.py records oracle_once() of its boards in
tests/golden/uniq_cases.json; load_fixture() reads them back.  Loaded once per
process and shared, never modified.

The boards are those of cand_cases.json (same names, same order).  Cost
condition: at the default sweep, the host build of plane_uniq.h takes no more
than PASS_BUDGET passes for any of them -- a lane sustains about 10^5 passes a
second while its wave waits for it (the 513-board case holds the
22 012-pass board twice and two calls take 0.22 s), and a board gets no more
than about a second of that.  make_uniq_cases.py prints the passes per board
and would replace a board over the budget by the next of its set; none is.
"""
import functools
import json
import os

import numpy as np

from cand_cases import ALL, FAULT, INVALID, PEERS, board_from_text, board_text, count_of, marks_from_text, marks_text  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "uniq_cases.json")
PASS_BUDGET = 100_000  # host-model passes of one fixture board at the default sweep


def oracle_once(board):
    """(once[81], marks[81], count) of one board from the oracle's counter
    alone: per empty cell and digit that repeats no digit of the cell's units,
    k = O.count_solutions(board with the cell set, 2); k >= 1 sets the marks
    bit, k == 1 the once bit.  A given's own bits come from
    O.count_solutions(board, 2) in the same way.  A byte > 9: zeros and
    INVALID; clashing givens: zeros and 0."""
    from oracle import oracle as O
    import count_cases as C
    board = np.asarray(board, dtype=np.uint8).reshape(81)
    if (board > 9).any():
        return [0] * 81, [0] * 81, INVALID
    if C.givens_clash(board):
        return [0] * 81, [0] * 81, 0
    whole = O.count_solutions(board, 2)
    if whole == 0:
        return [0] * 81, [0] * 81, 0
    once, marks = [0] * 81, [0] * 81
    for c in range(81):
        if board[c]:
            marks[c] = 1 << (int(board[c]) - 1)
            once[c] = marks[c] if whole == 1 else 0
            continue
        seen = {int(board[p]) for p in PEERS[c]}
        for d in range(1, 10):
            if d in seen:
                continue
            trial = board.copy()
            trial[c] = d
            k = O.count_solutions(trial, 2)
            if k >= 1:
                marks[c] |= 1 << (d - 1)
            if k == 1:
                once[c] |= 1 << (d - 1)
    return once, marks, count_of(marks)


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/uniq_cases.json as (names, boards (n, 81) uint8, once
    (n, 81) uint16, marks (n, 81) uint16, count (n,) int32), read-only."""
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    names = [c["name"] for c in cases]
    boards = np.array([board_from_text(c["board"]) for c in cases], dtype=np.uint8)
    once = np.array([marks_from_text(c["once"]) for c in cases], dtype=np.uint16)
    marks = np.array([marks_from_text(c["marks"]) for c in cases], dtype=np.uint16)
    count = np.array([c["count"] for c in cases], dtype=np.int32)
    for v in (boards, once, marks, count):
        v.setflags(write=False)
    return names, boards, once, marks, count


def composed(solver, boards):
    """The composition that unique_candidates replaces, from calls that were
    there before it: marks = solver.candidates(boards), every marks bit of an
    empty cell expanded into the board with that clue added, and one
    solver.count_solutions(limit=2) over all of them.  Returns (once (n, 81)
    int16, marks, count (n,) int32, counts): once has the bit where the
    expanded board's count is 1, and a given's own bit where the board's own
    count is 1; counts are the expanded boards' counts (each 1 or 2: a
    candidate has a completion).  Device tensors, tensor operations only.
    scripts/uniq_bench.py times this as its yardstick."""
    import torch
    p = solver._dev(torch.as_tensor(boards, dtype=torch.uint8).reshape(-1, 81))
    marks, count = solver.candidates(p, return_count=True)
    bit = torch.arange(9, dtype=torch.int32, device=p.device)
    has = ((marks.to(torch.int32).unsqueeze(2) >> bit) & 1) != 0
    i, c, v = torch.nonzero(has & (p == 0).unsqueeze(2), as_tuple=True)
    trial = p[i]
    trial[torch.arange(i.shape[0], device=p.device), c] = (v + 1).to(torch.uint8)
    counts = solver.count_solutions(trial, limit=2)
    once = torch.zeros(p.shape, dtype=torch.int32, device=p.device)
    one = counts == 1
    once.index_put_((i[one], c[one]), (1 << v[one]).to(torch.int32), accumulate=True)
    own = (p != 0) & (count == 1).unsqueeze(1)
    once = torch.where(own, marks.to(torch.int32), once).to(torch.int16)
    return once, marks, count, counts
