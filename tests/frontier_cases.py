"""A plain reference of the frontier split's contract (include/sudoku_hip.h,
sdk_expand_frontier), for test_frontier_contract.py on the CPU and
test_gpu_frontier.py on the GPU: pure numpy plus the oracle.

Nothing here restates the packed kernel's propagation.  check_level tests
what the header promises for ANY sound propagation: a node's children keep
its cells, are the candidates of the walk's next cell of one common grid P
(the node with whatever the propagation filled in), digits ascending, none
missing and none extra -- and, where the walk's answer of the node is known,
the child that carries it is there and everything in front of it fails.

Answers are the walk's (status, solution) pairs.  Where they come from:
  * the committed fixture tests/golden/random_generated.npz (fixture());
  * O.solve_unique_batch for boards with one completion;
  * "the walk fails" on a board with clean givens: the oracle's counter says
    it has no completion.  O.count_solutions(board, 1) == 0 and
    O.solve_unique_batch's count == 0 are the same statement; the second (the
    counter that fills singles before each branch, pinned to the plain one by
    test_oracle.py and to the first by test_frontier_contract.py) is the one
    used: a few sparse dead children keep the first busy for ten seconds each;
  * the literal walk O.solve_batch(., "node_literal" / "gen") for boards
    whose givens clash -- the counter is about valid grids only, and only
    such boards can reach node.py's short-circuit (node.py:44-45).
"""
import functools
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# units: rows, columns, boxes; peers of a cell: its row, column and box
UNITS = np.array([[r * 9 + k for k in range(9)] for r in range(9)]
                 + [[k * 9 + c for k in range(9)] for c in range(9)]
                 + [[(br + k // 3) * 9 + bc + k % 3 for k in range(9)] for br in (0, 3, 6) for bc in (0, 3, 6)])
PEERS = np.zeros((81, 81), dtype=bool)
for _u in UNITS:
    PEERS[np.ix_(_u, _u)] = True
PEERS[np.arange(81), np.arange(81)] = False


def givens_clash(board) -> bool:
    """Do the digits on the board repeat in a row, column or box?"""
    u = np.asarray(board, dtype=np.int64)[UNITS]
    seen = np.zeros((27, 10), dtype=np.int64)
    np.add.at(seen, (np.arange(27)[:, None], u), 1)
    return bool((seen[:, 1:] > 1).any())


def next_cell(g, order) -> int:
    """The walk's next cell of g (-1: none).  gen (gen.py:6-28, whose scan
    breaks only its inner loop): the first empty cell of the LAST row that
    has one; node (node.py:62-74): the first empty cell, row-major."""
    e = np.flatnonzero(np.asarray(g) == 0)
    if e.size == 0:
        return -1
    if order == "node":
        return int(e[0])
    return int(e[e // 9 == e[-1] // 9][0])


def absent_digits(g, cell):
    """Digits 1..9 that stand nowhere in the row, column and box of `cell`."""
    return np.setdiff1d(np.arange(1, 10), np.asarray(g)[PEERS[cell]])


def walk_fails(node, kids, order):
    """Per kid: the walk finds no completion.  Clean givens: the oracle's
    counter; clashing givens (the counter is about valid grids only): the
    literal walk itself."""
    kids = np.ascontiguousarray(kids, dtype=np.uint8).reshape(-1, 81)
    if len(kids) == 0:
        return np.zeros(0, dtype=bool)
    if givens_clash(node):
        _, st = O.solve_batch(kids, order="node_literal" if order == "node" else "gen")
        return st != 1
    return O.solve_unique_batch(kids)[1] == 0


def check_level(nodes, offsets, children, order, answers, stats=None):
    """One frontier level against the contract.  nodes (n, 81), offsets
    (n + 1,), children (total, 81); answers[i] = the walk's (status,
    solution) of node i, or None for a node the oracle has no single answer
    for (structural rules only).  Raises AssertionError naming the node.
    stats (optional dict): counts "earlier" siblings proven to fail."""
    nodes = np.asarray(nodes, dtype=np.uint8).reshape(-1, 81)
    children = np.asarray(children, dtype=np.uint8).reshape(-1, 81)
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(nodes)
    assert offsets.shape == (n + 1,), f"level: {offsets.shape[0]} offsets for {n} nodes"
    assert len(answers) == n, f"level: {len(answers)} answers for {n} nodes"
    assert offsets[0] == 0, f"level: offsets[0] = {offsets[0]}"
    counts = np.diff(offsets)
    for i in np.flatnonzero(counts < 0):
        raise AssertionError(f"node {i}: offsets decrease ({offsets[i]} -> {offsets[i + 1]})")
    for i in np.flatnonzero(counts > 9):
        raise AssertionError(f"node {i}: {counts[i]} children")
    assert offsets[n] == len(children), f"level: offsets[n] = {offsets[n]} but {len(children)} children"
    for i in range(n):
        g = nodes[i]
        C = children[offsets[i]:offsets[i + 1]]
        # ---- structure
        kept = g != 0
        for k, ch in enumerate(C):
            assert (ch[kept] == g[kept]).all(), f"node {i}: child {k} changes a filled cell of the node"
            assert ch.max() <= 9, f"node {i}: child {k} holds a byte > 9"
        if len(C) >= 2:
            diff = np.flatnonzero((C != C[0]).any(axis=0))
            assert diff.size == 1, f"node {i}: the children differ in cells {diff.tolist()}, not in exactly one"
            c = int(diff[0])
            P = C[0].copy()
            P[c] = 0
            assert g[c] == 0, f"node {i}: branch cell {c} is filled in the node"
            want_c = next_cell(P, order)
            assert c == want_c, f"node {i}: branches on cell {c}, the walk's next cell is {want_c}"
            digits = C[:, c].astype(np.int64)
            assert (digits >= 1).all(), f"node {i}: a child leaves the branch cell {c} empty"
            assert (np.diff(digits) > 0).all(), f"node {i}: child digits {digits.tolist()} at cell {c} not ascending"
            if order == "node" and (P.astype(np.int64)[UNITS].sum(axis=1) == 45).all():
                want = np.arange(1, 10)  # node.py:44-45: is_valid_move accepts any digit
            else:
                want = absent_digits(P, c)
            missing = np.setdiff1d(want, digits).tolist()
            extra = np.setdiff1d(digits, want).tolist()
            assert not missing, f"node {i}: candidate digits {missing} of cell {c} have no child"
            assert not extra, f"node {i}: children with digits {extra} that cell {c} cannot take"
        elif len(C) == 1 and (C[0] != 0).all():
            if answers[i] is None:
                # solved by propagation alone means one completion: only a valid grid can stand here
                assert givens_clash(g) or O.check(C[0]), f"node {i}: its only child is full but no valid grid"
            else:
                st, W = answers[i]
                assert st == 1 and np.array_equal(C[0], W), f"node {i}: full child is not the walk's solution"
        # ---- the walk's answer
        if answers[i] is None:
            continue
        st, W = answers[i]
        if st == 1:
            W = np.asarray(W, dtype=np.uint8).reshape(81)
            agree = np.array([bool((ch[ch != 0] == W[ch != 0]).all()) for ch in C], dtype=bool)
            assert agree.sum() == 1, (f"node {i}: {int(agree.sum())} of {len(C)} children agree with the walk's "
                                      f"solution, exactly one must")
            kstar = int(np.flatnonzero(agree)[0])
            bad = np.flatnonzero(~walk_fails(g, C[:kstar], order))
            assert bad.size == 0, (f"node {i}: children {bad.tolist()} stand before the one that carries the walk's "
                                   f"solution (child {kstar}) and have a completion")
            if stats is not None:
                stats["earlier"] = stats.get("earlier", 0) + kstar
        else:
            bad = np.flatnonzero(~walk_fails(g, C, order))
            assert bad.size == 0, f"node {i}: the walk fails on it, yet children {bad.tolist()} have a completion"
        # (len(C) == 0 with a solved answer fails "exactly one" above)


WALK_BUDGET = 1 << 20  # digit tests short_walk allows a board


def short_walk(board, order):
    """The literal walk's (status, solution) of a board with clean givens if
    it ends within WALK_BUDGET digit tests (a few ms), else None.  The
    oracle's timed gen.py walk looks at its clock every 2^20 tests; with the
    count reset and no time allowed it stops exactly there.  Node order is
    that walk on the board with its rows reversed: both take the first empty
    column of a row and digits ascending, gen.py rows 8..0 and node.py rows
    0..8, and reversing the rows maps rows, columns and boxes onto
    themselves (test_frontier_contract.py pins it to the fixture)."""
    g = np.asarray(board, dtype=np.uint8).reshape(9, 9)
    flip = order == "node"
    O.lib().oracle_reset_nodes()
    done, out, st = O.solve_batch_timed(np.ascontiguousarray(g[::-1] if flip else g).reshape(1, 81), 0.0)
    if done != 1:
        return None
    sol = out[0].reshape(9, 9)
    return int(st[0]), np.ascontiguousarray(sol[::-1] if flip else sol).reshape(81)


def child_answers(parents, offsets, children, answers, order):
    """The walk's answers of one level's children, from their parents' and
    the oracle: the parent's solution W for the child consistent with W;
    else (0, child) when the child has no completion, the one completion
    when it has exactly one, the literal walk's answer when it has more and
    the walk is short (short_walk), else None (structural rules only).
    Children of a parent with clashing givens get the literal walk's own
    answer.  Returns (answers list, number of None)."""
    parents = np.asarray(parents, dtype=np.uint8).reshape(-1, 81)
    children = np.ascontiguousarray(children, dtype=np.uint8).reshape(-1, 81)
    out = [None] * len(children)
    ask = []  # children with clean givens the oracle has to be asked about
    for i in range(len(parents)):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if hi == lo:
            continue
        if givens_clash(parents[i]):
            sols, st = O.solve_batch(children[lo:hi], order="node_literal" if order == "node" else "gen")
            for k in range(lo, hi):
                out[k] = (int(st[k - lo]), sols[k - lo])
            continue
        W = answers[i][1] if answers[i] is not None and answers[i][0] == 1 else None
        for k in range(lo, hi):
            ch = children[k]
            if W is not None and (ch[ch != 0] == W[ch != 0]).all():
                out[k] = (1, W)
            elif answers[i] is not None and answers[i][0] != 1:
                out[k] = (0, ch)  # below a node the walk fails on
            else:
                ask.append(k)
    if ask:
        sols, cnt = O.solve_unique_batch(children[ask])
        for k, s, c in zip(ask, sols, cnt):
            out[k] = (0, children[k]) if c == 0 else (1, s) if c == 1 else short_walk(children[k], order)
    return out, sum(a is None for a in out)


def plain_expand(nodes, order):
    """One level of the walk's tree without any propagation (the literal
    walk's own children): per node with an empty cell one child per digit
    that sudoku.py's is_valid accepts at the walk's next cell; a full node
    is its own only child.  Returns (offsets, children)."""
    nodes = np.asarray(nodes, dtype=np.uint8).reshape(-1, 81)
    kids, offsets = [], [0]
    for g in nodes:
        c = next_cell(g, order)
        if c < 0:
            kids.append(g.copy())
        else:
            for d in absent_digits(g, c):
                ch = g.copy()
                ch[c] = d
                kids.append(ch)
        offsets.append(len(kids))
    return np.array(offsets, dtype=np.int64), np.array(kids, dtype=np.uint8).reshape(-1, 81)


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/random_generated.npz as a dict of read-only arrays
    (pinned to the oracle by test_oracle.py::test_random_generated_fixture)."""
    z = np.load(os.path.join(GOLDEN, "random_generated.npz"))
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def fixture_boards(empties, order, idx=None):
    """(boards, answers) of the fixture's batch with `empties` empty cells."""
    z = fixture()
    p, st, sols = z[f"puzzles_{empties}"], z[f"{order}_status_{empties}"], z[f"{order}_solutions_{empties}"]
    idx = range(len(p)) if idx is None else idx
    return p[list(idx)], [(int(st[i]), sols[i]) for i in idx]


# ------------------------------------------------------- the GPU tests' nodes
FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"
DEAD = "123456780000000009" + "0" * 63  # cell 8 has no digit left: no completion
# clash in row 0 (cells 0 and 1 both 8) plus three blanks: completable
DUP = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]


def b81(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


def _later_open(board, W, order):
    """How many of the plain walk's children of `board` stand behind the one
    on the walk's path and have two completions or more: the children the
    oracle has no single answer for."""
    off, kids = plain_expand(board[None], order)
    k = [bool((ch[ch != 0] == W[ch != 0]).all()) for ch in kids].index(True)
    return int((O.solve_unique_batch(kids[k + 1:])[1] >= 2).sum()) if k + 1 < len(kids) else 0


@functools.lru_cache(maxsize=None)
def pick_fixture(empties, order, count):
    """`count` indices of the fixture's batch with `empties` empty cells,
    chosen on the CPU so that the oracle alone can answer most of the second
    level: boards with the fewest first-level siblings behind the walk's path
    that have several completions, then the fewest completions (capped at
    64), then the lowest index."""
    p, a = fixture_boards(empties, order)
    if len(p) <= count:
        return tuple(range(len(p)))
    key = [(_later_open(g, w[1], order), O.count_solutions(g, 64), i) for i, (g, w) in enumerate(zip(p, a))]
    return tuple(sorted(i for _, _, i in sorted(key)[:count]))


@functools.lru_cache(maxsize=None)
def node_set(order):
    """The one-level test's nodes and the walk's answers for them: 32
    fixture boards each at 58, 64 and 70 empties and the four empty boards
    (all with two completions or more), 32 one-completion 17-clue boards, a
    full valid grid, a full grid of fives, DEAD, DUP and, in node order, the
    first 16 boards of golden_sc.json (node.py's short-circuit fires on
    them).  Returns (nodes (n, 81) read-only, answers list)."""
    import json
    from sudoku_solver_distributed_amd.gen import hard17_batch
    nodes, answers = [], []
    for e in (58, 64, 70, 81):
        p, a = fixture_boards(e, order, pick_fixture(e, order, 32))
        nodes.append(p)
        answers += a
    h = hard17_batch(32, seed=23).numpy()
    sols, cnt = O.solve_unique_batch(h)
    assert (cnt == 1).all()
    nodes.append(h)
    answers += [(1, s) for s in sols]
    lit = "node_literal" if order == "node" else "gen"
    walked = np.stack([b81(FULL), b81("5" * 81), b81(DUP)])  # tractable for the literal walk
    sols, st = O.solve_batch(walked, order=lit)
    nodes.append(walked)
    answers += [(int(s), g) for s, g in zip(st, sols)]
    assert O.count_solutions(b81(DEAD), 1) == 0  # the gen walk would enumerate rows 8..1 first
    nodes.append(b81(DEAD)[None])
    answers.append((0, b81(DEAD)))
    if order == "node":
        with open(os.path.join(GOLDEN, "golden_sc.json")) as f:
            sc = json.load(f)[:16]
        nodes.append(np.stack([b81(c["puzzle"]) for c in sc]))
        answers += [(int(c["solved"]), b81(c["solution"])) for c in sc]
    nodes = np.ascontiguousarray(np.concatenate(nodes))
    nodes.setflags(write=False)
    return nodes, answers
