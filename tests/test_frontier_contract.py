"""frontier_cases.check_level on the CPU: the contract checker accepts the
walk's own levels and rejects every way a frontier level can go wrong that
the final grid of a one-completion board would never show.

Levels come from frontier_cases.plain_expand (no propagation: the literal
walk's children), four deep, on fixture boards that all have two or more
completions (58, 64, 70 and 81 empties), in both walk orders.  Answers: the
fixture's for the root; below it the same answer along the walk's own path,
"fails" for what stands in front of that path (which check_level proves one
level up with the oracle's counter), none for the siblings behind it.
"""
import numpy as np
import pytest

import frontier_cases as F

EMPTIES = (58, 64, 70, 81)
BOARDS = 24
DEPTH = 4


def _levels(order):
    """[(nodes, offsets, children, answers)] * DEPTH for the roots of all sizes."""
    roots, answers = [], []
    for e in EMPTIES:
        p, a = F.fixture_boards(e, order, range(min(BOARDS, len(F.fixture()[f"puzzles_{e}"]))))
        roots.append(p)
        answers += a
    nodes = np.concatenate(roots)
    out = []
    for _ in range(DEPTH):
        offsets, children = F.plain_expand(nodes, order)
        out.append((nodes, offsets, children, answers))
        # below: only the walk's own path and what stands in front of it keeps an
        # answer (the oracle is not asked about the siblings behind it)
        nxt = [None] * len(children)
        for i, a in enumerate(answers):
            if a is None:
                continue
            for k in range(int(offsets[i]), int(offsets[i + 1])):
                ch = children[k]
                if a[0] == 1 and (ch[ch != 0] == a[1][ch != 0]).all():
                    nxt[k] = a
                    break
                nxt[k] = (0, ch)  # in front of the walk's path (check_level proves it at this level)
        nodes, answers = children, nxt
    return out


@pytest.fixture(scope="module", params=["gen", "node"])
def levels(request):
    return request.param, _levels(request.param)


def test_plain_levels_pass(levels):
    order, lv = levels
    stats = {}
    for nodes, offsets, children, answers in lv:
        assert all(a is None or a[0] in (0, 1) for a in answers)
        F.check_level(nodes, offsets, children, order, answers, stats=stats)
    assert all(a is not None and a[0] == 1 for a in lv[0][3])  # every root is solved by the walk
    # the "everything in front fails" rule had work to do
    print(f"{order}: {stats.get('earlier', 0)} earlier siblings proven dead, "
          f"level sizes {[len(x[0]) for x in lv]}")
    assert stats.get("earlier", 0) > 0


def test_fail_predicate_is_the_fast_counters():
    """walk_fails' counter (O.solve_unique_batch, count == 0) and
    O.count_solutions(child, 1) == 0 say the same on every child in front of
    the walk's path, node order (in gen order one level-4 node's three dead
    children take the plain fast counter 7-13 s each)."""
    from oracle import oracle as O
    seen = 0
    for nodes, offsets, children, answers in _levels("node"):
        for i, a in enumerate(answers):
            if a is None:
                continue
            for ch in children[offsets[i]:offsets[i + 1]]:
                if a[0] == 1 and (ch[ch != 0] == a[1][ch != 0]).all():
                    break
                assert F.walk_fails(nodes[i], ch, "node")[0] and O.count_solutions(ch, 1) == 0, i
                seen += 1
    assert seen > 0


def test_short_walk_is_the_fixtures_walk(levels):
    """frontier_cases.short_walk (the oracle's timed gen.py walk; node order
    by reversing the rows) gives the fixture's answer wherever it finishes."""
    order, lv = levels
    nodes, _, _, answers = lv[0]
    got = [F.short_walk(g, order) for g in nodes]
    assert sum(a is not None for a in got) >= len(nodes) // 2
    for a, w in zip(got, answers):
        assert a is None or (a[0] == w[0] and np.array_equal(a[1], w[1]))


def _pick(lv, order, want):
    """(level, node) of the first node on the walk's path that `want` accepts."""
    for li, (nodes, offsets, children, answers) in enumerate(lv):
        for i, a in enumerate(answers):
            if a is not None and a[0] == 1 and want(nodes[i], children[offsets[i]:offsets[i + 1]], a[1]):
                return li, i
    raise AssertionError("no node fits the mutation")


def _splice(offsets, children, i, new):
    """The level with node i's children replaced by `new`."""
    lo, hi = int(offsets[i]), int(offsets[i + 1])
    ch = np.concatenate([children[:lo], np.asarray(new, dtype=np.uint8).reshape(-1, 81), children[hi:]])
    off = offsets.copy()
    off[i + 1:] += len(new) - (hi - lo)
    return off, ch


def _kstar(C, W):
    return [bool((ch[ch != 0] == W[ch != 0]).all()) for ch in C].index(True)


def _rejected(lv, li, off, ch, order, i, text):
    nodes, _, _, answers = lv[li]
    with pytest.raises(AssertionError, match=rf"node {i}: .*{text}"):
        F.check_level(nodes, off, ch, order, answers)


def test_mutation_drop_solution_child(levels):
    order, lv = levels
    li, i = _pick(lv, order, lambda g, C, W: len(C) >= 3)
    _, offsets, children, answers = lv[li]
    C = children[offsets[i]:offsets[i + 1]]
    k = _kstar(C, answers[i][1])
    off, ch = _splice(offsets, children, i, np.delete(C, k, axis=0))
    _rejected(lv, li, off, ch, order, i, "candidate digits|agree with the walk")
    # a node with two children left with the wrong one: only the answer rule sees it
    li, i = _pick(lv, order, lambda g, C, W: len(C) == 2)
    _, offsets, children, answers = lv[li]
    C = children[offsets[i]:offsets[i + 1]]
    off, ch = _splice(offsets, children, i, np.delete(C, _kstar(C, answers[i][1]), axis=0))
    _rejected(lv, li, off, ch, order, i, "0 of 1 children agree with the walk")


def test_mutation_drop_other_child(levels):
    order, lv = levels
    for where in ("before", "after"):
        li, i = _pick(lv, order, lambda g, C, W: len(C) >= 3 and (
            _kstar(C, W) > 0 if where == "before" else _kstar(C, W) < len(C) - 1))
        _, offsets, children, answers = lv[li]
        C = children[offsets[i]:offsets[i + 1]]
        k = _kstar(C, answers[i][1])
        off, ch = _splice(offsets, children, i, np.delete(C, k - 1 if where == "before" else len(C) - 1, axis=0))
        _rejected(lv, li, off, ch, order, i, "candidate digits .* have no child")


def test_mutation_swap_siblings(levels):
    order, lv = levels
    li, i = _pick(lv, order, lambda g, C, W: len(C) >= 2)
    _, offsets, children, _ = lv[li]
    C = children[offsets[i]:offsets[i + 1]].copy()
    C[[0, 1]] = C[[1, 0]]
    off, ch = _splice(offsets, children, i, C)
    _rejected(lv, li, off, ch, order, i, "not ascending")


def test_mutation_branch_on_other_cell(levels):
    order, lv = levels

    def other(g):
        """An empty cell that is not the walk's next and has two candidates or more."""
        for c in np.flatnonzero(g == 0):
            if c != F.next_cell(g, order) and len(F.absent_digits(g, c)) >= 2:
                return int(c)
        return -1

    li, i = _pick(lv, order, lambda g, C, W: other(g) >= 0)
    nodes, offsets, children, _ = lv[li]
    g, c = nodes[i], other(nodes[i])
    new = []
    for d in F.absent_digits(g, c):
        new.append(g.copy())
        new[-1][c] = d
    off, ch = _splice(offsets, children, i, new)
    _rejected(lv, li, off, ch, order, i, f"branches on cell {c}, the walk's next cell is {F.next_cell(g, order)}")


def test_mutation_extra_child(levels):
    order, lv = levels

    def row_digit(g):
        c = F.next_cell(g, order)
        row = g[c // 9 * 9:c // 9 * 9 + 9]
        return int(row[row != 0][0]) if (row != 0).any() else 0

    li, i = _pick(lv, order, lambda g, C, W: len(C) >= 2 and row_digit(g) > 0)
    nodes, offsets, children, _ = lv[li]
    g = nodes[i]
    c, d = F.next_cell(g, order), row_digit(g)
    C = children[offsets[i]:offsets[i + 1]]
    extra = g.copy()
    extra[c] = d
    new = sorted([*C, extra], key=lambda x: int(x[c]))  # kept in digit order: only "extra" is wrong
    off, ch = _splice(offsets, children, i, new)
    _rejected(lv, li, off, ch, order, i, rf"children with digits \[{d}\] that cell {c} cannot take")


def test_mutation_shift_offsets(levels):
    order, lv = levels
    nodes, offsets, children, answers = lv[1]
    cnt = np.diff(offsets)
    i = next(j for j in range(1, len(cnt)) if cnt[j - 1] >= 2 and cnt[j] >= 2)
    for step in (1, -1):  # node i - 1 takes node i's first child / loses its last to node i
        off = offsets.copy()
        off[i] += step
        with pytest.raises(AssertionError, match=rf"node ({i - 1}|{i}): "):
            F.check_level(nodes, off, children, order, answers)
    # offsets that no longer end at the number of children, or start past 0
    off = offsets.copy()
    off[-1] += 1
    with pytest.raises(AssertionError, match="offsets"):
        F.check_level(nodes, off, children, order, answers)
    off = offsets.copy()
    off[0] = 1
    with pytest.raises(AssertionError, match="offsets"):
        F.check_level(nodes, off, children, order, answers)
