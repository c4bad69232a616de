"""The single-board split where walk order matters (runs on an MI355X):
sdk_expand_frontier's three kernels against the contract of
frontier_cases.check_level, BatchSolver.solve_one_split and
distributed.solve_split on boards with several completions, the ordered
solve under the race it exists for, and the check / first-candidate kernels
at their block edges.

Every expectation is the committed fixture's or the oracle's; the only
comparisons between two GPU runs are the tiling and `cap` invariances, whose
untiled, uncapped side test_level_contract checks against the contract.
"""
import functools

import numpy as np
import pytest
import torch

import frontier_cases as F
from conftest import load_golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ORDERS = {"gen": 0, "node": 1}
GUARD = 8  # rows behind the children buffer that no call may touch
FILL = 0xA5


def _expand_raw(solver, nodes, order, cap=None, n=None, rows=None):
    """sdk_expand_frontier through the C ABI on a children buffer prefilled
    with FILL: (return code, offsets (n + 1,), the whole buffer (rows +
    GUARD, 81)), as numpy.  cap / n default to 9 * len(nodes) / len(nodes);
    `order` is a name or a raw code."""
    nd = torch.as_tensor(np.array(nodes), dtype=torch.uint8).reshape(-1, 81).to(solver.device)
    n = nd.shape[0] if n is None else n
    cap = 9 * nd.shape[0] if cap is None else cap
    rows = max(cap, 0) if rows is None else rows
    tmp = torch.full((nd.shape[0] + 1, 81), FILL, dtype=torch.uint8, device=solver.device)
    offsets = torch.full((nd.shape[0] + 2,), -7, dtype=torch.int64, device=solver.device)
    buf = torch.full((rows + GUARD, 81), FILL, dtype=torch.uint8, device=solver.device)
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_expand_frontier(nd.data_ptr(), n, tmp.data_ptr(), offsets.data_ptr(), buf.data_ptr(), cap,
                                            ORDERS.get(order, order),
                                            int(torch.cuda.current_stream(solver.device).cuda_stream))
        torch.cuda.synchronize()
    offsets = offsets.cpu().numpy()
    assert offsets[-1] == -7, "an offset written past n + 1 entries"
    return rc, offsets[:-1], buf.cpu().numpy()


def _expand(solver, nodes, order):
    """(offsets, children) of one level, nothing written past them."""
    rc, off, buf = _expand_raw(solver, nodes, order)
    assert rc == 0
    total = int(off[-1])
    assert 0 <= total <= len(buf) - GUARD and (buf[total:] == FILL).all()
    return off, buf[:total]


_BASE = {}


def _base(solver, order):
    """The node set's first level (one run per order, shared, read-only)."""
    if order not in _BASE:
        nodes, _ = F.node_set(order)
        off, ch = _expand(solver, nodes, order)
        off.setflags(write=False)
        ch.setflags(write=False)
        _BASE[order] = (off, ch)
    return _BASE[order]


# ------------------------------------------------------------ one level
@pytest.mark.parametrize("order", ["gen", "node"])
def test_level_contract(solver, order):
    """expand_count_kernel / scan_kernel / expand_write_kernel on ~140 nodes
    with several completions, one completion, none, clashing givens and (node
    order) node.py's short-circuit: offsets, child order, one child per
    candidate, the walk's answer kept and nothing solvable in front of it --
    on the first level and on the level below it.  Catches: the child with
    the highest (or any) candidate dropped, siblings out of order, the two
    passes disagreeing on the branch cell or the count, a subtree with the
    walk's answer lost.  On the second level the oracle has no single answer
    for 6 of 514 nodes (gen) and 3 of 576 (node): several completions and a
    literal walk longer than frontier_cases.WALK_BUDGET; those get the
    structural rules only, and at most half of the level may."""
    nodes, answers = F.node_set(order)
    off, ch = _base(solver, order)
    F.check_level(nodes, off, ch, order, answers)
    # BatchSolver.expand is the same level
    assert np.array_equal(solver.expand(torch.from_numpy(nodes.copy()), order=order).cpu().numpy(), ch)
    ans2, structural = F.child_answers(nodes, off, ch, answers, order)
    print(f"{order}: {len(nodes)} nodes, {len(ch)} children, {structural} of them without a single oracle answer "
          f"(structural rules only)")
    assert len(ch) > len(nodes) and 2 * structural <= len(ch)
    off2, ch2 = _expand(solver, ch, order)
    stats = {}
    F.check_level(ch, off2, ch2, order, ans2, stats=stats)
    print(f"{order}: second level {len(ch2)} children, {stats.get('earlier', 0)} earlier siblings proven dead")


@pytest.mark.parametrize("order", ["gen", "node"])
def test_level_shapes(solver, order):
    """The node set tiled to sizes around WAVES_PER_BLOCK (4), the scan's
    span of 1 -> 2 -> 3 nodes per thread (1024 / 1025, 2049) and a partly
    empty last block: per node the untiled run's children, offsets their
    running sum."""
    nodes, _ = F.node_set(order)
    off, ch = _base(solver, order)
    cnt = np.diff(off)
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 2049, 2500):
        idx = np.arange(n) % len(nodes)
        got_off, got = _expand(solver, nodes[idx], order)
        assert np.array_equal(got_off, np.concatenate([[0], np.cumsum(cnt[idx])])), n
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx])
        assert np.array_equal(got, ch[rows]), n


@pytest.mark.parametrize("order", ["gen", "node"])
def test_level_cap(solver, order):
    """`cap`: rows below it as the uncapped run, rows at or above it and the
    guard rows untouched, all n + 1 offsets unchanged."""
    nodes, _ = F.node_set(order)
    off, ch = _base(solver, order)
    total, n = int(off[-1]), len(nodes)
    inside = next(int(off[i]) + 1 for i in range(n // 2, n) if off[i + 1] - off[i] >= 2)
    for cap in (total, total - 1, inside, 0):
        rc, got_off, buf = _expand_raw(solver, nodes, order, cap=cap, rows=total)
        assert rc == 0
        assert np.array_equal(got_off, off), cap
        assert np.array_equal(buf[:cap], ch[:cap]), cap
        assert (buf[cap:] == FILL).all(), cap


def test_level_arguments(solver):
    nodes, _ = F.node_set("gen")
    # n == 0: offsets[0] = 0 and nothing else
    rc, off, buf = _expand_raw(solver, nodes[:1], "gen", n=0)
    assert rc == 0 and off.tolist() == [0, -7] and (buf == FILL).all()
    for kw in ({"n": -1}, {"cap": -1}, {"order": 2}):
        kw = {"order": "gen", **kw}
        rc, off, buf = _expand_raw(solver, nodes[:4], kw.pop("order"), rows=36, **kw)
        assert rc == -2, kw
        assert (off == -7).all() and (buf == FILL).all(), kw
    # a node with a byte > 9 (raw path) gets no child; its neighbours keep theirs
    base_off, base = _base(solver, "gen")
    raw = nodes[:6].copy()
    raw[2, 80] = 10
    raw[4, 0] = 255
    off, ch = _expand(solver, raw, "gen")
    cnt = np.diff(base_off[:7])
    cnt[[2, 4]] = 0
    assert np.array_equal(np.diff(off), cnt)
    keep = np.concatenate([np.arange(base_off[i], base_off[i + 1]) for i in (0, 1, 3, 5)])
    assert np.array_equal(ch, base[keep])


# ---------------------------------------------------- the split end to end
def _singles_leave_open(g):
    """Naked and hidden singles to a fixpoint leave the board undecided (no
    contradiction, not every cell settled): a solver that propagates singles
    has to guess on it.  Returns the number of undecided cells (0: refuted
    or solved).  Chooses inputs only; the test asserts the guesses."""
    c = [1 << (int(v) - 1) if v else 0x1FF for v in g]
    changed = True
    while changed:
        changed = False
        for i in range(81):
            if c[i] & (c[i] - 1):
                continue
            for p in np.flatnonzero(F.PEERS[i]):
                if c[p] & c[i]:
                    c[p] &= ~c[i]
                    changed = True
        if not all(c):
            return 0
        for u in F.UNITS:
            once = twice = 0
            for p in u:
                twice |= once & c[p]
                once |= c[p]
            if once != 0x1FF:
                return 0
            for p in u:
                x = c[p] & once & ~twice
                if x and c[p] != x:
                    if x & (x - 1):
                        return 0
                    c[p] = x
                    changed = True
    return sum(1 for x in c if x & (x - 1))


@functools.lru_cache(maxsize=None)
def _slow_dead(count, seed=11):
    """`count` boards with no completion that need search to be refuted: a
    17-clue board with one more cell filled, by a digit its only completion
    does not hold there and sudoku.py's is_valid accepts.  Per board the
    first such (cell, digit), in a seeded order of 20 of its cells, that
    singles propagation does not refute."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    pool = hard17_batch(4 * count, seed=seed).numpy()
    sols, cnt = O.solve_unique_batch(pool)
    assert (cnt == 1).all()
    rng = np.random.default_rng(seed)
    out = []
    for g, s in zip(pool, sols):  # (boards that singles alone solve take no such digit: skipped)
        for cell in rng.permutation(np.flatnonzero(g == 0))[:20]:
            h = g.copy()
            for d in range(1, 10):
                h[cell] = d
                if d != s[cell] and O.is_valid(g, int(cell) // 9, int(cell) % 9, d) and _singles_leave_open(h):
                    out.append(h)
                    break
            else:
                continue
            break
        if len(out) == count:
            break
    b = np.array(out, dtype=np.uint8)
    assert b.shape == (count, 81) and (O.solve_unique_batch(b)[1] == 0).all()
    b.setflags(write=False)
    return b


SPLIT = ((58, 12), (64, 12), (70, 12), (81, 4))


@pytest.mark.parametrize("order", ["gen", "node"])
def test_split_returns_the_walks_solution(solver, order):
    """BatchSolver.frontier / solve_one_split and distributed.solve_split
    (world of one) on boards with several completions: any solved frontier
    node is a completion, only the lowest is the walk's.  Catches a subtree
    dropped from the frontier, siblings out of order and an ordered solve
    that returns a solved node other than the lowest."""
    from sudoku_solver_distributed_amd.distributed import solve_split
    for e, k in SPLIT:
        boards, answers = F.fixture_boards(e, order, range(k))
        for i, (g, (st, want)) in enumerate(zip(boards, answers)):
            assert st == 1
            root = torch.from_numpy(g.copy())[None]
            for t in (2, 64, 700):
                ok, grid = solver.solve_one_split(root, target=t, order=order)
                assert ok is True and np.array_equal(grid.cpu().numpy(), want), (e, i, t)
            info = {}
            ok, grid = solve_split(root, order=order, target=64, chunk=5, stats=info)
            assert ok is True and np.array_equal(grid.cpu().numpy(), want), (e, i, info)


@pytest.mark.parametrize("order", ["gen", "node"])
def test_split_without_completion(solver, order):
    """(False, the board itself) for a board that needs search to be refuted
    and for one the first sweep refutes."""
    from sudoku_solver_distributed_amd.distributed import solve_split
    for g in (*_slow_dead(64)[:3], F.b81(F.DEAD)):
        root = torch.from_numpy(g.copy())[None]
        for t in (2, 64, 700):
            ok, grid = solver.solve_one_split(root, target=t, order=order)
            assert ok is False and np.array_equal(grid.cpu().numpy(), g), t
        ok, grid = solve_split(root, order=order, target=64, chunk=5)
        assert ok is False and np.array_equal(grid.cpu().numpy(), g)


# ------------------------------------------- ordered mode under its race
@pytest.mark.parametrize("k", [1, 40])
@pytest.mark.parametrize("kernel,n", [("packed", 256), ("plane", 2049), ("auto", 8192 + 64)])
def test_ordered_mode_race(solver, kernel, n, k):
    """Boards 0..k-1 are still searching (no completion, and propagation
    does not show it) when boards above k -- three empty cells, one sweep --
    solve and publish WS_BEST.  The low boards must poll the word without
    cancelling themselves (psearch: b < idx), board k (17 clues) must be
    solved, and a cancelled board's row must come back as it went in.
    Catches: a low-index board cancelled, a cancelled row overwritten, best
    not the lowest solved index, a board left unanswered."""
    from sudoku_solver_distributed_amd import _lib
    from sudoku_solver_distributed_amd.gen import hard17_batch
    slow = _slow_dead(64)[:k]
    hard = hard17_batch(1, seed=12).numpy()
    src, cnt = O.solve_unique_batch(hard17_batch(256, seed=13).numpy())
    assert (cnt == 1).all()
    easy = src.copy()
    rng = np.random.default_rng(13)
    for g in easy:
        g[rng.choice(81, 3, replace=False)] = 0
    idx = np.arange(n - k - 1) % len(easy)
    boards = np.ascontiguousarray(np.concatenate([slow, hard, easy[idx]]))
    want, wc = O.solve_unique_batch(np.concatenate([hard, easy]))
    assert (wc == 1).all()
    want = np.concatenate([slow, want[:1], want[1:][idx]])
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS[kernel])
    try:
        # precondition: the slow boards do search in the kernel that takes the
        # batch (auto: the plane kernel from 8192 boards on, the packed one below)
        if kernel == "auto":
            solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
        solver.stats(reset=True)
        _, st = solver.solve(torch.from_numpy(slow.copy()))
        solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS[kernel])
        assert (st.cpu().numpy() == 0).all()
        guesses = solver.stats(reset=True)["guesses"]
        print(f"{kernel} n={n} k={k}: {guesses} guesses on the {k} slow boards alone")
        assert guesses >= k
        sols, st = solver.solve(torch.from_numpy(boards), ordered=True)
        sols, st = sols.cpu().numpy(), st.cpu().numpy()
        stats = solver.stats()
        assert (st[:k] == 0).all(), st[:k]
        assert st[k] == 1
        assert np.isin(st[k + 1:], (1, -2)).all(), np.unique(st)
        solved = st == 1
        assert np.array_equal(sols[solved], want[solved])
        assert np.array_equal(sols[~solved], boards[~solved])
        print(f"{kernel} n={n} k={k}: {int(solved.sum()) - 1} boards above k solved, "
              f"{int((st == -2).sum())} cancelled")
        assert stats["best"] == k
        assert stats["finished"] == n
        solver.verify()
    finally:
        solver.lib.sdk_set_solve_kernel(prev)


@pytest.mark.parametrize("kernel", ["packed", "plane"])
def test_ordered_cancelled_rows_keep_input(solver, kernel):
    """Board 0 solves in one sweep and 32767 17-clue boards follow, far more
    than run at once: most are abandoned, at their start or at a poll.
    Every cancelled row is its input, every solved one the oracle's grid.
    Catches a cancelled row overwritten with a half-filled search state."""
    from sudoku_solver_distributed_amd import _lib
    from sudoku_solver_distributed_amd.gen import hard17_batch
    n = 1 << 15
    pool = hard17_batch(256, seed=14).numpy()
    want, cnt = O.solve_unique_batch(pool)
    assert (cnt == 1).all()
    idx = np.arange(n) % len(pool)
    boards, want = pool[idx].copy(), want[idx].copy()
    boards[0] = want[0]
    boards[0, [3, 40, 77]] = 0
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS[kernel])
    try:
        solver.stats(reset=True)
        sols, st = solver.solve(torch.from_numpy(boards), ordered=True)
        sols, st = sols.cpu().numpy(), st.cpu().numpy()
        stats = solver.stats()
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    print(f"{kernel}: {int((st == -2).sum())} of {n} cancelled")
    assert (st == -2).any()  # (26648 with the packed kernel, 8704 with the plane kernel)
    assert st[0] == 1 and np.isin(st, (1, -2)).all(), np.unique(st)
    assert np.array_equal(sols[st == 1], want[st == 1])
    assert np.array_equal(sols[st == -2], boards[st == -2])
    assert stats["best"] == 0 and stats["finished"] == n


# ---------------------------------- check / first_candidate at block edges
def _edge_grids():
    """Grids for the check kernels beyond the golden lists: a valid grid with
    two cells swapped within a row / a column / a box, grids whose units all
    sum to 45 with a repeat, and grids with bytes above 9 whose units still
    all sum to 45 (four cells of one box on a rectangle: +d -d / -d +d keeps
    every row, column and box sum)."""
    full = F.b81(F.FULL)
    out = []
    for a, b in ((0, 5), (3, 66), (30, 40)):  # same row / same column / same box
        g = full.copy()
        g[a], g[b] = g[b], g[a]
        out.append(g)
    for (r, c), d in (((0, 0), 1), ((3, 3), 2), ((6, 1), 1), ((0, 0), 5), ((3, 4), 1), ((6, 3), 4)):
        g = full.astype(np.int64).reshape(9, 9)
        g[r, c] += d
        g[r + 1, c + 1] += d
        g[r, c + 1] -= d
        g[r + 1, c] -= d
        assert r // 3 == (r + 1) // 3 and c // 3 == (c + 1) // 3 and g.min() >= 0
        out.append(g.reshape(81).astype(np.uint8))
    return np.stack(out)


def _sized(pool, verdicts, n):
    """n boards of the pool, cyclically, ending on one whose verdict differs
    from its neighbour's."""
    idx = list(np.arange(n - 1) % len(pool))
    prev = verdicts[idx[-1]] if idx else None
    last = next(i for i in range(len(pool)) if prev is None or verdicts[i] != prev)
    return np.array(idx + [last])


def test_check_block_edges(solver):
    """check_kernel stages 64 grids per block through LDS: batch sizes
    around it, the last board's verdict differing from its neighbour's;
    verdicts are the oracle's sum / distinct-values arithmetic on any byte."""
    golden = np.array([F.b81(c["grid"]) for c in load_golden("golden_check.json")], dtype=np.uint8)
    pool = np.concatenate([golden, _edge_grids()])
    assert pool.max() > 9
    want = {0: np.array([int(O.check(g)) for g in pool]), 1: np.array([int(O.check_sums(g)) for g in pool])}
    sums = pool.astype(np.int64)[:, F.UNITS]
    assert np.array_equal(want[1], (sums.sum(axis=2) == 45).all(axis=1).astype(int))  # node.py:82-116
    distinct = np.array([[len(set(u)) == 9 for u in g] for g in sums])
    assert np.array_equal(want[0], ((sums.sum(axis=2) == 45) & distinct).all(axis=1).astype(int))  # sudoku.py:85
    built = slice(len(golden), None)
    assert not want[0][built].any() and set(want[1][built]) == {0, 1}  # repeats fail check; sums alone split them
    for mode in (0, 1):
        for n in (1, 63, 64, 65, 129):
            idx = _sized(pool, want[mode], n)
            got = solver.check(torch.from_numpy(pool[idx]), mode).cpu().numpy()
            assert np.array_equal(got, want[mode][idx]), (mode, n)


def test_first_candidate_block_edges(solver):
    """first_candidate_kernel runs 256 boards per block: batch sizes around
    it, the last board's answer differing from its neighbour's, cells -1 and
    81 answered -1."""
    cases = load_golden("golden_node.json")["first_candidate"]
    grids = [F.b81(c["grid"]) for c in cases]
    cells = [c["row"] * 9 + c["col"] for c in cases]
    for g in _edge_grids():
        for cell in (0, 40, 80):
            grids.append(g)
            cells.append(cell)
    grids, cells = np.array(grids, dtype=np.uint8), np.array(cells)
    want = np.array([O.first_candidate(g, int(c) // 9, int(c) % 9) or 0 for g, c in zip(grids, cells)])
    for n in (1, 255, 256, 257):
        idx = _sized(grids, want, n)
        got = solver.first_candidate(torch.from_numpy(grids[idx]), cells[idx]).cpu().numpy()
        assert np.array_equal(got, want[idx]), n
        bad = cells[idx].copy()
        bad[-1] = 81
        bad[0] = -1
        got = solver.first_candidate(torch.from_numpy(grids[idx]), bad).cpu().numpy()
        assert got[-1] == -1 and got[0] == -1 and np.array_equal(got[1:-1], want[idx][1:-1]), n
