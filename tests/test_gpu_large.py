"""Every byte offset past 2^31 and 2^32 (runs on an MI355X): batches of N81 =
53 025 065 boards (4.0 GiB an array) and N162 = 26 512 921 boards (marks of
4.0 GiB) through the raw C ABI, every output row compared -- a store that
wrapped lands in a low row, and only a full compare sees it.

large_cases.py has the thresholds, the two batch builders (dense: every row a
pool board by an arithmetic rule; sparse: pool boards at both ends and 192
rows either side of every threshold, numbered fillers elsewhere), the chunked
compare and the memory budget.  Expected answers are what the suite trusts
already, one per distinct pool board, gathered by the builder's rule:
abi_arena.pool() (the oracle, both walk orders), count_cases, the oracle's
check / check_sums / first_candidate / peer_solve, the fixtures
cand_cases.json, rate_cases.json, uniq_cases.json, min_cases.json, and the
sampler's host model.  Nothing is compared with another run of the library.

Outputs are pre-filled with 0xEE and statuses with 77; inputs are compared
with their own rebuild after the call (except in place); every test asserts
the status histogram its builder implies, so a batch that silently became
all filler fails."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import abi_arena as A
import count_cases as C
import large_cases as L
from abi_arena import ORDERS, _stream_handle

pytestmark = pytest.mark.gpu

FILL, ST_FILL = 0xEE, 77
MARK_FILL = 0xEEEE - (1 << 16)  # int16 view of 0xEE 0xEE


def _dev(solver, array):
    return torch.from_numpy(np.array(array)).to(solver.device)  # (a copy: the pools are read-only)


@contextlib.contextmanager
def _timed(what):
    """The call phase on the device, by events (printed: -s shows it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    yield
    e1.record()
    torch.cuda.synchronize()
    print(f"{what}: call {e0.elapsed_time(e1) / 1e3:.3f} s")


@contextlib.contextmanager
def _kernel(solver, name):
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS[name])
    assert prev > 0
    try:
        yield
    finally:
        solver.lib.sdk_set_solve_kernel(prev)


def _has_every(values, rows_index, what):
    """The window rows hold every kind / verdict the pool has."""
    values = np.asarray(values)
    assert set(np.unique(values[rows_index])) == set(np.unique(values)), what


# -------------------------------------------------------------------- solve
@functools.lru_cache(maxsize=None)
def _solve_rule(b=12_345):
    """hard17 and gen boards in turn; every 61st row dead / clash / invalid /
    single in turn, so deferred, unsolved and rejected rows sit past both
    thresholds."""
    kinds = {k: A.kind_indices(k) for k in A.KINDS}
    rare = [kinds[k] for k in ("dead", "clash", "invalid", "single")]
    return L.Dense([kinds["hard17"], kinds["gen"]], rare=rare, b=b)


def _solve_raw(solver, p, out, st, order):
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_solve_batch_grid(p.data_ptr(), out.data_ptr(), st.data_ptr(), p.shape[0],
                                             solver.workspace.data_ptr(), ORDERS[order], 0, _stream_handle(solver), 0)
    assert rc == 0, solver.lib.sdk_last_error()


def _plane_solve(solver, order, in_place):
    P, D, n, dev = A.pool(), _solve_rule(), L.N81, solver.device
    boards, (wr, ws) = _dev(solver, P["boards"]), (_dev(solver, x) for x in P["want"][order])
    _has_every(P["kind"], D.index(L.windows(n, 81)), "kinds in the windows")
    p = L.build(n, lambda lo, hi: D.gather(boards, lo, hi), dev)
    L.self_check(p, D, P["boards"], n, 81)
    out = p if in_place else L.filled(n, 81, torch.uint8, FILL, dev)
    st = L.filled(n, 0, torch.int32, ST_FILL, dev)
    with _kernel(solver, "plane"):
        solver.stats(reset=True)
        with _timed(f"solve plane {order}{' in place' if in_place else ''}"):
            _solve_raw(solver, p, out, st, order)
        stats = solver.stats()
    L.compare(st, lambda lo, hi: D.gather(ws, lo, hi), n, "status")
    L.compare(out, lambda lo, hi: D.gather(wr, lo, hi), n, "solutions")
    if not in_place:
        L.compare(p, lambda lo, hi: D.gather(boards, lo, hi), n, "puzzles after the call")
    want = D.histogram(n, P["want"][order][1])
    assert L.histogram(st, n) == want and want[1] > n // 2 and want[0] > 0 and want[-1] > 0
    assert stats["finished"] == n and stats["deferred"] > n // 61 // 8
    solver.verify()


def test_solve_plane_gen(solver):
    """The plane kernel, order gen, out of place: puzzles read and solutions
    written past 2^32 (the span loads' clamped num_records, the partial last
    dword of a batch more than 4 GiB long, the bit-slice stores)."""
    with L.budget(10 * L.GIB):
        _plane_solve(solver, "gen", in_place=False)


def test_solve_plane_node_in_place(solver):
    """Order node, d_solutions == d_puzzles: one array read and written."""
    with L.budget(6 * L.GIB):
        _plane_solve(solver, "node", in_place=True)


def test_solve_batches(solver):
    """sdk_solve_batches, three batches of 5, N81 and 70 001 rows in one
    launch sequence: local(p) * 81 of batch 1 passes 2^32."""
    import ctypes

    def body():
        P, dev, order = A.pool(), solver.device, "gen"
        boards, (wr, ws) = _dev(solver, P["boards"]), (_dev(solver, x) for x in P["want"][order])
        sizes = (5, L.N81, 70_001)
        rules = [_solve_rule(b) for b in (7, 12_345, 99)]
        ps = [L.build(n, lambda lo, hi, D=D: D.gather(boards, lo, hi), dev) for n, D in zip(sizes, rules)]
        L.self_check(ps[1], rules[1], P["boards"], sizes[1], 81)
        outs = [L.filled(n, 81, torch.uint8, FILL, dev) for n in sizes]
        sts = [L.filled(n, 0, torch.int32, ST_FILL, dev) for n in sizes]
        arr = ctypes.c_void_p * 3
        with _kernel(solver, "plane"):
            solver.stats(reset=True)
            with _timed("solve_batches"), torch.cuda.device(dev):
                rc = solver.lib.sdk_solve_batches(arr(*[p.data_ptr() for p in ps]), arr(*[o.data_ptr() for o in outs]),
                                                  arr(*[s.data_ptr() for s in sts]), (ctypes.c_int64 * 3)(*sizes), 3,
                                                  solver.workspace.data_ptr(), ORDERS[order], _stream_handle(solver), 0)
                assert rc == 0, solver.lib.sdk_last_error()
            stats = solver.stats()
        for k, (n, D) in enumerate(zip(sizes, rules)):
            L.compare(sts[k], lambda lo, hi: D.gather(ws, lo, hi), n, f"status of batch {k}")
            L.compare(outs[k], lambda lo, hi: D.gather(wr, lo, hi), n, f"solutions of batch {k}")
            L.compare(ps[k], lambda lo, hi: D.gather(boards, lo, hi), n, f"puzzles of batch {k} after the call")
            assert L.histogram(sts[k], n) == D.histogram(n, P["want"][order][1])
        assert stats["finished"] == sum(sizes)
        solver.verify()
    with L.budget(10 * L.GIB):
        body()


def test_solve_packed(solver):
    """The wave-per-board kernel forced: puzzles + p * 81 and sols + p * 81
    past 2^32.  Sparse: a wave a board is too slow for 53 M real boards."""
    def body():
        P, n, dev, order = A.pool(), L.N81, solver.device, "node"
        S = L.Sparse(n, 81, len(P["boards"]), seed=1)
        boards, (wr, ws) = _dev(solver, P["boards"]), (_dev(solver, x) for x in P["want"][order])
        assert len(np.unique(S.picks)) == len(P["boards"])
        p = L.build(n, lambda lo, hi: S.gather(boards, lo, hi, L.filler_boards), dev)
        L.self_check(p, S, P["boards"], n, 81, fillers=True)
        out, st = L.filled(n, 81, torch.uint8, FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        with _kernel(solver, "packed"):
            solver.stats(reset=True)
            with _timed("solve packed"):
                _solve_raw(solver, p, out, st, order)
            stats = solver.stats()
        L.compare(st, lambda lo, hi: S.gather(ws, lo, hi, L.constant(-1, 0, torch.int32)), n, "status")
        L.compare(out, lambda lo, hi: S.gather(wr, lo, hi, L.filler_boards), n, "solutions")
        L.compare(p, lambda lo, hi: S.gather(boards, lo, hi, L.filler_boards), n, "puzzles after the call")
        want = S.histogram(n, P["want"][order][1], -1)
        assert L.histogram(st, n) == want and want[1] > len(S.rows) // 2
        assert stats["finished"] == n
        solver.verify()
    with L.budget(10 * L.GIB):
        body()


# ------------------------------------------------- check, first_candidate
def test_check(solver):
    """Sudoku.check and node.py's check over solved grids and near-misses:
    grids + g0 * 81 of the block's staging loop."""
    from test_gpu_abi_buffers import _check_cases

    def body():
        grids, want = _check_cases()
        n, dev = L.N81, solver.device
        D = L.Dense([np.arange(len(grids))])
        for mode in (0, 1):
            _has_every(want[mode], D.index(L.windows(n, 81)), f"verdicts of mode {mode} in the windows")
        table = _dev(solver, grids)
        g = L.build(n, lambda lo, hi: D.gather(table, lo, hi), dev)
        L.self_check(g, D, grids, n, 81)
        for mode in (0, 1):
            ok, w = L.filled(n, 0, torch.int32, ST_FILL, dev), _dev(solver, want[mode])
            with _timed(f"check mode {mode}"), torch.cuda.device(dev):
                assert solver.lib.sdk_check_batch(g.data_ptr(), ok.data_ptr(), n, mode, _stream_handle(solver)) == 0
            L.compare(ok, lambda lo, hi: D.gather(w, lo, hi), n, f"ok, mode {mode}")
            hist = D.histogram(n, want[mode])
            assert L.histogram(ok, n) == hist and hist[0] > 0 and hist[1] > 0
        L.compare(g, lambda lo, hi: D.gather(table, lo, hi), n, "grids after the calls")
    with L.budget(6 * L.GIB):
        body()


def test_first_candidate(solver):
    from test_gpu_abi_buffers import _candidate_cases

    def body():
        grids, cells, want = _candidate_cases()
        n, dev = L.N81, solver.device
        D = L.Dense([np.arange(len(grids))])
        _has_every(want, D.index(L.windows(n, 81)), "answers in the windows")
        tg, tc, tw = _dev(solver, grids), _dev(solver, cells), _dev(solver, want)
        g = L.build(n, lambda lo, hi: D.gather(tg, lo, hi), dev)
        c = L.build(n, lambda lo, hi: D.gather(tc, lo, hi), dev)
        L.self_check(g, D, grids, n, 81)
        L.self_check(c, D, cells, n, 4)
        num = L.filled(n, 0, torch.int32, ST_FILL, dev)
        with _timed("first_candidate"), torch.cuda.device(dev):
            assert solver.lib.sdk_first_candidate_batch(g.data_ptr(), c.data_ptr(), num.data_ptr(), n,
                                                        _stream_handle(solver)) == 0
        L.compare(num, lambda lo, hi: D.gather(tw, lo, hi), n, "num")
        L.compare(g, lambda lo, hi: D.gather(tg, lo, hi), n, "grids after the call")
        L.compare(c, lambda lo, hi: D.gather(tc, lo, hi), n, "cells after the call")
        hist = D.histogram(n, want)
        assert L.histogram(num, n) == hist and len(hist) > 2
    with L.budget(6 * L.GIB):
        body()


# --------------------------------------------------------------- peer_solve
def test_peer_solve(solver):
    """One thread a board: boards + i * 81 and out + i * 81 past 2^31."""
    from test_gpu_abi_buffers import _peer_cases

    def body():
        boards, rows, status, vals = _peer_cases()
        n, dev = L.R31 + 777, solver.device
        S = L.Sparse(n, 81, len(boards), seed=2)
        assert len(np.unique(S.picks)) == len(boards)
        tb, tr, ts, tv = (_dev(solver, x) for x in (boards, rows, status, vals))
        b = L.build(n, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), dev)
        L.self_check(b, S, boards, n, 81, fillers=True)
        out = L.filled(n, 81, torch.uint8, FILL, dev)
        st, val = L.filled(n, 0, torch.int32, ST_FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        with _timed("peer_solve"), torch.cuda.device(dev):
            assert solver.lib.sdk_peer_solve_batch(b.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                                   _stream_handle(solver)) == 0
        L.compare(st, lambda lo, hi: S.gather(ts, lo, hi, L.constant(-1, 0, torch.int32)), n, "status")
        L.compare(val, lambda lo, hi: S.gather(tv, lo, hi, L.constant(0, 0, torch.int32)), n, "validations")
        L.compare(out, lambda lo, hi: S.gather(tr, lo, hi, L.filler_boards), n, "out")
        L.compare(b, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), n, "boards after the call")
        want = S.histogram(n, status, -1)
        assert L.histogram(st, n) == want and sum(c for v, c in want.items() if v != -1) == len(S.rows)
    with L.budget(6 * L.GIB):
        body()


# ---------------------------------------------------------- count_solutions
def test_count_solutions(solver):
    """limit 2 with d_first: puzzles + p * 81 and first + p * 81 past 2^32.
    d_first is the board's one completion or the input where the count says
    so; where a board has two or more, a valid grid that keeps its givens."""
    def body():
        boards, fixed, uniq, is_unique, names = C.pool()
        want = C.expected(2)
        n, dev = L.N81, solver.device
        D = L.Dense([np.flatnonzero(names == k) for k in "abcde"], rare=[np.flatnonzero(names == "f")])
        _has_every(want, D.index(L.windows(n, 81)), "counts in the windows")
        first_want = np.where((want == 1)[:, None], uniq, boards)
        assert is_unique[want == 1].all()
        tb, tw, tf = _dev(solver, boards), _dev(solver, want), _dev(solver, first_want)
        many = _dev(solver, want == 2)
        p = L.build(n, lambda lo, hi: D.gather(tb, lo, hi), dev)
        L.self_check(p, D, boards, n, 81)
        need = int(solver.lib.sdk_count_scratch_bytes(n, 0))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        first, count = L.filled(n, 81, torch.uint8, FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        with _timed("count_solutions"), torch.cuda.device(dev):
            assert solver.lib.sdk_count_solutions_batch(p.data_ptr(), count.data_ptr(), first.data_ptr(), n, 2,
                                                        scratch.data_ptr(), need, 0, _stream_handle(solver)) == 0
        L.compare(count, lambda lo, hi: D.gather(tw, lo, hi), n, "count")

        def completes(rows, at):  # a board with two or more completions: any of them
            idx = D.index(at)
            given = tb[idx]
            return many[idx] & L.valid_rows(rows) & ((given == 0) | (rows == given)).all(dim=1)
        L.compare(first, lambda lo, hi: D.gather(tf, lo, hi), n, "first", accept=completes)
        L.compare(p, lambda lo, hi: D.gather(tb, lo, hi), n, "puzzles after the call")
        hist = D.histogram(n, want)
        assert L.histogram(count, n) == hist and set(hist) == {-1, 0, 1, 2}
    with L.budget(14 * L.GIB):
        body()


# ------------------------------------- candidates, unique_candidates, rate
def _i16(marks):
    """Marks (at most 0x1FF) as the int16 torch compares."""
    return np.asarray(marks).astype(np.int16)


def _scratch(solver, need):
    return torch.empty(int(need), dtype=torch.uint8, device=solver.device)


def test_candidates(solver):
    """marks + p * 81 (162 bytes a row) past 2^32 and boards + p * 81 past
    2^31.  Every row is a fixture board: its one-completion boards by the
    dense rule, the whole fixture (the heavy boards too) in the windows."""
    import cand_cases as K

    def body():
        names, boards, marks, count = K.load_fixture()
        n, dev = L.N162, solver.device
        W = L.Windowed(n, (81, 162), len(boards), L.Dense([np.flatnonzero(count == 1)]), seed=3)
        assert len(np.unique(W.picks)) == len(boards)
        tb, tm, tc = _dev(solver, boards), _dev(solver, _i16(marks)), _dev(solver, count)
        b = L.build(n, lambda lo, hi: W.gather(tb, lo, hi), dev)
        L.self_check(b, W, boards, n, (81, 162))
        out, cnt = L.filled(n, 81, torch.int16, MARK_FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        need = solver.lib.sdk_candidates_scratch_bytes(n, 0)
        scratch = _scratch(solver, need)
        with _timed("candidates"), torch.cuda.device(dev):
            assert solver.lib.sdk_candidates_batch(b.data_ptr(), out.data_ptr(), cnt.data_ptr(), n, scratch.data_ptr(),
                                                   need, 0, _stream_handle(solver)) == 0
        L.compare(cnt, lambda lo, hi: W.gather(tc, lo, hi), n, "count")
        L.compare(out, lambda lo, hi: W.gather(tm, lo, hi), n, "marks")
        L.compare(b, lambda lo, hi: W.gather(tb, lo, hi), n, "boards after the call")
        want = W.histogram(n, count)
        assert L.histogram(cnt, n) == want and set(want) == {-1, 0, 1, 2} and want[1] > n - len(W.rows)
    with L.budget(12 * L.GIB):
        body()


def test_unique_candidates(solver):
    """once and marks, both 162 bytes a row, past 2^32.  Sparse: 2.8 M boards
    a second would make 26 M real boards ten seconds."""
    import uniq_cases as U

    def body():
        names, boards, once, marks, count = U.load_fixture()
        n, dev = L.N162, solver.device
        S = L.Sparse(n, (81, 162), len(boards), seed=4)
        assert len(np.unique(S.picks)) == len(boards)
        tb, to, tm, tc = _dev(solver, boards), _dev(solver, _i16(once)), _dev(solver, _i16(marks)), _dev(solver, count)
        b = L.build(n, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), dev)
        L.self_check(b, S, boards, n, (81, 162), fillers=True)
        d_once, d_marks = (L.filled(n, 81, torch.int16, MARK_FILL, dev) for _ in range(2))
        cnt = L.filled(n, 0, torch.int32, ST_FILL, dev)
        waves = 2048  # (a full grid's stacks, 2.7 GiB, are not needed: the fillers end at once)
        need = solver.lib.sdk_unique_candidates_scratch_bytes(n, waves)
        scratch = _scratch(solver, need)
        with _timed("unique_candidates"), torch.cuda.device(dev):
            assert solver.lib.sdk_unique_candidates_batch(b.data_ptr(), d_once.data_ptr(), d_marks.data_ptr(),
                                                          cnt.data_ptr(), n, scratch.data_ptr(), need, waves,
                                                          _stream_handle(solver)) == 0
        zero = L.constant(0, 81, torch.int16)
        L.compare(cnt, lambda lo, hi: S.gather(tc, lo, hi, L.constant(-1, 0, torch.int32)), n, "count")
        L.compare(d_once, lambda lo, hi: S.gather(to, lo, hi, zero), n, "once")
        L.compare(d_marks, lambda lo, hi: S.gather(tm, lo, hi, zero), n, "marks")
        L.compare(b, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), n, "boards after the call")
        want = S.histogram(n, count, -1)
        assert L.histogram(cnt, n) == want and want[1] > 0 and want[2] > 0 and want[0] > 0
    with L.budget(14 * L.GIB):
        body()


def _rate_call(solver, b, n, level, what):
    dev = solver.device
    rating, opens = L.filled(n, 0, torch.int32, ST_FILL, dev), L.filled(n, 4, torch.int32, ST_FILL, dev)
    marks = L.filled(n, 81, torch.int16, MARK_FILL, dev)
    need = solver.lib.sdk_rate_scratch_bytes(n, level)
    scratch = _scratch(solver, need)
    with _timed(what), torch.cuda.device(dev):
        assert solver.lib.sdk_rate_batch(b.data_ptr(), rating.data_ptr(), opens.data_ptr(), marks.data_ptr(), n, level,
                                         scratch.data_ptr(), need, _stream_handle(solver)) == 0
    return rating, opens, marks


def test_rate_level_4(solver):
    """max_level 4 with marks and open: marks past 2^32 from both kernels (the
    trial kernel writes the boards level 3 leaves open).  Sparse: 21 M/s."""
    import rate_cases as R

    def body():
        names, boards, rating, opens, marks = R.load_fixture()
        n, dev = L.N162, solver.device
        S = L.Sparse(n, (81, 162), len(boards), seed=5)
        assert len(np.unique(S.picks)) == len(boards)
        tb, tr, to, tm = _dev(solver, boards), _dev(solver, rating), _dev(solver, opens), _dev(solver, _i16(marks))
        b = L.build(n, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), dev)
        L.self_check(b, S, boards, n, (81, 162), fillers=True)
        d_rating, d_open, d_marks = _rate_call(solver, b, n, 4, "rate level 4")
        L.compare(d_rating, lambda lo, hi: S.gather(tr, lo, hi, L.constant(-1, 0, torch.int32)), n, "rating")
        L.compare(d_open, lambda lo, hi: S.gather(to, lo, hi, L.constant(-1, 4, torch.int32)), n, "open")
        L.compare(d_marks, lambda lo, hi: S.gather(tm, lo, hi, L.constant(0, 81, torch.int16)), n, "marks")
        L.compare(b, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), n, "boards after the call")
        want = S.histogram(n, rating, -1)
        assert L.histogram(d_rating, n) == want and set(want) == {-1, 0, 1, 2, 3, 4, 5}
    with L.budget(9 * L.GIB):
        body()


def test_rate_level_3(solver):
    """max_level 3, every row one of the fixture boards that levels 1..3
    settle (solved, or dead by then): rate_kernel alone, at its own rate."""
    import rate_cases as R

    def body():
        names, boards, rating, opens, marks = R.load_fixture()
        at3 = [R.at_level(r, o, 3) for r, o in zip(rating, opens)]
        keep = np.array([k for k, (r, o, known) in enumerate(at3) if known and r <= 3])
        boards, marks = boards[keep], marks[keep]
        rating = np.array([at3[k][0] for k in keep], dtype=np.int32)
        opens = np.array([at3[k][1] for k in keep], dtype=np.int32)
        assert set(rating) == {0, 1, 2, 3} and (opens[:, 3] == R.NOT_RUN).all()
        n, dev = L.N162, solver.device
        D = L.Dense([np.arange(len(boards))])
        _has_every(rating, D.index(L.windows(n, (81, 162))), "ratings in the windows")
        tb, tr, to, tm = _dev(solver, boards), _dev(solver, rating), _dev(solver, opens), _dev(solver, _i16(marks))
        b = L.build(n, lambda lo, hi: D.gather(tb, lo, hi), dev)
        L.self_check(b, D, boards, n, (81, 162))
        d_rating, d_open, d_marks = _rate_call(solver, b, n, 3, "rate level 3")
        L.compare(d_rating, lambda lo, hi: D.gather(tr, lo, hi), n, "rating")
        L.compare(d_open, lambda lo, hi: D.gather(to, lo, hi), n, "open")
        L.compare(d_marks, lambda lo, hi: D.gather(tm, lo, hi), n, "marks")
        L.compare(b, lambda lo, hi: D.gather(tb, lo, hi), n, "boards after the call")
        assert L.histogram(d_rating, n) == D.histogram(n, rating)
    with L.budget(9 * L.GIB):
        body()


# ----------------------------------------------------------------- minimize
def test_minimize(solver):
    """Greedy with d_order: boards, order and out past 2^32.  Sparse (1 to 10
    M boards a second); the fillers' order rows are all 255."""
    import min_cases as M

    def body():
        fx = M.load_fixture()
        pick = np.flatnonzero((fx["mode"] == M.GREEDY) & (fx["max_empty"] == 81))
        boards, order, rows = fx["boards"][pick], fx["order"][pick], fx["out"][pick]
        status, removed = fx["status"][pick], fx["removed"][pick]
        n, dev = L.N81, solver.device
        S = L.Sparse(n, 81, len(boards), seed=6)
        assert len(np.unique(S.picks)) == len(boards)
        tb, to, tr, ts, tv = (_dev(solver, x) for x in (boards, order, rows, status, removed))
        skip = L.constant(255, 81, torch.uint8)
        b = L.build(n, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), dev)
        o = L.build(n, lambda lo, hi: S.gather(to, lo, hi, skip), dev)
        L.self_check(b, S, boards, n, 81, fillers=True)
        L.self_check(o, S, order, n, 81)
        out = L.filled(n, 81, torch.uint8, FILL, dev)
        st, rem = L.filled(n, 0, torch.int32, ST_FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        waves = 1024  # (three arrays of 4 GiB: no room for a full grid's stacks, and the fillers end at once)
        need = solver.lib.sdk_minimize_scratch_bytes(n, waves)
        scratch = _scratch(solver, need)
        with _timed("minimize"), torch.cuda.device(dev):
            assert solver.lib.sdk_minimize_batch(b.data_ptr(), o.data_ptr(), out.data_ptr(), st.data_ptr(),
                                                 rem.data_ptr(), n, M.GREEDY, 81, scratch.data_ptr(), need, waves,
                                                 _stream_handle(solver)) == 0
        L.compare(st, lambda lo, hi: S.gather(ts, lo, hi, L.constant(-1, 0, torch.int32)), n, "status")
        L.compare(rem, lambda lo, hi: S.gather(tv, lo, hi, L.constant(0, 0, torch.int32)), n, "removed")
        L.compare(out, lambda lo, hi: S.gather(tr, lo, hi, L.filler_boards), n, "out")
        L.compare(b, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), n, "boards after the call")
        L.compare(o, lambda lo, hi: S.gather(to, lo, hi, skip), n, "order after the call")
        want = S.histogram(n, status, -1)
        assert L.histogram(st, n) == want and want[1] > 0 and want[2] > 0 and want[0] > 0
    with L.budget(14.5 * L.GIB):
        body()


# --------------------------------------------------- sample, random_grids
SAMPLE_SEED = 1


def test_sample(solver):
    """per_board 3 with first_key just below 2^64: item q samples board q / 3
    under key first_key + q, which wraps in the middle of the batch, and
    writes row q of an out array past 2^32.  Sparse in ITEM space: the real
    boards are those of the items in the windows and 64 boards around the
    item whose key is 0; their grids are the host model's at their own keys.
    A filler board's three items return it as given."""
    import native_build
    import sample_cases as SC

    def body():
        host = native_build.host_lib("sample_host")
        sets = C.sets()
        pool = np.concatenate([sets["a"][:32], sets["b"][:32], sets["d"][:32], sets["e"][:8], sets["f"]])
        per, dev = 3, solver.device
        nb = -(-L.N81 // per)
        items = nb * per
        assert items >= L.N81 and items * 81 > L.T32 and nb * 81 < L.T31
        first_key = 2 ** 64 - items // 2
        wrap = (2 ** 64 - first_key) // per  # the board whose items see the key pass 0
        rows = np.unique(np.concatenate([L.windows(items, 81) // per, np.arange(wrap - 32, wrap + 32)]))
        B = L.Sparse(nb, 81, len(pool), seed=7, rows=rows)
        assert len(np.unique(B.picks)) == len(pool)
        want_out, want_st = [], []
        for lo, hi in L.runs_of(rows):
            o, s = SC.host_sample(host, pool[B.index(np.arange(lo, hi))], SAMPLE_SEED, per,
                                  (first_key + per * lo) % 2 ** 64)
            want_out.append(o)
            want_st.append(s)
        want_out, want_st = np.concatenate(want_out), np.concatenate(want_st)
        item_rows = (per * rows[:, None] + np.arange(per)).ravel()
        IT = L.Sparse(items, 81, len(item_rows), rows=item_rows, picks=np.arange(len(item_rows)))
        assert set(L.windows(items, 81)) <= set(item_rows)
        tb, to, ts = _dev(solver, pool), _dev(solver, want_out), _dev(solver, want_st)
        b = L.build(nb, lambda lo, hi: B.gather(tb, lo, hi, L.filler_boards), dev)
        L.self_check(b, B, pool, nb, 81, fillers=True)
        out, st = L.filled(items, 81, torch.uint8, FILL, dev), L.filled(items, 0, torch.int32, ST_FILL, dev)
        waves = 2048
        need = solver.lib.sdk_sample_scratch_bytes(items, waves)
        scratch = _scratch(solver, need)
        with _timed("sample"), torch.cuda.device(dev):
            assert solver.lib.sdk_sample_batch(b.data_ptr(), out.data_ptr(), st.data_ptr(), nb, per, SAMPLE_SEED,
                                               first_key, scratch.data_ptr(), need, waves, _stream_handle(solver)) == 0
        L.compare(st, lambda lo, hi: IT.gather(ts, lo, hi, L.constant(-1, 0, torch.int32)), items, "status")
        given = lambda a, z, d: L.filler_boards(a, z, d, per)  # noqa: E731 (a filler's items return their board)
        L.compare(out, lambda lo, hi: IT.gather(to, lo, hi, given), items, "out")
        L.compare(b, lambda lo, hi: B.gather(tb, lo, hi, L.filler_boards), nb, "boards after the call")
        want = IT.histogram(items, want_st, -1)
        assert L.histogram(st, items) == want and want[1] > len(item_rows) // 2 and want[0] > 0
    with L.budget(9 * L.GIB):
        body()


def test_random_grids(solver):
    """NULL boards: N81 random full grids, out past 2^32.  Every row is a
    valid grid (large_cases.valid_rows), every status 1, and the rows in the
    windows are the host model's at their keys."""
    import native_build
    import sample_cases as SC

    def body():
        host = native_build.host_lib("sample_host")
        n, dev, first_key = L.N81, solver.device, 40
        out, st = L.filled(n, 81, torch.uint8, FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        need = solver.lib.sdk_sample_scratch_bytes(n, 0)
        scratch = _scratch(solver, need)
        with _timed("random_grids"), torch.cuda.device(dev):
            assert solver.lib.sdk_sample_batch(None, out.data_ptr(), st.data_ptr(), n, 1, SAMPLE_SEED, first_key,
                                               scratch.data_ptr(), need, 0, _stream_handle(solver)) == 0
        assert L.histogram(st, n) == {1: n}
        for lo in range(0, n, 1 << 20):
            ok = L.valid_rows(out[lo:lo + (1 << 20)])
            assert bool(ok.all()), f"row {lo + int(torch.nonzero(~ok)[0, 0])} is no valid grid"
        for lo, hi in L.runs_of(L.windows(n, 81)):
            want, status = SC.host_sample(host, None, SAMPLE_SEED, 1, first_key + lo, n=hi - lo)
            assert (status == 1).all() and np.array_equal(out[lo:hi].cpu().numpy(), want), f"rows [{lo}, {hi})"
    with L.budget(8 * L.GIB):
        body()


# ---------------------------------------------------------------- canonical
def test_canonical(solver):
    """slices = 2592: 64 * 2592 bytes of scratch records a board, so board
    12 946's records pass 2^31 and board 25 891's 2^32 ((board * slices + s) *
    RECORD_WORDS in both kernels).  Sparse with windows around both; canon
    from canon_cases.json, sym through gen.apply_symmetry, autos from the
    host build of canon.h."""
    from conftest import load_golden
    import frontier_cases as F
    import native_build
    from sudoku_solver_distributed_amd import gen
    from test_canon_host import _canon

    def body():
        doc = load_golden("canon_cases.json")["cases"]
        boards = np.stack([F.b81(c["board"]) for c in doc])
        canon = np.stack([F.b81(c["canon"]) for c in doc])
        host_canon, host_sym, autos = _canon(native_build.host_lib("canon_host", openmp=True), boards)
        assert np.array_equal(host_canon, canon)
        n, slices, dev = L.C32 + 7, L.CANON_SLICES, solver.device
        need = solver.lib.sdk_canonical_scratch_bytes(n, slices)
        assert need == 64 * slices * n > L.T32
        S = L.Sparse(n, 64 * slices, len(boards), seed=8)
        assert len(np.unique(S.picks)) == len(boards) and L.C31 in S.rows and L.C32 in S.rows and L.C32 - 1 in S.rows
        tb, tc, ts, ta = (_dev(solver, x) for x in (boards, canon, host_sym, autos))
        b = L.build(n, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), dev)
        L.self_check(b, S, boards, n, 64 * slices, fillers=True)
        out = L.filled(n, 81, torch.uint8, FILL, dev)
        sym, aut = L.filled(n, 0, torch.int32, ST_FILL, dev), L.filled(n, 0, torch.int32, ST_FILL, dev)
        scratch = _scratch(solver, need)
        for lo in range(0, need, 1 << 30):
            scratch[lo:lo + (1 << 30)].fill_(FILL)
        with _timed("canonical"), torch.cuda.device(dev):
            assert solver.lib.sdk_canonical_batch(b.data_ptr(), out.data_ptr(), sym.data_ptr(), aut.data_ptr(), n,
                                                  slices, scratch.data_ptr(), need, _stream_handle(solver)) == 0
        L.compare(out, lambda lo, hi: S.gather(tc, lo, hi, L.filler_boards), n, "canon")
        L.compare(sym, lambda lo, hi: S.gather(ts, lo, hi, L.constant(-1, 0, torch.int32)), n, "sym")
        L.compare(aut, lambda lo, hi: S.gather(ta, lo, hi, L.constant(-1, 0, torch.int32)), n, "autos")
        L.compare(b, lambda lo, hi: S.gather(tb, lo, hi, L.filler_boards), n, "boards after the call")
        got = sym.cpu().numpy()
        real = np.zeros(n, dtype=bool)
        real[S.rows] = True
        assert (got[~real] == -1).all() and (got[real] >= 0).all() and int(real.sum()) == len(S.rows)
        assert np.array_equal(gen.apply_symmetry(boards[S.picks], got[S.rows])[0], canon[S.picks])
    with L.budget(6 * L.GIB):
        body()


# ---------------------------------------------------------- expand_frontier
def _expand_raw(solver, nodes, tmp, offsets, children, cap, order):
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_expand_frontier(nodes.data_ptr(), nodes.shape[0], tmp.data_ptr(), offsets.data_ptr(),
                                            children.data_ptr(), cap, ORDERS[order], _stream_handle(solver))
    assert rc == 0, solver.lib.sdk_last_error()


def test_expand_frontier(solver):
    """R31 + 777 nodes with more than R32 children: nodes and tmp past 2^31,
    children + o * 81 past 2^32.  Dense over distinct nodes of
    frontier_cases.node_set chosen (by a call on them alone, used for nothing
    but their child counts) so that a node has a little over two children on
    average.  The first rows of the large call hold every distinct node once:
    frontier_cases.check_level checks those against the oracle, and every
    other node's children must be its first copy's, row for row; offsets are
    the running sum.  cap is the total exactly, then the total less five:
    the rows from cap on keep their fill."""
    import frontier_cases as F

    def body():
        order, dev = "gen", solver.device
        nodes, answers = F.node_set(order)
        k = len(nodes)
        sizing = [_dev(solver, nodes), L.filled(k, 81, torch.uint8, FILL, dev),
                  torch.zeros(k + 1, dtype=torch.int64, device=dev), L.filled(9 * k, 81, torch.uint8, FILL, dev)]
        _expand_raw(solver, *sizing, 9 * k, order)
        kids = np.diff(sizing[2].cpu().numpy())
        by_count = np.argsort(kids, kind="stable")
        sel = [int(i) for i in by_count if kids[i] <= 2]
        for i in by_count[len(sel):][::-1]:  # the widest nodes first, while the mean stays near two
            if (kids[sel].sum() + kids[i]) / (len(sel) + 1) <= 2.3:
                sel.append(int(i))
        sel = np.array(sorted(sel))
        mean = kids[sel].mean()
        assert 2.05 <= mean <= 2.3 and kids[sel].min() == 0 and kids[sel].max() >= 3, (mean, kids[sel])
        assert len(sel) <= L.SPAN
        nodes, answers, kids = nodes[sel], [answers[i] for i in sel], kids[sel]
        n = L.R31 + 777
        D = L.Dense([np.arange(len(nodes))])
        total = int((D.counts(n, len(nodes)) * kids).sum())
        assert total > L.R32 + 777 and n * 81 > L.T31
        tn, tk = _dev(solver, nodes), _dev(solver, kids.astype(np.int64))
        d_nodes = L.build(n, lambda lo, hi: D.gather(tn, lo, hi), dev)
        L.self_check(d_nodes, D, nodes, n, 81)
        # the running sum, chunk by chunk
        want_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        run = 0
        for lo, hi in L.chunks(n):
            want_off[lo + 1:hi + 1] = torch.cumsum(D.gather(tk, lo, hi), dim=0) + run
            run = int(want_off[hi])
        assert run == total
        tmp = L.filled(n, 81, torch.uint8, FILL, dev)
        offsets = L.filled(n + 1, 0, torch.int64, ST_FILL, dev)
        children = L.filled(total + 8, 81, torch.uint8, FILL, dev)
        with _timed("expand_frontier"):
            _expand_raw(solver, d_nodes, tmp, offsets, children, total, order)
        L.compare(offsets, lambda lo, hi: want_off[lo:hi], n + 1, "offsets")
        # every distinct node once in the first rows: the contract against the oracle, and the table
        first = len(nodes)
        head = D.index(np.arange(first))
        assert sorted(head) == list(range(first))
        off = offsets[:first + 1].cpu().numpy()
        rows = children[:off[-1]].cpu().numpy()
        F.check_level(nodes[head], off, rows, order, [answers[i] for i in head])
        start = np.zeros(first + 1, dtype=np.int64)
        table = np.zeros((int(kids.sum()), 81), dtype=np.uint8)
        start[1:] = np.cumsum(kids)
        for r, i in enumerate(head):
            table[start[i]:start[i + 1]] = rows[off[r]:off[r + 1]]
        tt, tstart = _dev(solver, table), _dev(solver, start)

        def want_children(lo, hi):  # child row c is child c - offsets[p] of node p, the last p with offsets[p] <= c
            c = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            p = torch.searchsorted(want_off, c, right=True) - 1
            return tt[tstart[D.index(p)] + (c - want_off[p])]
        L.compare(children[:total], want_children, total, "children")
        assert bool((children[total:] == FILL).all()), "rows past the total were written"
        L.compare(d_nodes, lambda lo, hi: D.gather(tn, lo, hi), n, "nodes after the call")
        # cap five short of the total
        for lo, hi in L.chunks(total):
            children[lo:hi].fill_(FILL)
        _expand_raw(solver, d_nodes, tmp, offsets, children, total - 5, order)
        L.compare(offsets, lambda lo, hi: want_off[lo:hi], n + 1, "offsets, cap = total - 5")
        L.compare(children[:total - 5], want_children, total - 5, "children, cap = total - 5")
        assert bool((children[total - 5:] == FILL).all()), "rows past cap were written"
    with L.budget(12 * L.GIB):
        body()


EXPAND_LAUNCH = (0xFFFFFFFF // 256) * 4  # nodes a launch of the two node kernels holds: 2^32 - 1 threads, a wave a node


def test_expand_frontier_past_one_launch(solver):
    """2^26 + 777 nodes: a wave a node is more than 2^32 threads, which one
    launch cannot hold (the runtime would run a part of the grid without an
    error), so the node kernels go in two launches; and nodes + p * 81 passes
    2^32.  Sparse: the fillers have no child, the nodes in the windows and
    either side of the launch boundary are frontier_cases.node_set's, checked
    by frontier_cases.check_level."""
    import frontier_cases as F

    def body():
        order, dev = "gen", solver.device
        nodes, answers = F.node_set(order)
        n = (1 << 26) + 777
        assert EXPAND_LAUNCH < n and n * 81 > L.T32
        rows = np.unique(np.concatenate([L.windows(n, 81), np.arange(EXPAND_LAUNCH - L.SPAN, EXPAND_LAUNCH + L.SPAN)]))
        S = L.Sparse(n, 81, len(nodes), seed=9, rows=rows)
        assert len(np.unique(S.picks)) == len(nodes)
        tn = _dev(solver, nodes)
        d_nodes = L.build(n, lambda lo, hi: S.gather(tn, lo, hi, L.filler_boards), dev)
        L.self_check(d_nodes, S, nodes, n, 81, fillers=True)
        cap = 9 * len(rows)
        tmp = L.filled(n, 81, torch.uint8, FILL, dev)
        offsets = L.filled(n + 1, 0, torch.int64, ST_FILL, dev)
        children = L.filled(cap, 81, torch.uint8, FILL, dev)
        with _timed("expand_frontier past one launch"):
            _expand_raw(solver, d_nodes, tmp, offsets, children, cap, order)
        # offsets rise only at the real rows ...
        real = torch.zeros(n, dtype=torch.bool, device=dev)
        real[_dev(solver, rows)] = True
        for lo, hi in L.chunks(n):
            step = offsets[lo + 1:hi + 1] - offsets[lo:hi]
            assert bool(((step == 0) | real[lo:hi]).all()) and bool((step >= 0).all()), f"offsets of rows [{lo}, {hi})"
        # ... where the level is the contract's
        at = _dev(solver, rows)
        off = torch.cat([offsets[at], offsets[n:]]).cpu().numpy()
        total = int(off[-1])
        assert off[0] == 0 and 0 < total <= cap and np.array_equal(offsets[at + 1].cpu().numpy(), off[1:])
        kids = children.cpu().numpy()
        assert (kids[total:] == FILL).all()
        # every distinct node's first copy against the oracle, its other copies equal to the first
        seen, keep = {}, []
        for j, i in enumerate(S.picks):
            kid = kids[off[j]:off[j + 1]]
            if i in seen:
                assert np.array_equal(kid, seen[i]), f"node row {rows[j]}: not the children of its first copy"
            else:
                seen[i] = kid
                keep.append(i)
        F.check_level(nodes[keep], np.concatenate([[0], np.cumsum([len(seen[i]) for i in keep])]),
                      np.concatenate([seen[i] for i in keep]), order, [answers[i] for i in keep])
        L.compare(d_nodes, lambda lo, hi: S.gather(tn, lo, hi, L.filler_boards), n, "nodes after the call")
    with L.budget(12 * L.GIB):
        body()


# -------------------------------------------------------------- completions
def test_completions(solver):
    """sdk_enumerate_batch on 61 copies of H1 (885 469 completions each): one
    list of 54 013 609 rows, grids + slot * 81 past 2^32.  Every board's count
    is H1_COUNT and every owner has that many rows; board 0's rows are checked
    on the host as test_gpu_enum checks them; every other board's rows, sorted
    on the device, are board 0's sorted rows."""
    import ctypes
    import enum_cases as N
    from sudoku_solver_distributed_amd.solver import EXACT_MAX_ROUNDS, EXACT_SLICE
    from test_gpu_enum import _check_h1_rows

    def body():
        h1, each = N.load_fixture()["h1"]
        copies, dev = 61, solver.device
        rows = copies * each
        assert each == N.H1_COUNT and rows == 54_013_609 and rows * 81 > L.T32
        boards = _dev(solver, np.tile(h1, (copies, 1)))
        grids, owner = L.filled(rows + 8, 81, torch.uint8, FILL, dev), L.filled(rows + 8, 0, torch.int32, ST_FILL, dev)
        count = L.filled(copies, 0, torch.int64, ST_FILL, dev)
        status = L.filled(copies, 0, torch.int32, ST_FILL, dev)
        need = solver.lib.sdk_enumerate_scratch_bytes(copies, 0, 0)
        scratch = _scratch(solver, need)
        info = (ctypes.c_int64 * 6)()
        with _timed("completions"), torch.cuda.device(dev):
            assert solver.lib.sdk_enumerate_batch(boards.data_ptr(), copies, grids.data_ptr(), owner.data_ptr(), rows,
                                                  0, count.data_ptr(), status.data_ptr(), EXACT_SLICE, EXACT_MAX_ROUNDS,
                                                  0, scratch.data_ptr(), need, 0, _stream_handle(solver), info) == 0
        del scratch
        print(dict(zip(N.INFO, info)))
        assert info[4] == info[5] == rows
        assert count.tolist() == [each] * copies and status.tolist() == [N.DONE] * copies
        assert bool((grids[rows:] == FILL).all()) and bool((owner[rows:] == ST_FILL).all()), "rows past the list"
        assert torch.equal(boards, _dev(solver, np.tile(h1, (copies, 1))))
        assert L.histogram(owner[:rows], rows, lowest=0) == {k: each for k in range(copies)}
        # 81 digits of 4 bits in six int64 keys of 15 digits (no byte above 9, so equal keys are equal rows)
        shifts = torch.arange(14, -1, -1, device=dev, dtype=torch.int64) * 4
        keys = torch.empty((6, rows), dtype=torch.int64, device=dev)
        for lo, hi in L.chunks(rows):
            g = grids[lo:hi]
            assert int(g.max()) <= 9 and int(g.min()) >= 1
            for k in range(6):
                part = g[:, 15 * k:15 * k + 15].to(torch.int64)
                keys[k, lo:hi] = (part << shifts[:part.shape[1]]).sum(dim=1)
        order = torch.arange(rows, device=dev)
        for k in range(5, -1, -1):  # stable sorts, the last key first, the owner last of all
            order = order[torch.sort(keys[k][order], stable=True)[1]]
        order = order[torch.sort(owner[:rows][order], stable=True)[1]]
        for k in range(6):
            by_board = keys[k][order].view(copies, each)
            assert bool((by_board == by_board[0]).all()), f"key {k}: a board's sorted rows are not board 0's"
        assert bool((owner[:rows][order[:each]] == 0).all())
        _check_h1_rows(grids.index_select(0, order[:each]).cpu().numpy(), h1)
    with L.budget(12 * L.GIB):
        body()
