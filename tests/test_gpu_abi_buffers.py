"""What include/sudoku_hip.h promises about caller memory, through the raw C
ABI (runs on an MI355X): solving in place, byte arrays at any address, no
byte written outside the documented extents, scratch and workspace of exactly
the stated size with arbitrary contents, every launch and memset on the
caller's stream, and the deferred list past its capacity.

Arguments are carved from guarded arenas (abi_arena.Arena: 0xA5 around
outputs, 0xFF -- a byte > 9 -- around inputs).  Expectations are the oracle
pool's (abi_arena.pool) or the entry's own reference: count_cases.expected,
tests/golden/canon_cases.json with gen.apply_symmetry, O.check / check_sums,
O.first_candidate, O.peer_solve / PeerNode, frontier_cases.check_level.
Two comparisons are GPU against GPU, on top of those: canon's automorphism
count and the peer node's state record against the wrapper's run on
allocator-aligned tensors (the fixture has no counts; the record's layout is
the library's own).  Ordered mode past the deferred list's capacity is not
covered.

Sections c and d here cover solve, check, first_candidate, peer_solve,
expand_frontier, count_solutions and canonical.  The same two checks of the
seven analysis entries -- rate, candidates, unique_candidates, minimize,
sample, count_exact and enumerate -- are in test_gpu_abi_streams.py, on the
harness both files share (abi_arena: _stream_handle, _poisons, _delay_rate,
_on_side_stream)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_arena as A
import count_cases as C
import frontier_cases as F
from abi_arena import (IN_FILL, OUT_FILL, ORDERS, Arena, _delay_rate, _on_side_stream, _poisons,  # noqa: F401
                       _stream_handle)
from conftest import load_golden
from oracle import oracle as O

pytestmark = pytest.mark.gpu

OFFSETS = [(0, 0), (1, 2), (2, 3), (3, 1)]  # input / output byte offsets (mod 4)
SLACK = 1 << 16  # arena bytes beyond the carved ones (guards, alignment)
# ... and behind a count scratch, the last region of its arena: more than one wave's stack lines (about 660 KB),
# so that a grid one wave larger than the scratch covers shows in the guards and stays inside the arena
COUNT_MARGIN = 1 << 20


# ------------------------------------------------------------------ helpers
def _kernel(solver, name):
    """Force a solve kernel; returns the selection to restore."""
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS[name])
    assert prev > 0
    return prev


def _put(view, array):
    view.copy_(torch.from_numpy(np.array(array)).to(view.device).view(view.dtype).reshape(view.shape))


def _solve_raw(solver, p, out, st, order, ordered=0, grid_waves=0, ws=None, stream=None):
    ws = solver.workspace if ws is None else ws
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_solve_batch_grid(p.data_ptr(), out.data_ptr(), st.data_ptr(), p.shape[0], ws.data_ptr(),
                                             ORDERS[order], ordered, _stream_handle(solver, stream), grid_waves)
    assert rc == 0, solver.lib.sdk_last_error()


def _solve_batches_raw(solver, ps, outs, sts, order, grid_waves=0, stream=None):
    k = len(ps)
    arr = ctypes.c_void_p * k
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_solve_batches(arr(*[p.data_ptr() for p in ps]), arr(*[o.data_ptr() for o in outs]),
                                          arr(*[s.data_ptr() for s in sts]),
                                          (ctypes.c_int64 * k)(*[p.shape[0] for p in ps]), k,
                                          solver.workspace.data_ptr(), ORDERS[order], _stream_handle(solver, stream),
                                          grid_waves)
    assert rc == 0, solver.lib.sdk_last_error()


def _pool_want(order, idx):
    rows, st = A.pool()["want"][order]
    return rows[idx], st[idx]


def _assert_solved(rows, st, order, idx, what):
    wr, ws = _pool_want(order, idx)
    rows, st = rows.cpu().numpy(), st.cpu().numpy()
    bad = np.nonzero((st != ws) | (rows != wr).any(axis=1))[0]
    assert len(bad) == 0, (what, [(int(i), int(idx[i]), int(st[i]), int(ws[i])) for i in bad[:8]])


def _carve_solve(ain, aout, n, oi, oo, tag=""):
    return (ain.boards(n, oi, name="puzzles" + tag), aout.boards(n, oo, name="solutions" + tag),
            aout.carve(4 * n, itemsize=4, name="status" + tag))


# ------------------------------------------------------- a. in-place solve
IN_PLACE = [("packed", 257, 0), ("packed", 20_011, 0), ("plane", 2049, 0), ("plane", 200_001, 1)]


@pytest.mark.parametrize("order", ["gen", "node"])
@pytest.mark.parametrize("kernel,n,grid_waves", IN_PLACE, ids=[f"{k}-{n}" for k, n, _ in IN_PLACE])
def test_in_place_solve(solver, kernel, n, grid_waves, order):
    """d_solutions == d_puzzles at an odd address, every pool kind
    interleaved: packed within the static hand-out and past it (queue), plane
    in one claim per lane and, at one wave per SIMD, with every lane claiming
    again.  Catches an output store that reaches a neighbour's bytes before
    that board's owner has read them (a whole-dword edge store), and a board
    re-read after its row was written."""
    idx = A.mixed(n, seed=ORDERS[order])
    boards = A.pool()["boards"][idx]
    ain, ast = Arena(solver.device, IN_FILL, 81 * n + SLACK), Arena(solver.device, OUT_FILL, 4 * n + SLACK)
    io = ain.boards(n, 1 + ORDERS[order], name="boards")
    st = ast.carve(4 * n, itemsize=4, name="status")
    _put(io, boards)
    prev = _kernel(solver, kernel)
    try:
        solver.stats(reset=True)
        _solve_raw(solver, io, io, st, order, grid_waves=grid_waves)
        torch.cuda.synchronize()
        stats = solver.stats()
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    _assert_solved(io, st, order, idx, (kernel, n))
    assert stats["finished"] == n
    ain.assert_guards()
    ast.assert_guards()


@pytest.mark.parametrize("kernel,n", [("packed", 257), ("plane", 2049)])
def test_in_place_solve_ordered(solver, kernel, n):
    """Ordered mode in place, test_ordered_cancelled_rows_keep_input's rule:
    best is the lowest solved index, rows below it are the pool's (none is
    solved), rows above it are answered as the pool says or cancelled and
    untouched, every board is counted."""
    P = A.pool()
    rest = A.mixed(n - 40, seed=3)
    for order in ("gen", "node"):
        unsolved = np.nonzero(P["want"][order][1] != 1)[0]
        idx = np.concatenate([np.random.default_rng(4).choice(unsolved, 40), rest])
        boards = P["boards"][idx]
        wr, ws = _pool_want(order, idx)
        best = int(np.nonzero(ws == 1)[0][0])
        assert best >= 40
        ain, ast = Arena(solver.device, IN_FILL, 81 * n + SLACK), Arena(solver.device, OUT_FILL, 4 * n + SLACK)
        io, st = ain.boards(n, 3, name="boards"), ast.carve(4 * n, itemsize=4, name="status")
        _put(io, boards)
        prev = _kernel(solver, kernel)
        try:
            solver.stats(reset=True)
            _solve_raw(solver, io, io, st, order, ordered=1)
            torch.cuda.synchronize()
            stats = solver.stats()
        finally:
            solver.lib.sdk_set_solve_kernel(prev)
        rows, got = io.cpu().numpy(), st.cpu().numpy()
        assert np.array_equal(got[:best + 1], ws[:best + 1]) and np.array_equal(rows[:best + 1], wr[:best + 1])
        cancelled = got == -2
        assert not cancelled[:best + 1].any()
        assert np.array_equal(got[~cancelled], ws[~cancelled]) and np.array_equal(rows[~cancelled], wr[~cancelled])
        assert np.array_equal(rows[cancelled], boards[cancelled])
        print(f"{kernel} {order}: best {best}, {int(cancelled.sum())} of {n} cancelled")
        assert stats["best"] == best and stats["finished"] == n
        ain.assert_guards()
        ast.assert_guards()


BATCHES = (1, 2049, 6200)


@pytest.mark.parametrize("order", ["gen", "node"])
@pytest.mark.parametrize("kernel", ["plane", "packed"])
def test_in_place_solve_batches(solver, kernel, order):
    """sdk_solve_batches with every batch in place, three batches at
    different odd addresses of one arena (plane: one queue over all three)."""
    total = sum(BATCHES)
    ain, ast = Arena(solver.device, IN_FILL, 81 * total + SLACK), Arena(solver.device, OUT_FILL, 4 * total + SLACK)
    idxs = [A.mixed(n, seed=10 + k) for k, n in enumerate(BATCHES)]
    ios = [ain.boards(n, (1, 3, 2)[k], name=f"batch{k}") for k, n in enumerate(BATCHES)]
    sts = [ast.carve(4 * n, itemsize=4, name=f"status{k}") for k, n in enumerate(BATCHES)]
    for io, idx in zip(ios, idxs):
        _put(io, A.pool()["boards"][idx])
    prev = _kernel(solver, kernel)
    try:
        solver.stats(reset=True)
        _solve_batches_raw(solver, ios, ios, sts, order, grid_waves=1)
        torch.cuda.synchronize()
        stats = solver.stats()
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    for k, (io, st, idx) in enumerate(zip(ios, sts, idxs)):
        _assert_solved(io, st, order, idx, (kernel, k))
    assert stats["finished"] == total
    ain.assert_guards()
    ast.assert_guards()


# ------------------------------- b. odd addresses and guards, every entry
@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_solve(solver, oi, oo):
    for kernel, n in (("packed", 65), ("plane", 2049), ("auto", 8192 + 63)):
        for order in ("gen", "node"):
            idx = A.mixed(n, seed=20 + oi)
            boards = A.pool()["boards"][idx]
            ain, aout = Arena(solver.device, IN_FILL, 81 * n + SLACK), Arena(solver.device, OUT_FILL, 85 * n + SLACK)
            p, out, st = _carve_solve(ain, aout, n, oi, oo)
            _put(p, boards)
            prev = _kernel(solver, kernel)
            try:
                _solve_raw(solver, p, out, st, order)
                torch.cuda.synchronize()
            finally:
                solver.lib.sdk_set_solve_kernel(prev)
            _assert_solved(out, st, order, idx, (kernel, n, order))
            aout.assert_guards()
            ain.assert_guards()
            assert np.array_equal(p.cpu().numpy(), boards)


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_solve_batches(solver, oi, oo):
    total = sum(BATCHES)
    for order in ("gen", "node"):
        ain = Arena(solver.device, IN_FILL, 81 * total + SLACK)
        aout = Arena(solver.device, OUT_FILL, 85 * total + SLACK)
        idxs = [A.mixed(n, seed=30 + k) for k, n in enumerate(BATCHES)]
        trip = [_carve_solve(ain, aout, n, (oi + k) % 4, (oo + 3 * k) % 4, str(k)) for k, n in enumerate(BATCHES)]
        for (p, _, _), idx in zip(trip, idxs):
            _put(p, A.pool()["boards"][idx])
        _solve_batches_raw(solver, [t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip], order)
        torch.cuda.synchronize()
        for k, ((p, out, st), idx) in enumerate(zip(trip, idxs)):
            _assert_solved(out, st, order, idx, (order, k))
            assert np.array_equal(p.cpu().numpy(), A.pool()["boards"][idx])
        aout.assert_guards()
        ain.assert_guards()


@functools.lru_cache(maxsize=None)
def _check_cases():
    from test_gpu_frontier import _edge_grids
    golden = np.array([F.b81(c["grid"]) for c in load_golden("golden_check.json")], dtype=np.uint8)
    grids = np.concatenate([golden, _edge_grids()])
    want = {0: np.array([int(O.check(g)) for g in grids], dtype=np.int32),
            1: np.array([int(O.check_sums(g)) for g in grids], dtype=np.int32)}
    return grids, want


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_check(solver, oi, oo):
    from test_gpu_frontier import _sized
    grids, want = _check_cases()
    n = 129
    for mode in (0, 1):
        idx = _sized(grids, want[mode], n)
        ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
        g, ok = ain.boards(n, oi, name="grids"), aout.carve(4 * n, itemsize=4, name="ok")
        _put(g, grids[idx])
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_check_batch(g.data_ptr(), ok.data_ptr(), n, mode, _stream_handle(solver)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy(), want[mode][idx]), mode
        aout.assert_guards()
        ain.assert_guards()
        assert np.array_equal(g.cpu().numpy(), grids[idx])


@functools.lru_cache(maxsize=None)
def _candidate_cases():
    cases = load_golden("golden_node.json")["first_candidate"]
    grids = np.array([F.b81(c["grid"]) for c in cases], dtype=np.uint8)
    cells = np.array([c["row"] * 9 + c["col"] for c in cases], dtype=np.int32)
    want = np.array([O.first_candidate(g, int(c) // 9, int(c) % 9) or 0 for g, c in zip(grids, cells)], dtype=np.int32)
    return grids, cells, want


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_first_candidate(solver, oi, oo):
    from test_gpu_frontier import _sized
    grids, cells, want = _candidate_cases()
    n = 257
    idx = _sized(grids, want, n)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    g, c = ain.boards(n, oi, name="grids"), ain.carve(4 * n, itemsize=4, name="cells")
    num = aout.carve(4 * n, itemsize=4, name="num")
    _put(g, grids[idx])
    _put(c, cells[idx])
    with torch.cuda.device(solver.device):
        assert solver.lib.sdk_first_candidate_batch(g.data_ptr(), c.data_ptr(), num.data_ptr(), n,
                                                    _stream_handle(solver)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(num.cpu().numpy(), want[idx])
    aout.assert_guards()
    ain.assert_guards()
    assert np.array_equal(g.cpu().numpy(), grids[idx]) and np.array_equal(c.cpu().numpy(), cells[idx])


PEER_CODE = {1: 1, 0: 0, -1: -4}  # oracle -> SDK_SOLVED / SDK_UNSOLVABLE / SDK_NO_RETURN


@functools.lru_cache(maxsize=None)
def _peer_cases():
    """65 boards of test_peer_solve's kind and the oracle's (row, status,
    validations) for each on a fresh node."""
    from test_peer_solve import _boards
    boards = np.ascontiguousarray(_boards(65, 31)[:65])
    res = [O.peer_solve(b) for b in boards]
    return (boards, np.array([r[1] for r in res], dtype=np.uint8),
            np.array([PEER_CODE[r[0]] for r in res], dtype=np.int32), np.array([r[2] for r in res], dtype=np.int32))


def _carve_peer(ain, aout, n, oi, oo):
    return (ain.boards(n, oi, name="boards"), aout.boards(n, oo, name="out"),
            aout.carve(4 * n, itemsize=4, name="status"), aout.carve(4 * n, itemsize=4, name="validations"))


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_peer_solve(solver, oi, oo):
    boards, rows, status, vals = _peer_cases()
    n = len(boards)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    b, out, st, val = _carve_peer(ain, aout, n, oi, oo)
    _put(b, boards)
    with torch.cuda.device(solver.device):
        assert solver.lib.sdk_peer_solve_batch(b.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                               _stream_handle(solver)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), status) and np.array_equal(val.cpu().numpy(), vals)
    assert np.array_equal(out.cpu().numpy(), rows)
    aout.assert_guards()
    ain.assert_guards()
    assert np.array_equal(b.cpu().numpy(), boards)


@functools.lru_cache(maxsize=None)
def _peer_seq_cases():
    """A five-request sequence on one node: (boards, rows, status,
    validations) from the oracle's PeerNode."""
    from test_peer_solve import _random_sequences
    boards = np.ascontiguousarray(_random_sequences(1, 5, 32)[0])
    node = O.PeerNode()
    res = [node.solve(b) for b in boards]
    return (boards, np.array([r[1] for r in res], dtype=np.uint8),
            np.array([PEER_CODE[r[0]] for r in res], dtype=np.int32), np.array([r[2] for r in res], dtype=np.int32))


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_peer_solve_seq(solver, oi, oo):
    from sudoku_solver_distributed_amd._lib import SDK_PEER_STATE_BYTES
    boards, rows, status, vals = _peer_seq_cases()
    n = len(boards)
    plain = solver.new_peer_state()
    solver.peer_solve_seq(torch.from_numpy(boards), plain)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    b, out, st, val = _carve_peer(ain, aout, n, oi, oo)
    state = aout.carve(SDK_PEER_STATE_BYTES, align=16, name="node state")
    state.zero_()
    _put(b, boards)
    with torch.cuda.device(solver.device):
        assert solver.lib.sdk_peer_solve_seq(b.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                             state.data_ptr(), _stream_handle(solver)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), status) and np.array_equal(val.cpu().numpy(), vals)
    assert np.array_equal(out.cpu().numpy(), rows)
    assert torch.equal(state, plain)
    aout.assert_guards()
    ain.assert_guards()
    assert np.array_equal(b.cpu().numpy(), boards)


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_expand(solver, oi, oo):
    n = 65
    for order in ("gen", "node"):
        nodes, answers = F.node_set(order)
        last = len(nodes) - 8  # every second node of the set and its last eight (the single boards)
        pick = np.concatenate([np.arange(0, last, len(nodes) // (n - 8))[:n - 8], np.arange(last, len(nodes))])
        assert len(pick) == n
        nd, ans = np.ascontiguousarray(nodes[pick]), [answers[i] for i in pick]
        cap = 9 * n
        ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
        d_nodes = ain.boards(n, oi, name="nodes")
        tmp = aout.boards(n, (oo + 1) % 4, name="tmp")
        offsets = aout.carve(8 * (n + 1), itemsize=8, name="offsets")
        children = aout.boards(cap, oo, name="children")
        _put(d_nodes, nd)
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_expand_frontier(d_nodes.data_ptr(), n, tmp.data_ptr(), offsets.data_ptr(),
                                                  children.data_ptr(), cap, ORDERS[order], _stream_handle(solver)) == 0
        torch.cuda.synchronize()
        off, ch = offsets.cpu().numpy(), children.cpu().numpy()
        total = int(off[-1])
        assert 0 < total <= cap and (ch[total:] == OUT_FILL).all()
        F.check_level(nd, off, ch[:total], order, ans)
        aout.assert_guards()
        ain.assert_guards()
        assert np.array_equal(d_nodes.cpu().numpy(), nd)


def _count_raw(solver, boards, first, count, scratch, max_waves, limit=2, stream=None):
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_count_solutions_batch(boards.data_ptr(), count.data_ptr(), first.data_ptr(),
                                                  boards.shape[0], limit, scratch.data_ptr(), scratch.numel(),
                                                  max_waves, _stream_handle(solver, stream))
    assert rc == 0


def _count_indices(n):
    from test_gpu_count import _mixed
    return _mixed(n)[1]


def _check_counts(boards, idx, count, first, limit=2):
    _, _, uniq, is_unique, _ = C.pool()
    cnt = count.cpu().numpy()
    want = C.expected(limit)[idx]
    bad = np.nonzero(cnt != want)[0]
    assert len(bad) == 0, [(int(i), int(idx[i]), int(cnt[i]), int(want[i])) for i in bad[:10]]
    C.check_first(boards, cnt, first.cpu().numpy(), uniq[idx], is_unique[idx])


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_count(solver, oi, oo):
    """count_load_words reads the 21 aligned dwords around a board: the 0xFF
    bytes they hold beside the batch must not reach a count."""
    for n, max_waves in ((65, 0), (4097, 2)):
        idx = _count_indices(n)
        boards = C.pool()[0][idx]
        need = int(solver.lib.sdk_count_scratch_bytes(n, max_waves))
        ain = Arena(solver.device, IN_FILL, 81 * n + SLACK)
        aout = Arena(solver.device, OUT_FILL, 85 * n + need + SLACK + COUNT_MARGIN)
        p = ain.boards(n, oi, name="puzzles")
        first, count = aout.boards(n, oo, name="first"), aout.carve(4 * n, itemsize=4, name="count")
        scratch = aout.carve(need, align=256, name="scratch")
        _put(p, boards)
        _count_raw(solver, p, first, count, scratch, max_waves)
        torch.cuda.synchronize()
        _check_counts(boards, idx, count, first)
        aout.assert_guards()
        ain.assert_guards()
        assert np.array_equal(p.cpu().numpy(), boards)


@functools.lru_cache(maxsize=None)
def _canon_cases(n=65):
    """n boards of tests/golden/canon_cases.json (cyclically, with a byte-10
    board in between) and the fixture's canonical forms."""
    doc = load_golden("canon_cases.json")["cases"]
    idx = np.arange(n) % len(doc)
    boards = np.stack([F.b81(doc[i]["board"]) for i in idx])
    canon = np.stack([F.b81(doc[i]["canon"]) for i in idx])
    boards[50, 80] = 10
    canon[50] = boards[50]
    names = [doc[i]["name"] for i in idx]
    return boards, canon, names


def _canon_raw(solver, boards, canon, sym, autos, scratch, slices, stream=None):
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_canonical_batch(boards.data_ptr(), canon.data_ptr(), sym.data_ptr(), autos.data_ptr(),
                                            boards.shape[0], slices, scratch.data_ptr(), scratch.numel(),
                                            _stream_handle(solver, stream))
    assert rc == 0


def _check_canon(solver, boards, want, names, canon, sym, autos):
    from sudoku_solver_distributed_amd import gen
    canon, sym, autos = canon.cpu().numpy(), sym.cpu().numpy(), autos.cpu().numpy()
    assert np.array_equal(canon, want)
    good = boards.max(axis=1) <= 9
    assert (sym[~good] == -1).all() and (autos[~good] == -1).all() and (~good).sum() == 1
    assert np.array_equal(gen.apply_symmetry(boards[good], sym[good])[0], want[good])
    assert int(autos[names.index("empty")]) == 3359232 and int(autos[names.index("one_clue")]) == 41472
    plain = solver.canonical(torch.from_numpy(boards), return_sym=True, return_autos=True, slices=1)
    assert np.array_equal(sym, plain[1].cpu().numpy()) and np.array_equal(autos, plain[2].cpu().numpy())


@pytest.mark.parametrize("oi,oo", OFFSETS)
def test_guards_canonical(solver, oi, oo):
    boards, want, names = _canon_cases()
    n = len(boards)
    for slices in (0, 7):
        need = int(solver.lib.sdk_canonical_scratch_bytes(n, slices))
        ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL, 85 * n + need + SLACK)
        b = ain.boards(n, oi, name="boards")
        canon, sym = aout.boards(n, oo, name="canon"), aout.carve(4 * n, itemsize=4, name="sym")
        autos = aout.carve(4 * n, itemsize=4, name="autos")
        scratch = aout.carve(need, align=256, name="scratch")
        _put(b, boards)
        _canon_raw(solver, b, canon, sym, autos, scratch, slices)
        torch.cuda.synchronize()
        _check_canon(solver, boards, want, names, canon, sym, autos)
        aout.assert_guards()
        ain.assert_guards()
        assert np.array_equal(b.cpu().numpy(), boards)


def test_guards_snapshot_stats(solver):
    solver.stats(reset=True)
    idx = A.mixed(2049, seed=40)
    prev = _kernel(solver, "plane")
    try:
        solver.solve(torch.from_numpy(A.pool()["boards"][idx]))
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    aout = Arena(solver.device, OUT_FILL)
    out = aout.carve(48, itemsize=8, name="d_out")
    with torch.cuda.device(solver.device):
        assert solver.lib.sdk_snapshot_stats(solver.workspace.data_ptr(), out.data_ptr(), _stream_handle(solver)) == 0
    torch.cuda.synchronize()
    s = solver.stats()
    assert out.tolist() == [s[k] for k in ("finished", "solved", "guesses", "sweeps", "best", "deferred")]
    assert s["finished"] == 2049 and s["solved"] == int((_pool_want("gen", idx)[1] == 1).sum()) and s["deferred"] > 0
    aout.assert_guards()


# --------------------- c. exact-size, poisoned scratch and workspace
@pytest.mark.parametrize("n,max_waves", [(65, 0), (4097, 2), (4097, 0)])
def test_exact_count_scratch(solver, n, max_waves):
    """Exactly sdk_count_scratch_bytes(n, max_waves) bytes inside guards,
    whatever they hold: a grid one wave larger than the scratch covers, or a
    stack line read before it is written, shows in the guards or the counts."""
    idx = _count_indices(n)
    boards = C.pool()[0][idx]
    need = int(solver.lib.sdk_count_scratch_bytes(n, max_waves))
    assert need > 256
    ain = Arena(solver.device, IN_FILL, 81 * n + SLACK)
    aout = Arena(solver.device, OUT_FILL, 85 * n + need + SLACK + COUNT_MARGIN)
    p = ain.boards(n, 1, name="puzzles")
    first, count = aout.boards(n, 3, name="first"), aout.carve(4 * n, itemsize=4, name="count")
    scratch = aout.carve(need, align=256, name="scratch")
    _put(p, boards)
    for what, fill in _poisons(scratch):
        fill()
        first.fill_(OUT_FILL)
        count.fill_(-1515870811)
        _count_raw(solver, p, first, count, scratch, max_waves)
        torch.cuda.synchronize()
        _check_counts(boards, idx, count, first)
        aout.assert_guards()
        ain.assert_guards()


@pytest.mark.parametrize("n,slices", [(65, 7), (65, 0), (1, 2592)])
def test_exact_canon_scratch(solver, n, slices):
    boards, want, names = _canon_cases()
    need = int(solver.lib.sdk_canonical_scratch_bytes(n, slices))
    assert need > 0 and (slices == 0 or need == 64 * n * slices)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL, 85 * n + need + SLACK)
    b = ain.boards(n, 2, name="boards")
    canon, sym = aout.boards(n, 1, name="canon"), aout.carve(4 * n, itemsize=4, name="sym")
    autos = aout.carve(4 * n, itemsize=4, name="autos")
    scratch = aout.carve(need, align=256, name="scratch")
    pick = slice(0, 65) if n == 65 else slice(names.index("puzzle_30"), names.index("puzzle_30") + 1)
    _put(b, boards[pick])
    for what, fill in _poisons(scratch):
        fill()
        _canon_raw(solver, b, canon, sym, autos, scratch, slices)
        torch.cuda.synchronize()
        if n == 65:
            _check_canon(solver, boards, want, names, canon, sym, autos)
        else:
            from sudoku_solver_distributed_amd import gen
            assert np.array_equal(canon.cpu().numpy(), want[pick]), what
            assert np.array_equal(gen.apply_symmetry(boards[pick], sym.cpu().numpy())[0], want[pick]), what
            assert int(autos[0]) >= 1
        aout.assert_guards()
        ain.assert_guards()


def test_exact_workspace(solver):
    """A workspace of exactly sdk_workspace_bytes() bytes inside guards,
    zeroed once: the plane kernel at one wave per SIMD with the widest tail
    through the XCD pool (the pool is the workspace's last bytes), then a
    batch of clashing boards (the deferred list, just before the pool)."""
    lib = solver.lib
    need = int(lib.sdk_workspace_bytes())
    aws = Arena(solver.device, OUT_FILL, need + SLACK)
    ws = aws.carve(need, align=256, name="workspace")
    ws.zero_()
    n, m = 70_001, 4097
    idx = A.mixed(n, seed=50, kinds=("hard17", "gen", "dead", "invalid", "single"))
    cidx = A.mixed(m, seed=51, kinds=("clash",))
    ain = Arena(solver.device, IN_FILL, 81 * (n + m) + SLACK)
    aout = Arena(solver.device, OUT_FILL, 85 * (n + m) + SLACK)
    p, out, st = _carve_solve(ain, aout, n, 1, 2)
    cp, cout, cst = _carve_solve(ain, aout, m, 2, 3, " (clash)")
    _put(p, A.pool()["boards"][idx])
    _put(cp, A.pool()["boards"][cidx])
    prev = _kernel(solver, "plane")
    stats, verdict = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 4)()
    try:
        assert lib.sdk_set_plane_tuning(-1, 40, 2, -1) == 0
        _solve_raw(solver, p, out, st, "gen", grid_waves=1, ws=ws)
        _solve_raw(solver, cp, cout, cst, "node", ws=ws)
        with torch.cuda.device(solver.device):
            assert lib.sdk_read_stats(ws.data_ptr(), stats, 0, _stream_handle(solver)) == 0
            assert lib.sdk_verify_workspace(ws.data_ptr(), verdict, _stream_handle(solver)) == 0, lib.sdk_last_error()
        torch.cuda.synchronize()
    finally:
        lib.sdk_set_plane_tuning(-1, -1, -1, -1)
        lib.sdk_set_solve_kernel(prev)
    _assert_solved(out, st, "gen", idx, "plane")
    _assert_solved(cout, cst, "node", cidx, "clash")
    assert stats[0] == n + m and stats[5] >= m
    assert list(verdict) == [n + m, n + m, 0, 0]
    aws.assert_guards()
    aout.assert_guards()
    ain.assert_guards()
    del ws, aws
    torch.cuda.empty_cache()


# ----------------------------------------------------------- d. stream order
def _dev(solver, array):
    return torch.from_numpy(np.array(array)).to(solver.device)


@pytest.mark.parametrize("kernel,n,grid_waves", [("packed", 257, 0), ("packed", 20_011, 0), ("plane", 70_001, 1)])
def test_stream_solve(solver, kernel, n, grid_waves):
    """Packed within the static hand-out (no re-arm launch) and past it,
    plane with more boards than lanes: the queue head's re-arm is a launch
    of its own."""
    idx = A.mixed(n, seed=60)
    real = _dev(solver, A.pool()["boards"][idx])
    ain, aout = Arena(solver.device, IN_FILL, 81 * n + SLACK), Arena(solver.device, OUT_FILL, 170 * n + SLACK)
    p, out, st = _carve_solve(ain, aout, n, 1, 2)
    out2, st2 = aout.boards(n, 3, name="solutions (dirty)"), aout.carve(4 * n, itemsize=4, name="status (dirty)")
    prev = _kernel(solver, kernel)
    try:
        rows, status = _on_side_stream(
            solver, f"solve {kernel} {n}", [(p, real)],
            lambda s: _solve_raw(solver, p, out, st, "gen", grid_waves=grid_waves, stream=s), [out, st],
            dirty=lambda s: _solve_raw(solver, p, out2, st2, "gen", grid_waves=grid_waves, stream=s))
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    _assert_solved(rows, status, "gen", idx, kernel)
    aout.assert_guards()


def test_stream_solve_batches(solver):
    total = sum(BATCHES)
    ain, aout = Arena(solver.device, IN_FILL, 81 * total + SLACK), Arena(solver.device, OUT_FILL, 170 * total + SLACK)
    idxs = [A.mixed(n, seed=61 + k) for k, n in enumerate(BATCHES)]
    trip = [_carve_solve(ain, aout, n, k + 1, (k + 2) % 4, str(k)) for k, n in enumerate(BATCHES)]
    ps, outs, sts = ([t[i] for t in trip] for i in range(3))
    outs2 = [aout.boards(n, 0, name=f"solutions{k} (dirty)") for k, n in enumerate(BATCHES)]
    sts2 = [aout.carve(4 * n, itemsize=4, name=f"status{k} (dirty)") for k, n in enumerate(BATCHES)]
    got = _on_side_stream(solver, "solve_batches", [(p, _dev(solver, A.pool()["boards"][i])) for p, i in zip(ps, idxs)],
                          lambda s: _solve_batches_raw(solver, ps, outs, sts, "node", grid_waves=1, stream=s),
                          outs + sts,
                          dirty=lambda s: _solve_batches_raw(solver, ps, outs2, sts2, "node", grid_waves=1, stream=s))
    for k, idx in enumerate(idxs):
        _assert_solved(got[k], got[3 + k], "node", idx, k)
    aout.assert_guards()


def test_stream_snapshot(solver):
    """Two snapshots around a solve, all on the side stream: their
    difference is that solve's own work."""
    n = 2049
    idx = A.mixed(n, seed=62)
    real = _dev(solver, A.pool()["boards"][idx])
    ain, aout = Arena(solver.device, IN_FILL, 81 * n + SLACK), Arena(solver.device, OUT_FILL, 85 * n + SLACK)
    p, out, st = _carve_solve(ain, aout, n, 3, 1)
    before, after = aout.carve(48, itemsize=8, name="before"), aout.carve(48, itemsize=8, name="after")
    ws = solver.workspace.data_ptr()

    def call(s):
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_snapshot_stats(ws, before.data_ptr(), _stream_handle(solver, s)) == 0
        _solve_raw(solver, p, out, st, "gen", stream=s)
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_snapshot_stats(ws, after.data_ptr(), _stream_handle(solver, s)) == 0
    prev = _kernel(solver, "plane")
    try:
        rows, status, b, a = _on_side_stream(solver, "snapshot", [(p, real)], call, [out, st, before, after])
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    _assert_solved(rows, status, "gen", idx, "snapshot")
    d = (a - b).tolist()
    assert d[0] == n and d[1] == int((_pool_want("gen", idx)[1] == 1).sum()) and d[5] > 0
    aout.assert_guards()


def test_stream_count(solver):
    n, max_waves = 4097, 2
    idx = _count_indices(n)
    boards = C.pool()[0][idx]
    need = int(solver.lib.sdk_count_scratch_bytes(n, max_waves))
    ain = Arena(solver.device, IN_FILL, 81 * n + SLACK)
    aout = Arena(solver.device, OUT_FILL, 170 * n + need + SLACK + COUNT_MARGIN)
    p = ain.boards(n, 1, name="puzzles")
    first, count = aout.boards(n, 3, name="first"), aout.carve(4 * n, itemsize=4, name="count")
    first2, count2 = aout.boards(n, 2, name="first (dirty)"), aout.carve(4 * n, itemsize=4, name="count (dirty)")
    scratch = aout.carve(need, align=256, name="scratch")
    f, c = _on_side_stream(solver, "count", [(p, _dev(solver, boards))],
                           lambda s: _count_raw(solver, p, first, count, scratch, max_waves, stream=s), [first, count],
                           dirty=lambda s: _count_raw(solver, p, first2, count2, scratch, max_waves, stream=s))
    _check_counts(boards, idx, c, f)
    aout.assert_guards()


def test_stream_canonical(solver):
    boards, want, names = _canon_cases()
    n, slices = len(boards), 7
    need = int(solver.lib.sdk_canonical_scratch_bytes(n, slices))
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL, 85 * n + need + SLACK)
    b = ain.boards(n, 3, name="boards")
    canon, sym = aout.boards(n, 2, name="canon"), aout.carve(4 * n, itemsize=4, name="sym")
    autos = aout.carve(4 * n, itemsize=4, name="autos")
    scratch = aout.carve(need, align=256, name="scratch")
    got = _on_side_stream(solver, "canonical", [(b, _dev(solver, boards))],
                          lambda s: _canon_raw(solver, b, canon, sym, autos, scratch, slices, stream=s),
                          [canon, sym, autos], scratch=[scratch])
    _check_canon(solver, boards, want, names, *got)
    aout.assert_guards()


def test_stream_check_and_first_candidate(solver):
    from test_gpu_frontier import _sized
    grids, want = _check_cases()
    n = 129
    for mode in (0, 1):
        idx = _sized(grids, want[mode], n)
        ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
        g, ok = ain.boards(n, 1, name="grids"), aout.carve(4 * n, itemsize=4, name="ok")

        def call(s):
            with torch.cuda.device(solver.device):
                assert solver.lib.sdk_check_batch(g.data_ptr(), ok.data_ptr(), n, mode, _stream_handle(solver, s)) == 0
        got, = _on_side_stream(solver, f"check mode {mode}", [(g, _dev(solver, grids[idx]))], call, [ok])
        assert np.array_equal(got.cpu().numpy(), want[mode][idx]), mode
    grids, cells, want = _candidate_cases()
    n = 257
    idx = _sized(grids, want, n)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    g, c = ain.boards(n, 2, name="grids"), ain.carve(4 * n, itemsize=4, name="cells")
    num = aout.carve(4 * n, itemsize=4, name="num")

    def call(s):
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_first_candidate_batch(g.data_ptr(), c.data_ptr(), num.data_ptr(), n,
                                                        _stream_handle(solver, s)) == 0
    # (cells of 0xFF bytes are -1: out of range, answered -1)
    got, = _on_side_stream(solver, "first_candidate", [(g, _dev(solver, grids[idx])), (c, _dev(solver, cells[idx]))],
                           call, [num])
    assert np.array_equal(got.cpu().numpy(), want[idx])


def test_stream_peer_solve(solver):
    from sudoku_solver_distributed_amd._lib import SDK_PEER_STATE_BYTES
    boards, rows, status, vals = _peer_cases()
    n = len(boards)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    b, out, st, val = _carve_peer(ain, aout, n, 1, 3)

    def call(s):
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_peer_solve_batch(b.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                                   _stream_handle(solver, s)) == 0
    got = _on_side_stream(solver, "peer_solve", [(b, _dev(solver, boards))], call, [out, st, val])
    assert np.array_equal(got[0].cpu().numpy(), rows) and np.array_equal(got[1].cpu().numpy(), status)
    assert np.array_equal(got[2].cpu().numpy(), vals)
    # one node, five requests: the state record is an input too (a new node's zeros)
    boards, rows, status, vals = _peer_seq_cases()
    n = len(boards)
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    b, out, st, val = _carve_peer(ain, aout, n, 2, 1)
    state = ain.carve(SDK_PEER_STATE_BYTES, align=16, name="node state")

    def call_seq(s):
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_peer_solve_seq(b.data_ptr(), out.data_ptr(), st.data_ptr(), val.data_ptr(), n,
                                                 state.data_ptr(), _stream_handle(solver, s)) == 0
    got = _on_side_stream(solver, "peer_solve_seq", [(b, _dev(solver, boards)), (state, solver.new_peer_state())],
                          call_seq, [out, st, val])
    assert np.array_equal(got[0].cpu().numpy(), rows) and np.array_equal(got[1].cpu().numpy(), status)
    assert np.array_equal(got[2].cpu().numpy(), vals)


def test_stream_expand(solver):
    """Three kernels (count, scan, write): one of them on another stream
    reads 0xFF nodes, unscanned counts or 0xA5 offsets."""
    n, order = 65, "node"
    nodes, answers = F.node_set(order)
    nd, ans = np.ascontiguousarray(nodes[-n:]), answers[-n:]
    cap = 9 * n
    ain, aout = Arena(solver.device, IN_FILL), Arena(solver.device, OUT_FILL)
    d_nodes = ain.boards(n, 3, name="nodes")
    tmp = aout.boards(n, 1, name="tmp")
    offsets = aout.carve(8 * (n + 1), itemsize=8, name="offsets")
    children = aout.boards(cap, 2, name="children")

    def call(s):
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_expand_frontier(d_nodes.data_ptr(), n, tmp.data_ptr(), offsets.data_ptr(),
                                                  children.data_ptr(), cap, ORDERS[order],
                                                  _stream_handle(solver, s)) == 0
    off, ch = _on_side_stream(solver, "expand", [(d_nodes, _dev(solver, nd))], call, [offsets, children], scratch=[tmp])
    off, ch = off.cpu().numpy(), ch.cpu().numpy()
    total = int(off[-1])
    assert 0 < total <= cap and (ch[total:] == OUT_FILL).all()
    F.check_level(nd, off, ch[:total], order, ans)
    aout.assert_guards()


# --------------------------------------------- e. deferred-list overflow
CLASHING, ORDINARY = (1 << 20) + 4097, 100_003


@functools.lru_cache(maxsize=None)
def _overflow_indices(clashing, ordinary, seed):
    rng = np.random.default_rng(seed)
    clash = A.kind_indices("clash")
    plain = np.concatenate([A.kind_indices("hard17"), A.kind_indices("gen")])
    idx = np.concatenate([clash[rng.integers(0, len(clash), clashing)], plain[rng.integers(0, len(plain), ordinary)]])
    return rng.permutation(idx)


@pytest.mark.parametrize("order", ["gen", "node"])
def test_deferred_list_overflow(solver, order):
    """More clashing-givens boards than the deferred list holds (2^20): the
    wave-per-board pass finds them by status.  Built on the device from the
    pool; unordered only.  Catches a deferred board skipped past the list's
    end (the last partial group of 64 included) and a stale overflow word in
    the call that follows."""
    P = A.pool()
    pb = _dev(solver, P["boards"])
    wr, ws = _dev(solver, P["want"][order][0]), _dev(solver, P["want"][order][1])
    prev = _kernel(solver, "plane")
    try:
        idx = _dev(solver, _overflow_indices(CLASHING, ORDINARY, 70))
        n = idx.numel()
        p = pb.index_select(0, idx)
        solver.stats(reset=True)
        out, st = solver.solve(p, order=order)
        assert torch.equal(st, ws.index_select(0, idx)) and torch.equal(out, wr.index_select(0, idx))
        stats = solver.stats(reset=True)
        assert stats["deferred"] > 2 ** 20 and stats["finished"] == n
        solver.verify()
        del p, out, st
        # ... the same through three batches of one launch sequence
        sizes = (400_001, 7, 750_003)
        idx = _dev(solver, _overflow_indices(CLASHING, sum(sizes) - CLASHING, 71))
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        ids = [idx[a:b] for a, b in zip(cuts, cuts[1:])]
        ps = [pb.index_select(0, i) for i in ids]
        outs = [torch.full_like(x, OUT_FILL) for x in ps]
        sts = [torch.full((x.shape[0],), 77, dtype=torch.int32, device=x.device) for x in ps]
        solver.solve_batches(ps, outs, sts, order=order)
        for i, o, s in zip(ids, outs, sts):
            assert torch.equal(s, ws.index_select(0, i)) and torch.equal(o, wr.index_select(0, i))
        stats = solver.stats(reset=True)
        assert stats["deferred"] > 2 ** 20 and stats["finished"] == sum(sizes)
        solver.verify()
    finally:
        solver.lib.sdk_set_solve_kernel(prev)
    # the next, ordinary call is unaffected (auto: the plane kernel at this size)
    n = 8192 + 63
    small = A.mixed(n, seed=72)
    out, st = solver.solve(pb.index_select(0, _dev(solver, small)), order=order)
    _assert_solved(out, st, order, small, "after the overflow")
    stats = solver.stats()
    assert stats["finished"] == n and 0 < stats["deferred"] < n
    solver.verify()
