"""CPU checks of the completion list (csrc/plane_enum.h, what enum_kernel's
lanes run): the header compiled for the host with the round loop simulated
serially (tests/native/enum_host.cpp, built by native_build.py).  A list is
checked as a set (enum_cases.py): rows valid, givens kept, rows distinct,
their number the exact count the fixture or the oracle knows.  Then the
overflow rule, the per-board limit, PARTIAL, the corners, and the C ABI's
argument checks through ctypes (no GPU)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import enum_cases as N
from native_build import host_lib

GRIDS = (1, 3)  # simulated waves


@pytest.fixture(scope="module")
def host():
    return host_lib("enum_host")


def _slice(name):
    from sudoku_solver_distributed_amd.solver import EXACT_SLICE
    s, tasks = N.KNOBS[name]
    return (EXACT_SLICE if s is None else s), tasks


@pytest.fixture(scope="module")
def selection():
    """Pool indices: every board with at most 1022 completions (a byte > 9
    and clashing givens among them), and the three lightest of set b (up to
    about 10^5 completions)."""
    _, count, _ = N.pool()
    b = np.nonzero(N.pool_sets() == "b")[0]
    b = b[(count[b] > 1022) & (count[b] <= 100000)]
    b = b[np.argsort(count[b], kind="stable")]
    heavy = np.concatenate([b[:2], b[-1:]])  # the two lightest of them and the heaviest
    assert len(set(heavy.tolist())) == 3 and count[heavy].max() > 30000
    return np.concatenate([np.nonzero(count <= 1022)[0], heavy])


@pytest.fixture(scope="module")
def runs(host, selection):
    """Every (grid, knobs) over the selection, once, side by side on threads
    (the entry keeps no state and ctypes releases the GIL)."""
    boards, count, _ = N.pool()
    sel = boards[selection]
    total = int(count[selection].sum())
    jobs = [(w, name) for w in GRIDS for name in N.KNOBS]

    def run(job):
        w, name = job
        s, tasks = _slice(name)
        return N.host_enum(host, sel, total + 3, waves=w, slice=s, max_tasks=tasks)

    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
        return dict(zip(jobs, ex.map(run, jobs)))


@pytest.mark.parametrize("waves", GRIDS)
@pytest.mark.parametrize("knobs", list(N.KNOBS))
def test_lists_are_the_completion_sets(runs, selection, waves, knobs):
    boards, want, want_status = N.pool()
    grids, owner, count, status, info = runs[(waves, knobs)]
    assert np.array_equal(count, want[selection]) and np.array_equal(status, want_status[selection])
    assert info["total"] == info["listed"] == int(want[selection].sum())
    N.check_complete(boards[selection], grids, owner, info["listed"], want[selection])
    N.check_path(knobs, info)
    s, _ = _slice(knobs)
    assert info["max_passes"] <= s + N.RUN_MAX
    assert (status == N.INVALID).sum() == 1 and (want[selection] == 0).sum() > 256


def test_sorted_lists_are_identical_across_knobs_and_grids(runs, selection):
    """The set never depends on the knobs or the grid; lanes donated and
    parked on the way."""
    ref = None
    for key, (grids, owner, _, _, info) in runs.items():
        rows, off = N.by_board(grids, owner, info["listed"], len(selection))
        if ref is None:
            ref = (rows, off)
        assert np.array_equal(rows, ref[0]) and np.array_equal(off, ref[1]), key
    assert any(info["donated"] > 0 for *_, info in runs.values())
    assert any(info["parks"] > 0 for *_, info in runs.values())


@pytest.fixture(scope="module")
def few():
    """40 light boards with completions and their exact counts."""
    boards, want, _ = N.pool()
    idx = N.light(40)
    return boards[idx], want[idx]


def test_overflow_drops_rows_and_keeps_counts(host, few):
    boards, want = few
    total = int(want.sum())
    assert total > 40
    for capacity in (1, total - 1, total):
        for waves, slice in ((1, 4096), (3, 1)):
            grids, owner, count, status, info = N.host_enum(host, boards, capacity, waves=waves, slice=slice)
            assert info["total"] == total and info["listed"] == min(total, capacity)
            assert np.array_equal(count, want) and (status == N.DONE).all()
            per = N.check_listed(boards, grids, owner, info["listed"])
            assert (per <= want).all()
            if capacity == total:
                assert np.array_equal(per, want)


def test_limit_is_strict(host, few):
    """Limits of 1, 2 and 64 on boards with fewer, exactly and more
    completions: LIMITED has exactly `limit` distinct valid rows and count ==
    limit, the others are DONE and complete, capacity = n * limit never
    overflows."""
    boards, want = few
    assert (want == 1).any() and (want == 2).any() and (want < 64).any() and (want > 64).any() and (want > 2).any()
    for limit in (1, 2, 64):
        for waves, slice, tasks in ((1, 4096, 0), (3, 1, 0), (3, 8, 64)):
            grids, owner, count, status, info = N.host_enum(host, boards, len(boards) * limit, limit=limit, waves=waves,
                                                            slice=slice, max_tasks=tasks)
            lim = want >= limit
            assert np.array_equal(status, np.where(lim, N.LIMITED, N.DONE)), (limit, waves)
            assert np.array_equal(count, np.minimum(want, limit))
            assert info["total"] == info["listed"] == int(count.sum()) <= len(boards) * limit
            N.check_complete(boards, grids, owner, info["listed"], count)


def test_limit_rows_are_rows_of_the_full_list(host, few):
    boards, want = few
    full = N.host_enum(host, boards, int(want.sum()))
    grids, owner, count, _, info = N.host_enum(host, boards, 2 * len(boards), limit=2, waves=3, slice=1)
    key = lambda g, o, m: set(zip(o[:m].tolist(), N.row_keys(g[:m]).tolist()))  # noqa: E731
    assert key(grids, owner, info["listed"]) <= key(full[0], full[1], full[4]["listed"])


def test_one_heavy_board_stops_at_its_limit(host):
    """The empty board with limit 64 among light boards: 64 completions, not
    max_rounds rounds."""
    boards, want = N.pool()[0][N.light(8)], N.pool()[1][N.light(8)]
    batch = np.concatenate([boards[:4], np.zeros((1, 81), np.uint8), boards[4:]])
    grids, owner, count, status, info = N.host_enum(host, batch, 9 * 64, limit=64, waves=3, slice=16)
    exp = np.concatenate([want[:4], [2 ** 40], want[4:]])
    assert np.array_equal(count, np.minimum(exp, 64)) and status[4] == N.LIMITED
    assert np.array_equal(status, np.where(exp >= 64, N.LIMITED, N.DONE))
    N.check_complete(batch, grids, owner, info["listed"], count)
    assert info["rounds"] < 64


def test_round_budget_gives_partial_with_its_rows(host, few):
    """The empty board and a set-b board after three rounds: PARTIAL, rows
    valid and distinct, count == the board's rows <= the exact count; the
    boards around them DONE and complete."""
    boards, want = few
    h1, h1_count = N.load_fixture()["h1"]
    assert h1_count > 3 * (1024 + N.RUN_MAX) * 192  # more completions than the call has passes
    batch = np.concatenate([boards[:20], np.zeros((1, 81), np.uint8), h1[None], boards[20:]])
    grids, owner, count, status, info = N.host_enum(host, batch, 1 << 20, waves=3, slice=1024, max_rounds=3)
    assert info["rounds"] == 3 and info["listed"] == info["total"]
    assert status[20] == N.PARTIAL and status[21] == N.PARTIAL and 0 <= count[21] <= h1_count
    rest = np.setdiff1d(np.arange(len(batch)), [20, 21])
    assert (status[rest] == N.DONE).all() and np.array_equal(count[rest], want)
    N.check_complete(batch, grids, owner, info["listed"], count)
    assert count[20] + count[21] > 0


def test_corners(host):
    """Clashing givens, a byte > 9 and the full grid (one row: itself);
    capacity 0 against the exact count's host model."""
    import exact_cases as E
    boards, want, want_status = N.pool()
    full = boards[np.nonzero((boards != 0).all(axis=1) & (want == 1))[0][0]]
    clash = boards[np.nonzero((want == 0) & (want_status == N.DONE) & (N.pool_sets() == "f"))[0][0]]
    bad = boards[want_status == N.INVALID][0]
    grids, owner, count, status, info = N.host_enum(host, np.stack([clash, bad, full]), 4)
    assert count.tolist() == [0, 0, 1] and status.tolist() == [N.DONE, N.INVALID, N.DONE]
    assert info["total"] == info["listed"] == 1 and owner[0] == 2 and np.array_equal(grids[0], full)
    assert (grids[1:] == 0xA5).all() and (owner[1:] == -7).all()
    idx = np.concatenate([N.light(60), np.nonzero(want_status == N.INVALID)[0]])
    for waves, slice, tasks in ((1, 256, 0), (3, 8, 64)):
        _, _, count, status, info = N.host_enum(host, boards[idx], 0, waves=waves, slice=slice, max_tasks=tasks)
        c2, s2, st2 = E.host_exact(host_lib("exact_host"), boards[idx], waves=waves, slice=slice, max_tasks=tasks)
        assert np.array_equal(count, c2) and np.array_equal(status, s2)
        assert info["listed"] == 0 and info["total"] == int(c2.sum())
        assert [info[k] for k in ("rounds", "donated", "parks", "max_passes")] == [st2[k] for k in st2]


def test_host_model_argument_checks(host):
    g = np.zeros(81, np.uint8)
    c, s, r, o = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(81, np.uint8), np.zeros(1, np.int32)
    f = host.enum_host_batch

    def call(grids=r.ctypes.data, owner=o.ctypes.data, capacity=1, limit=0, slice=1, rounds=1, tasks=0):
        return f(g.ctypes.data, 1, grids, owner, capacity, limit, c.ctypes.data, s.ctypes.data, 1, slice, rounds, tasks,
                 81, None)

    assert call() == 0
    assert call(capacity=-1) == -2 and call(limit=-1) == -2 and call(capacity=2 ** 31) == -2
    assert call(grids=None) == -2 and call(owner=None) == -2
    assert call(grids=None, owner=None, capacity=0) == 0
    assert call(slice=0) == -2 and call(rounds=0) == -2 and call(tasks=-1) == -2
    assert f(None, 0, None, None, -1, -1, None, None, 0, 0, 0, -1, 81, None) == 0  # n == 0 first


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_enumerate_batch, L.sdk_enumerate_scratch_bytes
    need = sb(100, 2, 64)
    assert need == L.sdk_count_exact_scratch_bytes(100, 2, 64) > 0

    def call(boards=64, n=100, grids=64, owner=64, capacity=8, limit=0, count=64, status=64, slice=8, rounds=4,
             tasks=64, scratch=64, size=need, waves=2):
        return f(boards, n, grids, owner, capacity, limit, count, status, slice, rounds, tasks, scratch, size, waves,
                 None, None)

    assert call(capacity=-1) == -2 and call(limit=-1) == -2 and call(capacity=2 ** 31) == -2
    assert call(grids=None) == -2 and call(owner=None) == -2 and call(owner=66) == -2
    assert call(slice=0) == -2 and call(rounds=0) == -2 and call(tasks=-1) == -2 and call(n=-1) == -2
    assert call(waves=-1) == -2 and call(n=2 ** 31) == -2
    assert call(boards=None) == -2 and call(count=None) == -2 and call(status=None) == -2 and call(scratch=None) == -2
    assert call(count=68) == -2 and call(status=66) == -2 and call(scratch=72) == -2 and call(size=need - 1) == -2
    assert call(slice=2 ** 31 - 1, rounds=2 ** 31 - 1) == -2  # a pass budget of 2^63
    assert f(None, 0, None, None, -1, -1, None, None, 0, 0, -1, None, 0, -1, None, None) == 0  # n == 0 first
    assert sb(-1, 0, 0) == 0 and sb(1, -1, 0) == 0 and sb(1, 0, -1) == 0 and sb(2 ** 31, 0, 0) == 0
    wave = 64 * 81 * 128 + 64 * 8
    assert sb(101, 2, 64) == 256 + 2 * wave + 2 * 64 * 128 + 416
    from sudoku_solver_distributed_amd import _lib
    assert (_lib.SDK_ENUM_DONE, _lib.SDK_ENUM_PARTIAL, _lib.SDK_ENUM_LIMITED) == (1, 2, 3)
