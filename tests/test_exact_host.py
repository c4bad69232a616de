"""CPU checks of the exact completion count (csrc/plane_exact.h, what
exact_kernel's lanes run): the header compiled for the host with the round
loop simulated serially (tests/native/exact_host.cpp, built by
native_build.py) against the oracle's counter and the recorded fixture
(exact_cases.py), and the C ABI's argument checks through ctypes (no GPU)."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import count_cases as C
import exact_cases as E
from native_build import host_lib

GRIDS = (1, 3)  # simulated waves
PARTS = 4       # the pool runs as this many interleaved batches, side by side on the CPUs


@pytest.fixture(scope="module")
def host():
    return host_lib("exact_host")


def _slice(name):
    from sudoku_solver_distributed_amd.solver import EXACT_SLICE
    s, tasks = E.KNOBS[name]
    return (EXACT_SLICE if s is None else s), tasks


@pytest.fixture(scope="module")
def pool_runs(host):
    """Every (grid, knobs) over the whole pool, computed once: the host model
    is serial, so the runs (and the pool's PARTS interleaved batches) go side
    by side on threads -- the entry keeps no state and ctypes releases the GIL.
    (waves, knob name) -> list of (part's pool indices, count, status, stats)."""
    boards = E.pool()[0]
    jobs = [(w, name, np.arange(p, len(boards), PARTS)) for w in GRIDS for name in E.KNOBS for p in range(PARTS)]

    def run(job):
        w, name, idx = job
        s, tasks = _slice(name)
        return (idx,) + E.host_exact(host, boards[idx], waves=w, slice=s, max_tasks=tasks)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(run, jobs))
    out = {}
    for (w, name, _), r in zip(jobs, res):
        out.setdefault((w, name), []).append(r)
    return out


def test_fixture_is_what_it_claims():
    """The recorded heavy boards are the ones heavy() builds today, b's counts
    go with b's boards (spot-checked against the oracle on its six lightest),
    and the pool holds every kind of answer."""
    from oracle import oracle as O
    fx = E.load_fixture()
    assert np.array_equal(fx["h1"][0], E.heavy(E.H1_ERASED)) and fx["h1"][1] == E.H1_COUNT
    assert np.array_equal(fx["h2"][0], E.heavy(E.H2_ERASED)) and fx["h2"][1] == E.H2_COUNT
    b = C.sets()["b"]
    for i in np.argsort(fx["b"])[:6]:
        assert O.count_solutions(b[i], E.NO_LIMIT) == fx["b"][i]
    assert list(fx["b"][:6]) and fx["b"].min() >= 64 and fx["b"].max() > 100000
    boards, count, status = E.pool()
    assert len(boards) == 5 * 256 - 256 + 4 and not (boards == 0).all(axis=1).any()
    assert (status == E.INVALID).sum() == 1 and (count[status == E.INVALID] == 0).all()
    assert (count == 0).sum() > 256 and (count == 1).sum() > 64 and (count > 1024).sum() > 128


@pytest.mark.parametrize("waves", GRIDS)
@pytest.mark.parametrize("knobs", list(E.KNOBS))
def test_pool_counts_are_exact(pool_runs, waves, knobs):
    _, want, want_status = E.pool()
    s, _ = _slice(knobs)
    for idx, count, status, stats in pool_runs[(waves, knobs)]:
        bad = np.nonzero((count != want[idx]) | (status != want_status[idx]))[0]
        assert len(bad) == 0, [(int(idx[i]), int(count[i]), int(want[idx[i]]), int(status[i])) for i in bad[:10]]
        E.check_path(knobs, stats)
        print(waves, knobs, stats, "overshoot", stats["max_passes"] - s)
        assert stats["max_passes"] <= s + E.RUN_MAX  # DESIGN.md §20's bound of a round


def test_h1_alone_small_slice(host):
    h1, want = E.load_fixture()["h1"]
    count, status, stats = E.host_exact(host, h1, waves=3, slice=16)
    assert (int(count[0]), int(status[0])) == (want, E.DONE)
    assert stats["donated"] > 0 and stats["rounds"] > 1
    assert stats["max_passes"] <= 16 + E.RUN_MAX


def test_h1_additivity_and_symmetry(host):
    """The counts of H1 with one more clue (c, d), d = 1..9, add up to H1's
    (a clashing or impossible digit counts 0), and H1's images under two
    symmetries have H1's count."""
    from sudoku_solver_distributed_amd.gen import apply_symmetry
    h1, want = E.load_fixture()["h1"]
    cell = int(np.nonzero(h1 == 0)[0][7])
    plus = np.repeat(h1[None], 9, axis=0)
    plus[:, cell] = np.arange(1, 10)
    images, _ = apply_symmetry(np.repeat(h1[None], 2, axis=0), np.array([1234567, 1296 * 1296 + 424242]))
    count, status, _ = E.host_exact(host, np.concatenate([plus, images]), waves=3, slice=64)
    assert (status == E.DONE).all()
    assert int(count[:9].sum()) == want and (count[:9] > 0).sum() >= 2
    assert list(count[9:]) == [want, want]


def test_round_budget_gives_partial_and_spares_the_rest(host):
    """The empty board after three rounds: PARTIAL with a lower bound; the
    boards around it are DONE and exact."""
    boards, want, _ = E.pool()
    sel = np.nonzero((want > 0) & (want < 200))[0][:40]
    batch = np.concatenate([boards[sel[:20]], np.zeros((1, 81), np.uint8), boards[sel[20:]]])
    count, status, stats = E.host_exact(host, batch, waves=3, slice=256, max_rounds=3)
    assert stats["rounds"] == 3
    assert status[20] == E.PARTIAL and count[20] >= 0
    rest = np.arange(len(batch)) != 20
    assert (status[rest] == E.DONE).all() and np.array_equal(count[rest], want[sel])
    assert stats["max_passes"] <= 256 + E.RUN_MAX


def test_small_stack_faults_never_miscounts(host):
    """max_depth = 2 with a slice above any pass count (one task a board, as
    the capped count runs it): exactly the boards whose search goes deeper
    report SDK_FAULT with count 0; every other board its count."""
    cboards, _, _, _, names = C.pool()
    sel = np.nonzero((names == "a") | (names == "d") | (names == "f"))[0]
    sel = sel[cboards[sel].any(axis=1)]  # (not the empty board)
    boards = cboards[sel]
    full, full_status, _ = E.host_exact(host, boards, waves=1, slice=1 << 30)
    count, status, _ = E.host_exact(host, boards, waves=1, slice=1 << 30, max_depth=2)
    deep = np.zeros(len(boards), dtype=bool)
    cnt = host_lib("count_host")
    for k, g in enumerate(boards):
        c, p, d = np.zeros(1, np.int32), ctypes.c_uint64(), ctypes.c_uint32()
        cnt.count_host_batch(g.ctypes.data, c.ctypes.data, None, 1, 1024, 81, ctypes.byref(p), ctypes.byref(d))
        deep[k] = d.value > 2
    assert deep.sum() > 20 and (~deep).sum() > 20
    assert (status[deep] == E.FAULT).all() and (count[deep] == 0).all()
    assert np.array_equal(status[~deep], full_status[~deep]) and np.array_equal(count[~deep], full[~deep])


def test_host_model_argument_checks(host):
    g = np.zeros(81, np.uint8)
    c, s = np.zeros(1, np.int64), np.zeros(1, np.int32)
    f = host.exact_host_batch
    assert f(g.ctypes.data, c.ctypes.data, s.ctypes.data, 1, 1, 0, 1, 0, 81, None) == -2   # slice 0
    assert f(g.ctypes.data, c.ctypes.data, s.ctypes.data, 1, 1, 1, 0, 0, 81, None) == -2   # max_rounds 0
    assert f(g.ctypes.data, c.ctypes.data, s.ctypes.data, 1, 1, 1, 1, -1, 81, None) == -2  # max_tasks < 0
    assert f(None, None, None, 0, 1, 0, 0, -1, 81, None) == 0                              # n == 0 first


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_count_exact_batch, L.sdk_count_exact_scratch_bytes
    need = sb(100, 2, 64)
    assert need > 0

    def call(boards=64, count=64, status=64, n=100, slice=8, rounds=4, tasks=64, scratch=64, size=need, waves=2):
        return f(boards, count, status, n, slice, rounds, tasks, scratch, size, waves, None, None)

    assert call(slice=0) == -2
    assert call(rounds=0) == -2
    assert call(tasks=-1) == -2
    assert call(n=-1) == -2
    assert call(waves=-1) == -2
    assert call(n=2 ** 31) == -2
    assert call(boards=None) == -2 and call(count=None) == -2 and call(status=None) == -2 and call(scratch=None) == -2
    assert call(count=68) == -2      # d_count needs 8-byte alignment
    assert call(status=66) == -2     # d_status 4
    assert call(scratch=72) == -2    # the scratch 16
    assert call(size=need - 1) == -2
    assert call(slice=2 ** 31 - 1, rounds=2 ** 31 - 1) == -2  # a pass budget of 2^63: d_count could overflow
    assert f(None, None, None, 0, 0, 0, -1, None, 0, -1, None, None) == 0  # n == 0 before any other check
    from sudoku_solver_distributed_amd import _lib
    assert (_lib.SDK_EXACT_DONE, _lib.SDK_EXACT_PARTIAL) == (1, 2)


def test_scratch_bytes_formula(L):
    sb = L.sdk_count_exact_scratch_bytes
    wave = 64 * 81 * 128 + 64 * 8
    assert sb(0, 1, 1) == 256 + wave + 2 * 128
    assert sb(100, 2, 64) == 256 + 2 * wave + 2 * 64 * 128 + 400
    assert sb(101, 2, 64) == 256 + 2 * wave + 2 * 64 * 128 + 416      # the counters rounded up to 16
    assert sb(100, 3, 0) == 256 + 3 * wave + 2 * (4 * 64 * 3) * 128 + 400  # the default: four tasks a lane
    full = L.sdk_device_cu_count() * 16  # at most four waves on each of a CU's four SIMDs
    assert sb(1, 0, 0) <= 256 + full * (wave + 8 * 64 * 128) + 16
    assert sb(1, 0, 0) == sb(1 << 20, 0, 0) - (4 << 20) + 16          # the grid does not depend on n
    assert sb(-1, 0, 0) == 0 and sb(1, -1, 0) == 0 and sb(1, 0, -1) == 0 and sb(2 ** 31, 0, 0) == 0
    assert sb(1, 0, 2 ** 31) == 0
