"""CPU checks of rule D's box -> row table (csrc/plane_solver.h: lock_fill,
lock_index, lock_entry, and the passes that take the table -- what the plane
kernel's lane loop runs with SDK_PLANE_LOCKTBL): the lookup is
point_rows_apply on every band word, and a pass with the table leaves what the
pass without it leaves.  The header compiled for the host
(tests/native/lock_table_host.cpp over csrc/host_model.h)."""
import ctypes

import numpy as np
import pytest

import native_build
from oracle import oracle as O

_vp, _i64, _int, _u32, _u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
native_build.PROTOS.setdefault("lock_table_host", {
    "lock_table_fill": ([_vp, _u32], None),
    "lock_table_index": ([_u32], _u32),
    "lock_table_check_all": ([_vp, _vp], _i64),
    # in, n, tbl, node_order, max_depth, mrv_after, passes
    "lock_table_lockstep": ([_vp, _i64, _vp, _int, _u32, _u32, _vp], _i64),
    "lock_table_pass_random": ([_vp, _i64, _u64], _i64),
})

ROWS = 0x1FF | (0x1FF << 10) | (0x1FF << 20)
GUARDS = (1 << 9) | (1 << 19) | (1 << 29)


@pytest.fixture(scope="module")
def lock():
    return native_build.host_lib("lock_table_host")


@pytest.fixture(scope="module")
def table(lock):
    """the table as a 256-thread workgroup fills it (the kernel's own fill function)"""
    tbl = np.full(512, 0xFFFFFFFF, np.uint32)
    lock.lock_table_fill(tbl.ctypes.data, 256)
    return tbl


def test_fill_is_the_same_for_any_workgroup_size(lock, table):
    for nthreads in (1, 64, 100, 512, 1024):
        t = np.full(512, 0xFFFFFFFF, np.uint32)
        lock.lock_table_fill(t.ctypes.data, nthreads)
        assert np.array_equal(t, table), nthreads


def test_entries_keep_guard_bits_clear(table):
    assert not (table & ~np.uint32(ROWS)).any()
    assert not (table & np.uint32(GUARDS)).any()
    assert table[0] == ROWS and table[511] == ROWS  # no place / every mini-row: nothing points


def test_index_is_the_mini_row_pattern(lock):
    """bit 3j + k of the index: row k of box j of the band word holds a place"""
    for k in range(3):
        for j in range(3):
            for c in range(3):
                assert lock.lock_table_index(1 << (10 * k + 3 * j + c)) == 1 << (3 * j + k)
    assert lock.lock_table_index(0) == 0 and lock.lock_table_index(ROWS) == 511


def test_lookup_is_point_rows_apply_on_every_band_word(lock, table):
    """all 2^27 band words: y & tbl[lock_index(y)] == point_rows_apply(y)"""
    first = ctypes.c_uint32(0)
    bad = lock.lock_table_check_all(table.ctypes.data, ctypes.byref(first))
    assert bad == 0, "first differing word 0x%08x" % first.value


def test_a_wrong_entry_is_seen(lock, table):
    """the exhaustive check does fail on a table with one bit of one entry off"""
    t = table.copy()
    t[0b000000011] ^= 1 << 0  # rows 0 and 1 of box 0 hold places: the entry drops a cell of row 0 it must keep
    first = ctypes.c_uint32(0)
    assert lock.lock_table_check_all(t.ctypes.data, ctypes.byref(first)) > 0


def _gen_style(n, empties, seed):
    """gen.py-style boards on the CPU: complete grids with cells erased"""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    grids, _ = O.solve_unique_batch(hard17_batch(n, seed=seed).numpy())
    rng = np.random.default_rng(seed)
    for g in grids:
        g[rng.choice(81, empties, replace=False)] = 0
    return grids


@pytest.fixture(scope="module")
def boards():
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    return np.ascontiguousarray(np.concatenate([hard17_batch(300, seed=11).numpy(),
                                                hard_search_batch(300, seed=12).numpy(), _gen_style(200, 50, 13)]))


@pytest.mark.parametrize("order", ["gen", "node"])
def test_pass_ahead_with_table_lockstep_with_pass_ahead(lock, table, boards, order):
    """pass_ahead with the table against pass_ahead, from the same state, after
    every pass of the searches of hard 17-clue, search-heavy and gen-style
    boards: planes, verdict, und and nd identical."""
    passes = ctypes.c_uint64(0)
    bad = lock.lock_table_lockstep(boards.ctypes.data, len(boards), table.ctypes.data, int(order == "node"), 32, 128,
                                   ctypes.byref(passes))
    print("passes compared", passes.value)
    assert passes.value > 10 * len(boards)
    assert bad == 0


def test_lockstep_sees_a_wrong_entry(lock, table, boards):
    t = table.copy()
    t[:] = ROWS  # a table that never clears anything: rule D's box -> row form off
    passes = ctypes.c_uint64(0)
    assert lock.lock_table_lockstep(boards.ctypes.data, 100, t.ctypes.data, 0, 32, 128, ctypes.byref(passes)) > 0


def test_pass_with_table_on_random_planes(lock, table):
    assert lock.lock_table_pass_random(table.ctypes.data, 200_000, 7) == 0
