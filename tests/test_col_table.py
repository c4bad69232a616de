"""CPU checks of rule C's column table (csrc/plane_solver.h: col_fill,
col_entry, col_offset and the passes that take plane::PassTables -- what the
plane kernel's lane loop runs with SDK_PLANE_COLTBL): every entry is the
arithmetic of the pass on its column pattern, and a pass with the tables
leaves what the pass without them leaves.  The header compiled for the host
(tests/native/col_table_host.cpp over csrc/host_model.h)."""
import ctypes

import numpy as np
import pytest

import native_build
from oracle import oracle as O

_vp, _i64, _int, _u32, _u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
native_build.PROTOS.setdefault("col_table_host", {
    "col_table_entries": ([], _int),
    "col_table_box_shift": ([], _u32),
    "col_table_fill": ([_vp, _vp, _u32], None),
    "col_table_offset": ([_u32], _u32),
    "col_table_arith": ([_u32, _vp, _vp], None),
    # in, n, lock, col, node_order, max_depth, mrv_after, passes, tot[5]
    "col_table_lockstep": ([_vp, _i64, _vp, _vp, _int, _u32, _u32, _vp, _vp], _i64),
    "col_table_pass_random": ([_vp, _vp, _i64, _u64], _i64),
    "col_table_old_overloads": ([_vp, _i64, _u64], _i64),
})

ROWS = 0x1FF | (0x1FF << 10) | (0x1FF << 20)
FULL = "534678912672195348198342567859761423426853791713924856961537284287419635345286179"


def b81(s):
    return np.frombuffer(s.encode(), np.uint8) - ord("0")


@pytest.fixture(scope="module")
def col():
    return native_build.host_lib("col_table_host")


def _fill(col, nthreads):
    lock = np.full(512, 0xFFFFFFFF, np.uint32)
    ctab = np.full(512, 0xFFFF, np.uint16)
    col.col_table_fill(lock.ctypes.data, ctab.ctypes.data, nthreads)
    return lock, ctab


@pytest.fixture(scope="module")
def tables(col):
    """both tables as a 256-thread workgroup fills them (the kernel's own fill functions)"""
    return _fill(col, 256)


def test_fill_is_the_same_for_any_workgroup_size(col, tables):
    assert col.col_table_entries() == 512
    for nthreads in (1, 64, 100, 256, 1024):
        lock, ctab = _fill(col, nthreads)
        assert np.array_equal(lock, tables[0]) and np.array_equal(ctab, tables[1]), nthreads


def test_every_entry_is_the_pass_arithmetic(col, tables):
    """all 512 column patterns: vp in bits 0-8, the box bits 0/3/6 moved up by the shift, nothing else"""
    sh = col.col_table_box_shift()
    assert sh >= 9 and 6 + sh < 16
    vp, boxes = ctypes.c_uint32(0), ctypes.c_uint32(0)
    for i in range(512):
        col.col_table_arith(i, ctypes.byref(vp), ctypes.byref(boxes))
        e = int(tables[1][i])
        assert e & 0x1FF == vp.value, i
        assert e >> sh == boxes.value, i
        assert e & ~(0x1FF | (0x49 << sh)) == 0, i
        # and the arithmetic is what it says: a box's column is in vp iff it is the box's only occupied one
        for j in range(3):
            cols = (i >> (3 * j)) & 7
            assert (boxes.value >> (3 * j)) & 1 == (cols != 0)
            assert (vp.value >> (3 * j)) & 7 == (cols if cols in (1, 2, 4) else 0)


def test_offset_ignores_what_lies_above_the_nine_columns(col):
    rng = np.random.default_rng(5)
    for i in range(512):
        assert col.col_table_offset(i) == 2 * i
        for hi in rng.integers(0, 1 << 23, 8):
            assert col.col_table_offset(i | (int(hi) << 9)) == 2 * i
    assert col.col_table_offset(0xFFFFFFFF) == 2 * 511


def _gen_style(n, empties, seed):
    """gen.py-style boards on the CPU: complete grids with cells erased"""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    grids, _ = O.solve_unique_batch(hard17_batch(n, seed=seed).numpy())
    rng = np.random.default_rng(seed)
    for g in grids:
        g[rng.choice(81, empties, replace=False)] = 0
    return grids


def _edge_boards():
    """dead boards and clashing givens, as tests/test_pass_ahead.py builds them"""
    dup = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
    dead = np.zeros(81, np.uint8)  # cell (8, 8) has no candidate: row 8 holds 2..9, column 8 a 1
    dead[72:80] = [2, 3, 4, 5, 6, 7, 8, 9]
    dead[63 + 8] = 1
    dead2 = b81(FULL).copy()  # a full grid with one cell emptied and its digit's twin next to it changed
    dead2[0] = 0
    dead2[1] = 5
    return np.array([b81("0" * 81), b81(FULL), b81(FULL[:40] + "0" + FULL[41:]), dead, dead2, b81("5" * 81), b81(dup)],
                    dtype=np.uint8)


@pytest.fixture(scope="module")
def boards():
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    return np.ascontiguousarray(np.concatenate([hard17_batch(1500, seed=31).numpy(),
                                                hard_search_batch(512, seed=32).numpy(), _gen_style(512, 50, 33),
                                                _edge_boards()]))


def _lockstep(col, boards, lock, ctab, order):
    passes = ctypes.c_uint64(0)
    tot = np.zeros(5, np.uint64)
    bad = col.col_table_lockstep(boards.ctypes.data, len(boards), lock.ctypes.data, ctab.ctypes.data,
                                 int(order == "node"), 32, 128, ctypes.byref(passes), tot.ctypes.data)
    return bad, passes.value, [int(v) for v in tot]


@pytest.mark.parametrize("order", ["gen", "node"])
def test_pass_ahead_with_tables_lockstep_with_pass_ahead(col, tables, boards, order):
    """pass_ahead with both tables against pass_ahead, from the same state,
    after every pass of the searches of hard 17-clue, search-heavy, gen-style,
    dead and clashing boards: planes, verdict, und and nd identical; and the
    searches run on the tables alone take the same passes and guesses to the
    same ends."""
    bad, passes, tot = _lockstep(col, boards, tables[0], tables[1], order)
    print("passes compared", passes, "totals", tot)
    assert passes > 10 * len(boards)
    assert bad == 0
    assert tot[0] == tot[2] and tot[1] == tot[3] and tot[4] == 0


def test_lockstep_sees_a_wrong_entry(col, tables, boards):
    ctab = tables[1].copy()
    ctab &= np.uint16(0xFE00)  # no box ever has one column: rule D's box -> column form and the box singles off
    bad, _, _ = _lockstep(col, boards[1400:1600], tables[0], ctab, "gen")
    assert bad > 0
    ctab = tables[1].copy()
    ctab[0b100010001] ^= 1 << col.col_table_box_shift()  # one entry: box 0 holds a place and says it has none
    bad, _, _ = _lockstep(col, boards[1400:1600], tables[0], ctab, "gen")
    assert bad > 0


def test_passes_with_tables_on_random_planes(col, tables):
    assert col.col_table_pass_random(tables[0].ctypes.data, tables[1].ctypes.data, 200_000, 7) == 0


def test_old_overloads_read_the_lock_table_only(col, tables):
    """pass / pass_ahead given a bare pointer: 512 words, then guard words whose
    values would change the result if the pass looked anything up there (as
    column entries they claim one-column boxes everywhere; as keep masks they
    clear every cell)"""
    for poison in (0x00000000, 0xFFFFFFFF, 0x01FF01FF, 0x92009200):
        buf = np.concatenate([tables[0], np.full(1024, poison, np.uint32)])
        assert col.col_table_old_overloads(buf.ctypes.data, 20_000, 11) == 0
