"""CPU checks of the unavoidable sets (csrc/ua.h, what the ua kernels run):
the fixture tests/golden/ua_cases.json itself -- the enumeration at 9 cells
and the Python restatement at 12, neither of which ua.h had a part in --
against the figures DESIGN.md §24 lists; the header compiled for the host
(tests/native/ua_host.cpp) against the fixture in rows (as multisets), counts,
statuses and minimal sets at max_size 4, 6, 9 and 12; the nesting of the rows
in max_size; the filter's host model against the subset definition; the
stand-alone program under the sanitizers; and the C ABI's argument checks
through ctypes (no GPU).  Every check is an equality."""
import ctypes
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import native_build
import ua_cases as U

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
native_build.PROTOS.setdefault("ua_host", {
    # grids, n, max_size, rows, capacity, count, status, info (2 x int64), nodes (NULL ok) -> 0 / -2
    "ua_host_batch": ([_vp, _i64, _int, _vp, _i64, _vp, _vp, _vp, _vp], _int),
    "ua_host_batch_split": ([_vp, _i64, _int, _vp, _i64, _vp, _vp, _vp, _vp, _int], _int),  # ... and split (0 / 1)
    "ua_host_minimal": ([_vp, _vp, _i64, _vp], None),  # rows, offsets, groups, keep
})


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("ua_host", openmp=True)


@pytest.fixture(scope="module")
def cases():
    return U.load_fixture()


def run_host(lib, grids, max_size, capacity=1 << 16, split=0):
    grids = np.ascontiguousarray(grids, dtype=np.uint8).reshape(-1, 81)
    n = len(grids)
    rows = np.full((capacity, 4), 0xA5A5A5A5, dtype=np.uint32)
    count = np.full(n, 12345, dtype=np.int32)
    status = np.full(n, 12345, dtype=np.int32)
    info = np.zeros(2, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.uint64)
    rc = lib.ua_host_batch_split(grids.ctypes.data, n, max_size, rows.ctypes.data, capacity, count.ctypes.data,
                                 status.ctypes.data, info.ctypes.data, nodes.ctypes.data, split)
    assert rc == 0
    assert (rows[info[1]:] == 0xA5A5A5A5).all()
    return rows[:info[1]], count, status, (int(info[0]), int(info[1])), nodes


def host_minimal(lib, rows, offsets):
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 4)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    keep = np.full(max(len(rows), 1), 77, dtype=np.uint8)
    lib.ua_host_minimal(rows.ctypes.data, offsets.ctypes.data, len(offsets) - 1, keep.ctypes.data)
    return keep[:len(rows)]


def test_fixture_is_what_the_design_lists(cases):
    """The recorded answers themselves: the grids, the cyclic grid's figures,
    the enumeration equal to the restatement up to 9 cells, a small set in
    every hard17 grid, the digit bound and the link fact's consequence that
    a minimal set's cells are all distinct rows."""
    names = [c.name for c in cases]
    assert names == (["cyclic"] + [f"hard17_{k}" for k in range(12)] + [f"random_{k}" for k in range(8)]
                     + ["byte_0", "byte_10", "row_repeat"])
    for c in cases:
        assert c.status == U.status_of(c.grid), c.name
    assert [c.status for c in cases[-3:]] == [U.INVALID, U.INVALID, U.NOT_A_GRID]
    cyc = cases[0]
    assert np.array_equal(cyc.grid, U.cyclic_grid())
    sizes = lambda masks: dict(Counter(bin(m).count("1") for m in masks))
    assert sum(cyc.rows(8).values()) == 81 and sizes(cyc.minimal(8)) == {6: 81}
    assert sum(cyc.rows(10).values()) == 99 and len(cyc.rows(10)) == 90 and sizes(cyc.minimal(10)) == {6: 81}
    assert sum(cyc.rows(12).values()) == 963 and sizes(cyc.minimal(12)) == {6: 81, 12: 54}
    assert sum(cyc.rows(5).values()) == 0
    assert sum(cyc.enum9.values()) == 99  # (the 18 rows beyond 8 cells have 9)
    for c in U.valid_cases():
        assert c.rows(9) == c.enum9, c.name
        g = [int(v) for v in c.grid]
        for m in c.rows12:
            cells = U.cells_of(m)
            digits = Counter(g[x] for x in cells)
            assert min(digits.values()) >= 2 and len(digits) <= len(cells) // 2, c.name
        assert set(c.minimal(12)) == {m for m, f in zip(list(c.rows12), U.minimal_flags(list(c.rows12))) if f}
        if c.name.startswith("hard17_"):
            assert any(bin(m).count("1") in (4, 6) for m in c.minimal(12)), c.name


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("max_size", [4, 6, 9, 12])
def test_host_matches_fixture(host, cases, max_size, split):
    """Task by task, and with every task cut into its eight split tasks (what
    the kernel runs on a small batch)."""
    grids = np.stack([c.grid for c in cases])
    rows, count, status, (total, listed), _ = run_host(host, grids, max_size, split=split)
    assert total == listed == len(rows)
    assert status.tolist() == [c.status for c in cases]
    got = U.by_owner(rows, len(cases))
    for i, c in enumerate(cases):
        want = c.rows(max_size)
        assert got[i] == want, (c.name, sum(got[i].values()), sum(want.values()))
        assert count[i] == sum(want.values()), c.name
    # the minimal sets: the filter's host model on the rows grouped by owner
    order = np.argsort(rows[:, 3], kind="stable")
    grouped = rows[order]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(grouped[:, 3], minlength=len(cases)))])
    keep = host_minimal(host, grouped, offsets)
    for i, c in enumerate(cases):
        mine = grouped[offsets[i]:offsets[i + 1]][keep[offsets[i]:offsets[i + 1]] == 1]
        masks = U.words_to_masks(mine)
        assert len(set(masks)) == len(masks) and sorted(masks, key=U.sort_key) == c.minimal(max_size), c.name


def test_rows_nest_in_max_size(host, cases):
    """m = 4 and 5 give the same rows; the rows at m are the rows at m + 1
    of at most m cells, m = 4..13, on four grids."""
    pick = [cases[0], cases[1], cases[13], cases[20]]
    grids = np.stack([c.grid for c in pick])
    prev = None
    for m in range(14, 3, -1):
        rows, count, _, _, _ = run_host(host, grids, m, capacity=1 << 17)
        now = U.by_owner(rows, len(pick))
        assert [sum(c.values()) for c in now] == count.tolist()
        if prev is not None:
            for a, b in zip(now, prev):
                assert a == Counter({k: v for k, v in b.items() if bin(k).count("1") <= m}), m
        if m == 5:
            five = now
        prev = now
    assert prev == five and all(bin(k).count("1") == 4 for c in prev for k in c)


def test_capacity_and_bad_arguments_of_the_host_model(host, cases):
    grids = np.stack([c.grid for c in cases[:3]])
    _, count, _, (total, _), _ = run_host(host, grids, 8)
    rows, count2, _, (total2, listed2), _ = run_host(host, grids, 8, capacity=total - 1)
    assert (total2, listed2) == (total, total - 1) and np.array_equal(count, count2)
    _, count0, _, info0, _ = run_host(host, grids, 8, capacity=0)
    assert info0 == (total, 0) and np.array_equal(count, count0)
    z = np.zeros(4, dtype=np.int64)
    for m in (3, 17):
        assert host.ua_host_batch(grids.ctypes.data, 3, m, None, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -2


def test_minimal_filter_against_the_definition(host, cases):
    """Shuffled groups with duplicates: keep[k] is 1 exactly when no row of
    the group is a proper subset of row k and no earlier row equals it --
    by Python ints here."""
    rng = np.random.default_rng(24)
    groups = []
    for c in (cases[0], cases[2], cases[15]):
        masks = list(c.rows(12).elements())
        masks += [masks[k] for k in rng.integers(0, len(masks), 40)]
        groups.append([masks[k] for k in rng.permutation(len(masks))])
    groups.insert(1, [])                          # an empty group
    groups.append([0b1111, 0b0111, 0b0111, 1 << 80 | 0b0111, 1 << 80])   # hand-made: subsets across the words
    groups.append([(1 << 81) - 1])
    rows = np.concatenate([U.rows_to_words(g, owner=99 + i) for i, g in enumerate(groups)])
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    keep = host_minimal(host, rows, offsets)
    for i, g in enumerate(groups):
        want = [int(not any((g[j] == g[k] and j < k) or (g[j] != g[k] and g[j] & ~g[k] == 0) for j in range(len(g))))
                for k in range(len(g))]
        assert keep[offsets[i]:offsets[i + 1]].tolist() == want, i
    assert keep[offsets[-3]:offsets[-2]].tolist() == [0, 1, 0, 0, 1]


def test_standalone_program_under_sanitizers(tmp_path, cases):
    """tests/native/ua_host.cpp as a program of its own (-DUA_HOST_MAIN) built
    with -fsanitize=address,undefined: the cyclic grid, a hard17 grid, a
    random grid and the three bad grids at 12 cells, no report."""
    exe = str(tmp_path / "ua_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DUA_HOST_MAIN", "-o", exe,
                           os.path.join(native_build.NATIVE, "ua_host.cpp")])
    pick = [cases[0], cases[3], cases[14]] + cases[-3:]
    text = "".join("%s %d\n" % (U.grid_text(c.grid), 12) for c in pick)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(pick)
    for line, c in zip(lines, pick):
        total = sum(c.rows12.values())
        assert line == "%d %d %d %d" % (c.status, total, total, len(c.minimal12)), (c.name, line)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f, sb, fm = L.sdk_unavoidable_batch, L.sdk_unavoidable_scratch_bytes, L.sdk_unavoidable_minimal_batch
    assert _lib.SDK_UA_MAX_SIZE == 16 and _lib.SDK_UA_DONE == 1 and _lib.SDK_UA_NOT_A_GRID == -2
    need = sb(100, 0)
    assert need == 64 + 128 * 100 and sb(100, 7) == need and sb(0, 0) == 64
    assert sb(2 ** 31 - 1, 0) == 64 + 128 * (2 ** 31 - 1)
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(1 << 31, 0) == 0 and sb(2 ** 63 - 1, 0) == 0
    ok = dict(g=16, n=100, m=12, r=16, cap=10, c=16, s=16, i=16, sc=16, nb=need, w=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["g"], a["n"], a["m"], a["r"], a["cap"], a["c"], a["s"], a["i"], a["sc"], a["nb"], a["w"], None)
    assert call(m=3) == -2 and call(m=17) == -2                  # max_size out of range
    assert call(n=-1) == -2 and call(n=1 << 31, nb=1 << 50) == -2  # n negative / above 2^31 - 1
    assert call(cap=-1) == -2 and call(w=-1) == -2               # negative capacity / max_waves
    assert call(nb=need - 1) == -2                               # scratch one byte short
    for name in ("g", "c", "s", "i", "sc", "r"):                 # a required pointer is NULL
        assert call(**{name: None}) == -2, name
    assert call(r=24) == -2 and call(r=24, cap=0) == -2          # d_rows not 16-byte aligned
    assert call(c=18) == -2 and call(s=18) == -2                 # d_count / d_status misaligned
    assert call(i=20) == -2 and call(sc=20) == -2                # d_info / scratch misaligned
    assert f(None, 0, 12, None, 0, None, None, None, None, 0, 0, None) == 0    # n == 0
    assert f(None, 0, 3, None, 0, None, None, None, None, 0, 0, None) == -2    # ... still checks max_size
    assert f(None, 0, 12, None, -1, None, None, None, None, 0, 0, None) == -2
    assert fm(None, None, 0, None, 0, None) == 0                 # groups == 0
    assert fm(None, None, -1, None, 0, None) == -2 and fm(None, None, 0, None, -1, None) == -2
    assert fm(16, 16, 1 << 31, 16, 0, None) == -2
    assert fm(None, 16, 1, 16, 0, None) == -2 and fm(16, None, 1, 16, 0, None) == -2 and fm(16, 16, 1, None, 0, None) == -2
    assert fm(24, 16, 1, 16, 0, None) == -2 and fm(16, 20, 1, 16, 0, None) == -2
