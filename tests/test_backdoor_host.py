"""CPU checks of the backdoor search (csrc/backdoor.h, what the backdoor
kernels run): the fixture tests/golden/backdoor_cases.json itself -- written by
rate_host_batch alone over every subset of the empty cells -- against the
figures DESIGN.md §23 lists; the header compiled for the host
(tests/native/backdoor_host.cpp) against the fixture on every case and output;
the unranking against itertools; the plain-Python definition of
backdoor_cases.py live at sizes 0 and 1; and the C ABI's argument checks
through ctypes (no GPU).  Every check is an equality."""
import ctypes
import os
import subprocess
from collections import Counter
from itertools import combinations
from math import comb

import numpy as np
import pytest

import backdoor_cases as BC
import native_build

_vp, _i64, _int, _u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
native_build.PROTOS.setdefault("backdoor_host", {
    # boards, grids, size, count (NULL ok), first (NULL ok), cover (NULL ok), n, level, max_size
    "backdoor_host_batch": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int], None),
    "backdoor_host_choose": ([_u32, _int], _u32),
    "backdoor_host_unrank": ([_u32, _int, _u32, _vp], None),
})

RUNS = [(1, 3), (2, 3), (3, 3), (2, 1), (1, 4)]


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("backdoor_host", openmp=True)


@pytest.fixture(scope="module")
def fixture():
    return BC.load_fixture()


def run_host(lib, boards, grids, level, max_size, count=True, first=True, cover=True):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    grids = np.ascontiguousarray(grids, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    s = np.full(n, 12345, dtype=np.int32)
    c = np.full(n, 12345, dtype=np.int32) if count else None
    f = np.full((n, 4), 77, dtype=np.uint8) if first else None
    v = np.full((n, 81), 77, dtype=np.uint8) if cover else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    lib.backdoor_host_batch(boards.ctypes.data, grids.ctypes.data, s.ctypes.data, ptr(c), ptr(f), ptr(v), n, level, max_size)
    return s, c, f, v


def test_fixture_is_what_the_design_lists(fixture):
    """The recorded answers themselves: the corpora's tallies per level, the
    named triples, no run answered max_size + 1 on more boards than listed,
    and every size 0..4 and both negative codes present."""
    names, _, _, runs = fixture
    assert set(runs) == set(RUNS)

    def tally(prefix, key):
        idx, size = runs[key][0], runs[key][1]
        return dict(Counter(int(s) for i, s in zip(idx, size) if names[i].startswith(prefix)))
    assert tally("class_", (1, 3)) == {3: 31, 4: 49}
    assert tally("class_", (2, 3)) == {0: 34, 1: 44, 2: 2}
    assert tally("class_", (3, 3)) == {0: 54, 1: 26}
    assert tally("seed_", (1, 3)) == {1: 4, 2: 31, 3: 5}
    assert tally("seed_", (2, 3)) == {1: 40}
    assert tally("seed_", (3, 3)) == {0: 8, 1: 32}
    assert tally("puzzles_30_", (1, 3)) == {0: 12}

    def triple(name, key):
        idx, size, count, first, _ = runs[key]
        (k,) = [k for k, i in enumerate(idx) if names[i] == name]
        return int(size[k]), int(count[k]), tuple(int(v) for v in first[k] if v != 255)
    assert triple("proper_undecided", (1, 3)) == (3, 12, (3, 23, 73))
    assert triple("proper_undecided", (2, 3)) == (3, 566, (1, 3, 66))
    assert triple("proper_undecided", (3, 3)) == (3, 862, (1, 3, 66))
    assert triple("class_2", (1, 4)) == (4, 27, (0, 3, 28, 41))
    assert triple("class_3", (1, 4)) == (4, 95, (0, 27, 35, 70))
    assert triple("class_4", (1, 4)) == (4, 4, (5, 9, 47, 59))
    assert triple("class_5", (1, 4)) == (4, 34, (0, 15, 28, 48))
    assert triple("empty", (1, 4)) == (5, 0, ()) and triple("full_grid", (1, 3)) == (0, 1, ())
    for name in ("given_changed", "grid_row_repeat"):
        assert triple(name, (2, 3)) == (BC.MISMATCH, 0, ())
    for name in ("board_byte_10", "grid_byte_0"):
        assert triple(name, (2, 3)) == (BC.INVALID, 0, ())
    # the two completions of one board have backdoors of their own
    a, b = triple("undecided_trials_removed_a", (2, 3)), triple("undecided_trials_removed_b", (2, 3))
    assert a[0] >= 1 and b[0] >= 1
    seen = set()
    for (level, max_size), (idx, size, count, first, cover) in runs.items():
        seen |= {int(s) for s in size}
        assert (size <= max_size + 1).all()
        none = size == max_size + 1
        # answered max_size + 1: no more of the corpora's boards than the tables give the run
        corpus = np.array([names[i].startswith(("class_", "seed_")) for i in idx])
        allowed = {(1, 3): 49, (2, 3): 0, (3, 3): 0, (2, 1): 2, (1, 4): 0}[(level, max_size)]
        assert int((none & corpus).sum()) <= allowed, (level, max_size)
        solved = size >= 1
        used = (first != 255).sum(1)
        assert (used[solved & ~none] == size[solved & ~none]).all() and (used[~solved | none] == 0).all()
        assert (count[none | (size < 0)] == 0).all() and (count[size == 0] == 1).all()
        assert (cover[none | (size <= 0)] == 0).all()
        for k in np.nonzero(solved & ~none)[0]:
            f = first[k][:size[k]]
            assert (np.diff(f.astype(int)) > 0).all() and cover[k][f].all()
            assert size[k] <= cover[k].sum() <= size[k] * count[k]
    assert seen == {BC.MISMATCH, BC.INVALID, 0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("level,max_size", RUNS)
def test_host_matches_fixture(host, fixture, level, max_size):
    names, boards, grids, runs = fixture
    idx, size, count, first, cover = runs[(level, max_size)]
    s, c, f, v = run_host(host, boards[idx], grids[idx], level, max_size)
    bad = np.nonzero((s != size) | (c != count) | (f != first).any(1) | (v != cover).any(1))[0]
    assert len(bad) == 0, [(names[idx[k]], int(s[k]), int(size[k]), int(c[k]), int(count[k]), f[k].tolist()) for k in bad[:8]]
    only, c0, f0, v0 = run_host(host, boards[idx], grids[idx], level, max_size, count=False, first=False, cover=False)
    assert np.array_equal(only, size) and c0 is None and f0 is None and v0 is None


def test_size_does_not_grow_with_the_level(fixture):
    _, _, _, runs = fixture
    (i1, s1, *_), (i2, s2, *_), (i3, s3, *_) = runs[(1, 3)], runs[(2, 3)], runs[(3, 3)]
    assert np.array_equal(i1, i2) and np.array_equal(i2, i3)
    ok = s1 >= 0
    assert (s2[ok] <= s1[ok]).all() and (s3[ok] <= s2[ok]).all() and np.array_equal(s1[~ok], s3[~ok])


def unrank(lib, n, j, r):
    out = np.zeros(4, dtype=np.uint8)
    lib.backdoor_host_unrank(n, j, r, out.ctypes.data)
    return tuple(int(v) for v in out[:j]), out[j:].tolist()


def test_choose_and_unranking(host):
    """C(n, j) for every n <= 81, j <= 4; the subset of the first rank, the
    last rank and the ranks either side of every multiple of 64 up to 256, by
    the closed form of the lexicographic order; every rank for n <= 12 against
    itertools.combinations."""
    for n in range(82):
        for j in range(5):
            assert host.backdoor_host_choose(n, j) == comb(n, j), (n, j)

    def nth(n, j, r):  # the definition: skip whole blocks of subsets by their first element
        out, x = [], 0
        for left in range(j, 0, -1):
            while comb(n - 1 - x, left - 1) <= r:
                r -= comb(n - 1 - x, left - 1)
                x += 1
            out.append(x)
            x += 1
        return tuple(out)
    for n in range(1, 82):
        for j in range(1, 5):
            total = comb(n, j)
            ranks = {0, total - 1} | {m + d for m in (64, 128, 192, 256) for d in (-1, 0, 1)}
            for r in sorted(r for r in ranks if 0 <= r < total):
                got, rest = unrank(host, n, j, r)
                assert got == nth(n, j, r) and rest == [255] * (4 - j), (n, j, r)
    for n in range(1, 13):
        for j in range(1, min(n, 4) + 1):
            for r, want in enumerate(combinations(range(n), j)):
                assert unrank(host, n, j, r)[0] == want, (n, j, r)
    assert unrank(host, 81, 4, comb(81, 4) - 1)[0] == (77, 78, 79, 80)


def test_python_definition_at_sizes_0_and_1(host, fixture):
    """Eight boards, level 2 at max_size 1, by backdoor_cases.backdoors (every
    one of the 81 cells tried, givens included) against the host build."""
    names, boards, grids, _ = fixture
    pick = ["class_0", "class_1", "class_2", "seed_0", "seed_1", "proper_undecided", "full_grid", "given_changed"]
    sel = [names.index(n) for n in pick]
    s, c, f, v = run_host(host, boards[sel], grids[sel], 2, 1)
    sizes = set()
    for k, i in enumerate(sel):
        want = BC.backdoors(boards[i], grids[i], 2, 1)
        assert (int(s[k]), int(c[k]), f[k].tolist(), v[k].tolist()) == want, names[i]
        sizes.add(want[0])
    assert sizes == {BC.MISMATCH, 0, 1, 2}


def test_standalone_program_under_sanitizers(tmp_path, fixture):
    """tests/native/backdoor_host.cpp as a program of its own
    (-DBACKDOOR_HOST_MAIN) built with -fsanitize=address,undefined: a case of
    every size and code at level 2, no report."""
    names, boards, grids, runs = fixture
    idx, size, count, first, cover = runs[(2, 3)]
    exe = str(tmp_path / "backdoor_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DBACKDOOR_HOST_MAIN", "-o", exe,
                           os.path.join(native_build.NATIVE, "backdoor_host.cpp")])
    sel = [int(np.nonzero(size == s)[0][0]) for s in sorted(set(int(v) for v in size)) if s != BC.INVALID]
    text = "".join("%s %s 2 3\n" % ("".join(str(int(v)) for v in boards[idx[k]]), "".join(str(int(v)) for v in grids[idx[k]]))
                   for k in sel)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(sel)
    for line, k in zip(lines, sel):
        want = "%d %d %s %d" % (size[k], count[k], ",".join(str(int(v)) for v in first[k]), cover[k].sum())
        assert line == want, (names[idx[k]], line, want)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f, sb = L.sdk_backdoor_batch, L.sdk_backdoor_scratch_bytes
    assert _lib.SDK_BACKDOOR_MAX_SIZE == 4 and _lib.SDK_BACKDOOR_MISMATCH == -2 and _lib.SDK_BACKDOOR_MAX_LEVEL == 3
    need = sb(100, 3, 0)
    assert need == 256 + 320 * 100 and sb(100, 1, 7) == need and sb(0, 4, 0) == 256
    assert sb(2 ** 31 - 1, 4, 0) == 256 + 320 * (2 ** 31 - 1)
    assert sb(-1, 3, 0) == 0 and sb(1, 0, 0) == 0 and sb(1, 5, 0) == 0 and sb(1, 3, -1) == 0 and sb(1 << 31, 3, 0) == 0
    assert sb(2 ** 63 - 1, 3, 0) == 0
    ok = dict(b=16, g=16, s=16, c=None, fi=None, co=None, n=100, level=2, size=3, sc=16, nb=need, w=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["b"], a["g"], a["s"], a["c"], a["fi"], a["co"], a["n"], a["level"], a["size"], a["sc"], a["nb"], a["w"], None)
    assert call(level=0) == -2 and call(level=4) == -2       # level out of range
    assert call(size=0) == -2 and call(size=5) == -2         # max_size out of range
    assert call(n=-1) == -2                                  # negative n
    assert call(n=1 << 31, nb=1 << 50) == -2                 # n above 2^31 - 1
    assert call(w=-1) == -2                                  # negative max_waves
    assert call(nb=need - 1) == -2                           # scratch one byte short
    assert call(b=None) == -2 and call(g=None) == -2         # a required pointer is NULL
    assert call(s=None) == -2 and call(sc=None) == -2
    assert call(s=18) == -2 and call(c=18) == -2             # d_size / d_count / scratch misaligned
    assert call(sc=20) == -2
    assert f(None, None, None, None, None, None, 0, 2, 3, None, 0, 0, None) == 0   # n == 0
    assert f(None, None, None, None, None, None, 0, 0, 3, None, 0, 0, None) == -2  # ... still checks the level
    assert f(None, None, None, None, None, None, 0, 2, 5, None, 0, 0, None) == -2
