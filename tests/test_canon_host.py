"""CPU checks of the canonical form (csrc/canon.h, what canon_kernel's lanes
and canon_reduce_kernel run): the header compiled for the host
(tests/native/canon_host.cpp, built by native_build.py) against the fixture tests/golden/canon_cases.json
(made by the CPU tool scripts/hard17/hard17_search.c --canon, re-run here),
against an independent numpy brute force for sym and autos, and the C ABI's
argument checks through ctypes (no GPU).  Every check is an equality."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from native_build import host_lib

SYMMETRIES = 3359232


def _arr(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


@pytest.fixture(scope="module")
def cases():
    doc = load_golden("canon_cases.json")["cases"]
    names = [c["name"] for c in doc]
    boards = np.stack([_arr(c["board"]) for c in doc])
    canon = np.stack([_arr(c["canon"]) for c in doc])
    return names, boards, canon


@pytest.fixture(scope="module")
def host():
    return host_lib("canon_host", openmp=True)


def _canon(lib, boards, S=1):
    """(canon, sym, autos) of the host build, each board cut into S slices."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.full_like(boards, 77)
    sym = np.full(len(boards), 12345, dtype=np.int32)
    autos = np.full(len(boards), 12345, dtype=np.int32)
    lib.canon_host_batch(boards.ctypes.data, out.ctypes.data, sym.ctypes.data, autos.ctypes.data, len(boards), S)
    return out, sym, autos


@pytest.fixture(scope="module")
def host_full(host, cases):
    return _canon(host, cases[1])


def test_fixture_is_the_tools_output(cases, tmp_path):
    """The stored canon is what hard17_search --canon prints today, one board
    per invocation; and the set is what the fixture claims."""
    sys.path.insert(0, GOLDEN)
    import make_canon_cases as M
    names, boards, canon = cases
    exe = M.build_tool(str(tmp_path))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        got = list(ex.map(lambda b: M.tool_canon(exe, M.text(b)), boards))
    assert got == [M.text(c) for c in canon]
    by = dict(zip(names, got))
    assert by["empty"] == "0" * 81 and by["one_clue"] == "0" * 80 + "1"
    assert by["pair_a"] == by["pair_b"] and by["pair_a"] != by["hard_search_0"]
    made = M.boards()  # the generator still makes these boards
    assert [n for n, _ in made] == names and np.array_equal(np.stack([b for _, b in made]), boards)
    assert sum(n.startswith("grid_") or n == "cyclic_grid" for n in names) == 8
    assert sum(n.startswith("puzzle_") for n in names) == 16
    clues = (boards[[n.startswith("puzzle_") for n in names]] > 0).sum(1)
    assert clues.min() >= 24 and clues.max() <= 40


def test_host_canon_matches_fixture(host_full, cases):
    _, boards, canon = cases
    got, sym, autos = host_full
    assert np.array_equal(got, canon)
    assert (sym >= 0).all() and (sym < SYMMETRIES).all() and (autos >= 1).all()


def test_corpus_lines_are_fixed_points(host):
    """data/hard17_classes.txt is "one class per line, minlex form"."""
    from sudoku_solver_distributed_amd.gen import hard17_classes
    classes = np.stack([_arr(s) for s in hard17_classes()])
    assert len(classes) == 80
    got, _, _ = _canon(host, classes)
    assert np.array_equal(got, classes)


SLICE_BOARDS = ("empty", "cyclic_grid", "one_clue", "two_clues_box", "grid_1", "grid_2", "puzzle_24", "puzzle_33",
                "random_bytes_0", "hard_search_0", "pair_a", "pair_b")


@pytest.mark.parametrize("S", [2, 7, 18, 2592])
def test_slices_never_change_results(host, host_full, cases, S):
    names, boards, _ = cases
    sel = [names.index(n) for n in SLICE_BOARDS]
    got = _canon(host, boards[sel], S)
    for g, w in zip(got, host_full):
        assert np.array_equal(g, w[sel])


def test_slice_records_cover_disjoint_symmetries(host, cases):
    """The records of 7 slices: each sym lies in its own slice's range, and
    the ties of the slices that hold the smallest image add up to autos."""
    names, boards, _ = cases
    for name in ("empty", "one_clue"):
        b = np.ascontiguousarray(boards[names.index(name)])
        recs = []
        for s in range(7):
            lo, hi = s * 2592 // 7, (s + 1) * 2592 // 7
            w = np.zeros(16, dtype=np.uint32)
            host.canon_host_slice(b.ctypes.data, lo, hi, w.ctypes.data)
            assert w[13] == 0 and lo * 1296 <= w[11] < hi * 1296
            recs.append((tuple(int(x) for x in w[:11]), int(w[12])))
        ties = sum(t for img, t in recs if img == min(recs)[0])
        assert ties == (SYMMETRIES if name == "empty" else 41472)


def test_invalid_byte_is_reported(host, cases):
    _, boards, _ = cases
    b = boards[[5, 6, 7]].copy()
    b[1, 80] = 10
    got, sym, autos = _canon(host, b, 3)
    assert np.array_equal(got[1], b[1]) and sym[1] == -1 and autos[1] == -1
    assert (sym[[0, 2]] >= 0).all()


# ---- sym and autos against a brute force written here, from the definition

PERM3 = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _perm(p):
    bp, inner = p // 216, ((p // 36) % 6, (p // 6) % 6, p % 6)
    return [3 * PERM3[bp][k // 3] + PERM3[inner[k // 3]][k % 3] for k in range(9)]


def _brute(board):
    """(canon, sym, autos): loop over the 2592 row variants, the 1296 column
    permutations vectorised; digits relabelled by their first position."""
    g = board.reshape(9, 9).astype(np.int64)
    cols = np.array([_perm(p) for p in range(1296)])
    weights = 16 ** np.arange(8, -1, -1, dtype=np.int64)
    best, best_sym, ties = None, -1, 0
    for rv in range(2592):
        t, R = rv // 1296, _perm(rv % 1296)
        src = g.T if t else g
        img = src[R][:, cols].transpose(1, 0, 2).reshape(1296, 81)  # img[ci, 9 i + j] = src[R[i], C[j]]
        first = np.stack([np.where((img == x).any(1), (img == x).argmax(1), 99) for x in range(10)], axis=1)
        rank = 1 + (first[:, None, 1:] < first[:, 1:, None]).sum(2)
        maps = np.zeros((1296, 10), dtype=np.int64)
        maps[:, 1:] = np.where(first[:, 1:] < 99, rank, 0)
        rel = np.take_along_axis(maps, img, axis=1)
        keys = rel.reshape(1296, 9, 9) @ weights  # one number per image row
        order = np.lexsort(keys.T[::-1])
        k0 = tuple(keys[order[0]])
        if best is not None and k0 > best:
            continue
        same = np.nonzero((keys == keys[order[0]]).all(1))[0]
        if best is None or k0 < best:
            best, best_img, ties, best_sym = k0, rel[order[0]].copy(), 0, rv * 1296 + int(same.min())
        ties += len(same)
    return best_img.astype(np.uint8), best_sym, ties


BRUTE_BOARDS = ("empty", "one_clue", "pair_b", "puzzle_30", "cyclic_grid")


@pytest.fixture(scope="module")
def brute(cases):
    """The brute force of the five boards, side by side (about 10 s each)."""
    from concurrent.futures import ProcessPoolExecutor
    names, boards, _ = cases
    with ProcessPoolExecutor(len(BRUTE_BOARDS)) as ex:
        return dict(zip(BRUTE_BOARDS, ex.map(_brute, [boards[names.index(n)] for n in BRUTE_BOARDS])))


@pytest.mark.parametrize("name", BRUTE_BOARDS)
def test_sym_and_autos_match_brute_force(host_full, cases, brute, name):
    names, boards, canon = cases
    i = names.index(name)
    want, sym, autos = brute[name]
    assert np.array_equal(want, canon[i])
    assert (int(host_full[1][i]), int(host_full[2][i])) == (sym, autos)
    if name == "empty":
        assert (sym, autos) == (0, SYMMETRIES)
    if name == "one_clue":
        assert autos == SYMMETRIES // 81 == 41472  # the group is transitive on the cells


def test_apply_symmetry_restates_the_definition(host_full, cases):
    from sudoku_solver_distributed_amd.gen import apply_symmetry, line_perms
    _, boards, canon = cases
    assert np.array_equal(line_perms(), np.array([_perm(p) for p in range(1296)]))
    img, maps = apply_symmetry(boards, host_full[1])
    assert np.array_equal(img, canon)
    # the digit maps: 0 -> 0, the digits present onto 1..k
    for b, m in zip(boards, maps):
        present = sorted(set(b.tolist()) - {0})
        assert m[0] == 0 and sorted(m[present].tolist()) == list(range(1, len(present) + 1))
        assert all(m[x] == 0 for x in range(1, 10) if x not in present)
    # sym 0 is the identity up to relabelling; one sym for all boards
    img0, _ = apply_symmetry(boards[6:8], 0)
    assert np.array_equal(img0 > 0, boards[6:8] > 0)
    with pytest.raises(ValueError):
        apply_symmetry(boards[:1], SYMMETRIES)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_canonical_batch, L.sdk_canonical_scratch_bytes
    need = sb(100, 7)
    assert need == 100 * 7 * 64
    assert f(16, 32, 16, None, 100, -1, 16, need, None) == -2     # slices -1
    assert f(16, 32, 16, None, 100, 2593, 16, need, None) == -2   # slices past SDK_CANON_MAX_SLICES
    assert f(16, 32, 16, None, -1, 7, 16, need, None) == -2       # negative n
    assert f(None, 32, 16, None, 100, 7, 16, need, None) == -2    # a required pointer is NULL
    assert f(16, None, 16, None, 100, 7, 16, need, None) == -2
    assert f(16, 32, None, None, 100, 7, 16, need, None) == -2
    assert f(16, 32, 16, None, 100, 7, None, need, None) == -2
    assert f(16, 32, 16, None, 100, 7, 16, need - 1, None) == -2  # scratch one byte short
    assert f(16, 16, 16, None, 100, 7, 16, need, None) == -2      # d_canon aliases d_boards
    need0 = sb(100, 0)                                            # auto slices: sized by the same rule
    assert need0 >= 100 * 64 and need0 % (100 * 64) == 0
    assert f(16, 32, 16, None, 100, 0, 16, need0 - 1, None) == -2
    assert f(None, None, None, None, 0, 0, None, 0, None) == 0    # n == 0
    assert f(None, None, None, None, 0, 2593, None, 0, None) == -2  # ... still checks slices
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(1, 2593) == 0 and sb(0, 0) == 0
    assert sb(1, 2592) == 2592 * 64 and sb(1 << 20, 1) == (1 << 20) * 64
    from sudoku_solver_distributed_amd import _lib
    assert _lib.SDK_CANON_SYMMETRIES == SYMMETRIES and _lib.SDK_CANON_MAX_SLICES == 2592
