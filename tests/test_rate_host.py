"""CPU checks of the puzzle rating (csrc/rate.h, what rate_kernel's lanes and
rate_trial_kernel's trials run): the header compiled for the host
(tests/native/rate_host.cpp) against the fixture tests/golden/rate_cases.json
and, live, against the plain-Python definition of rate_cases.py; that nothing
depends on the schedule of the rules or on a symmetry of the board; and the C
ABI's argument checks through ctypes (no GPU).  Every check is an equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import native_build
import rate_cases as R

_vp = ctypes.c_void_p
# in, rating, open (NULL ok), marks (NULL ok), n, max_level
native_build.PROTOS.setdefault("rate_host", {"rate_host_batch": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int], None)})


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("rate_host")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def rate(lib, boards, max_level=4, opens=True, marks=True):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    r = np.full(n, 12345, dtype=np.int32)
    o = np.full((n, 4), 12345, dtype=np.int32) if opens else None
    m = np.full((n, 81), 0xFFFF, dtype=np.uint16) if marks else None
    lib.rate_host_batch(boards.ctypes.data, r.ctypes.data, o.ctypes.data if opens else None,
                        m.ctypes.data if marks else None, n, max_level)
    return r, o, m


def spread(rating, per=7):
    """Indices of up to `per` fixture boards of every rating 0..5."""
    return np.concatenate([np.nonzero(rating == k)[0][:per] for k in range(6)])


def test_fixture_is_what_the_design_lists(fixture):
    """The recorded answers themselves: the named boards, the corpora's
    tallies, and a dead state first seen at every level."""
    names, _, rating, opens, marks = fixture
    at = {n: k for k, n in enumerate(names)}
    for name, (_, want, want_open) in R.NAMED.items():
        assert rating[at[name]] == want and opens[at[name]].tolist() == want_open, name
    tally = lambda prefix: {int(k): int(v) for k, v in zip(*np.unique(
        [rating[i] for n, i in at.items() if n.startswith(prefix)], return_counts=True))}
    assert tally("class_") == {2: 34, 3: 20, 4: 26}
    assert tally("seed_") == {3: 34, 4: 222}
    assert tally("puzzles_30_") == {1: 48, 5: 12}
    assert opens[at["class_0"]].tolist() == [63, 0, 0, 0] and opens[at["seed_0"]].tolist() == [57, 54, 54, 0]
    for level in (1, 2, 3, 4):
        o = opens[at[f"mutation_dead_at_level_{level}"]].tolist()
        assert o[level - 1:] == [-1] * (5 - level) and all(v > 0 for v in o[:level - 1])
    solved = (rating >= 1) & (rating <= 4)
    assert (marks[rating == 0] == 0).all()
    assert (np.bitwise_and(marks[solved], marks[solved] - 1) == 0).all() and (marks[solved] != 0).all()
    assert {int(v) for v in rating} == {0, 1, 2, 3, 4, 5}


def test_host_matches_fixture_at_level_4(host, fixture):
    names, boards, rating, opens, marks = fixture
    r, o, m = rate(host, boards, 4)
    bad = np.nonzero((r != rating) | (o != opens).any(1) | (m != marks).any(1))[0]
    assert len(bad) == 0, [(names[i], int(r[i]), int(rating[i]), o[i].tolist(), opens[i].tolist()) for i in bad[:8]]
    only, none_o, none_m = rate(host, boards, 4, opens=False, marks=False)  # both optional outputs NULL
    assert np.array_equal(only, rating) and none_o is None and none_m is None


@pytest.mark.parametrize("max_level", [1, 2, 3])
def test_lower_levels_follow_the_definition(host, fixture, max_level):
    """rating, open and SDK_RATE_NOT_RUN at max_level m, derived from the
    level-4 answers; the marks where the level-4 answer holds them (a board
    solved or dead by level m), and the count of cells they leave open
    everywhere."""
    names, boards, rating, opens, marks = fixture
    r, o, m = rate(host, boards, max_level)
    for i in range(len(boards)):
        want_r, want_o, marks_known = R.at_level(rating[i], opens[i], max_level)
        assert (int(r[i]), o[i].tolist()) == (want_r, want_o), names[i]
        if marks_known:
            assert np.array_equal(m[i], marks[i]), names[i]
        else:
            assert want_r == max_level + 1
            assert int((np.bitwise_and(m[i], m[i] - 1) != 0).sum()) == want_o[max_level - 1], names[i]
    assert (o[:, max_level:] == R.NOT_RUN).all()


def test_host_matches_the_python_definition_live(host, fixture):
    """About 40 boards over all ratings, every max_level, marks included,
    against rate_cases.rate run now."""
    _, boards, rating, _, _ = fixture
    sel = spread(rating)
    assert len(sel) >= 36
    for max_level in (1, 2, 3, 4):
        r, o, m = rate(host, boards[sel], max_level)
        for k, i in enumerate(sel):
            want = R.rate(boards[i], max_level)
            assert (int(r[k]), o[k].tolist(), m[k].tolist()) == want, (int(i), max_level)


def test_schedule_of_the_rules_does_not_matter(fixture):
    """The digits, cells and trials in descending order, a sweep's trials all
    on the sweep's first state: identical outputs on every fixture board."""
    _, boards, _, _, _ = fixture
    a = native_build.host_lib("rate_host")
    b = native_build.host_lib("rate_host", defines=("SDK_RATE_DESCEND=1",))
    for max_level in (1, 2, 3, 4):
        for x, y in zip(rate(a, boards, max_level), rate(b, boards, max_level)):
            assert np.array_equal(x, y), max_level


def test_symmetry_images_keep_rating_and_open(host, fixture):
    """Relabelled, permuted and transposed images of 16 boards over all
    ratings: the same rating and open counts, and as many candidates."""
    from sudoku_solver_distributed_amd.gen import _symmetry_images
    _, boards, rating, opens, marks = fixture
    sel = spread(rating, per=3)[:16]
    assert len(sel) == 16
    for k, i in enumerate(sel):
        images = _symmetry_images(boards[i:i + 1], 6, seed=300 + k)
        r, o, m = rate(host, images, 4)
        assert (r == rating[i]).all() and (o == opens[i]).all(), int(i)
        count = lambda a: int(np.unpackbits(a.view(np.uint8)).sum())
        assert all(count(m[j]) == count(marks[i]) for j in range(len(images)))


def test_bytes_above_9_are_invalid(host, fixture):
    _, boards, rating, opens, marks = fixture
    b = boards[:12].copy()
    b[1, 0], b[3, 80], b[5, 40], b[7, 17] = 10, 255, 16, 12
    hit = [1, 3, 5, 7]
    for max_level in (1, 4):
        r, o, m = rate(host, b, max_level)
        assert (r[hit] == R.INVALID).all() and (o[hit] == R.INVALID).all() and (m[hit] == 0).all()
    rest = [k for k in range(12) if k not in hit]
    assert np.array_equal(r[rest], rating[rest]) and np.array_equal(o[rest], opens[rest])
    assert np.array_equal(m[rest], marks[rest])


def test_standalone_program_under_sanitizers(tmp_path, fixture):
    """tests/native/rate_host.cpp as a program of its own (-DRATE_HOST_MAIN)
    built with -fsanitize=address,undefined: a board of every rating through
    every max_level, no report."""
    names, boards, rating, opens, _ = fixture
    exe = str(tmp_path / "rate_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-DRATE_HOST_MAIN", "-o", exe, os.path.join(native_build.NATIVE, "rate_host.cpp")])
    sel = spread(rating, per=1)
    text = "".join("".join(str(int(v)) for v in boards[i]) + "\n" for i in sel)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(sel)
    for line, i in zip(lines, sel):
        o = opens[i].tolist()
        assert line.split()[-4:] == [f"4:{rating[i]}[{o[0]}", str(o[1]), str(o[2]), f"{o[3]}]"], (names[i], line)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f, sb = L.sdk_rate_batch, L.sdk_rate_scratch_bytes
    assert _lib.SDK_RATE_MAX_LEVEL == 4 and _lib.SDK_RATE_NOT_RUN == -2
    need = sb(100, 4)
    assert need == 256 + 8 * 100 and sb(100, 3) == sb(100, 1) == 256 and sb(0, 4) == 256
    assert sb(-1, 4) == 0 and sb(1, 0) == 0 and sb(1, 5) == 0 and sb(1 << 31, 4) == 0
    assert f(16, 16, None, None, 100, 0, 16, need, None) == -2       # max_level 0
    assert f(16, 16, None, None, 100, 5, 16, need, None) == -2       # max_level past SDK_RATE_MAX_LEVEL
    assert f(16, 16, None, None, -1, 4, 16, need, None) == -2        # negative n
    assert f(16, 16, None, None, 1 << 31, 4, 16, 1 << 40, None) == -2  # n above 2^31 - 1
    assert f(16, 16, None, None, 100, 4, 16, need - 1, None) == -2   # scratch one byte short
    assert f(16, 16, None, None, 100, 3, 16, 255, None) == -2
    assert f(None, 16, None, None, 100, 4, 16, need, None) == -2     # a required pointer is NULL
    assert f(16, None, None, None, 100, 4, 16, need, None) == -2
    assert f(16, 16, None, None, 100, 4, None, need, None) == -2
    assert f(16, 16, None, 17, 100, 4, 16, need, None) == -2         # d_marks at an odd address
    assert f(16, 18, None, None, 100, 4, 16, need, None) == -2       # d_rating / d_open / scratch misaligned
    assert f(16, 16, 18, None, 100, 4, 16, need, None) == -2
    assert f(16, 16, None, None, 100, 4, 20, need, None) == -2
    assert f(None, None, None, None, 0, 4, None, 0, None) == 0       # n == 0
    assert f(None, None, None, None, 0, 0, None, 0, None) == -2      # ... still checks max_level
