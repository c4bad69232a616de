"""CPU checks of the unique candidates (csrc/plane_uniq.h, what uniq_kernel's
lanes run): the header compiled for the host (tests/native/uniq_host.cpp)
against the fixture tests/golden/uniq_cases.json (the oracle's counter asked
once per cell and digit, to two); that nothing depends on the schedule of the
searches; the stack-depth fault; the boards answered without a search; and the
C ABI's argument checks through ctypes (no GPU).  Every check is an equality."""
import ctypes

import numpy as np
import pytest

import cand_cases as K
import native_build
import uniq_cases as U

_vp = ctypes.c_void_p
# in, once, marks (NULL ok), count (NULL ok), n, max_depth, sweep (0: as compiled), stats (NULL ok),
# passes per board (NULL ok)
native_build.PROTOS.setdefault("uniq_host", {
    "uniq_host_batch": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp], None)})

COMPILED_DEPTH = 81  # plane::COUNT_MAX_DEPTH
WAVE_BYTES = 64 * 85 * 128


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("uniq_host")


@pytest.fixture(scope="module")
def fixture():
    return U.load_fixture()


def uniq(lib, boards, marks=True, count=True, max_depth=COMPILED_DEPTH, sweep=0, stats=None, passes=False):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    o = np.full((n, 81), 0xFFFF, dtype=np.uint16)
    m = np.full((n, 81), 0xFFFF, dtype=np.uint16) if marks else None
    c = np.full(n, 12345, dtype=np.int32) if count else None
    st = (ctypes.c_uint64 * 5)()
    per = np.zeros(n, dtype=np.uint64)
    lib.uniq_host_batch(boards.ctypes.data, o.ctypes.data, m.ctypes.data if marks else None,
                        c.ctypes.data if count else None, n, max_depth, sweep, st, per.ctypes.data)
    if stats is not None:
        stats.update(passes=st[0], sweep_passes=st[1], searches=st[2], deepest=st[3], worst=st[4])
    return (o, m, c, per) if passes else (o, m, c)


def test_fixture_is_the_candidates_fixture_with_once(fixture):
    """The recorded answers themselves: cand_cases.json's boards, marks and
    counts in its order; once inside marks; a given's own bit and a unique
    board's every bit exactly where the count is 1; and bits that are really
    compared: set, and clear inside the marks, on the boards with several
    completions."""
    names, boards, once, marks, count = fixture
    cn, cb, cm, cc = K.load_fixture()
    assert names == cn and np.array_equal(boards, cb) and np.array_equal(marks, cm) and np.array_equal(count, cc)
    assert not (once & ~marks).any()
    for k, n in enumerate(names):
        if count[k] == 1:
            assert np.array_equal(once[k], marks[k]), n
        elif count[k] == 2:
            given = boards[k] != 0
            assert not once[k][given].any(), n
        else:
            assert not once[k].any(), n
    several = count == 2
    assert (once[several] != 0).any(1).sum() >= 64 and ((marks & ~once)[several] != 0).any(1).all()
    at = names.index("f_empty")
    assert not once[at].any() and (marks[at] == K.ALL).all()
    assert sum(n.startswith("b_") for n in names) >= 8


def test_host_matches_fixture(host, fixture):
    names, boards, once, marks, count = fixture
    stats = {}
    o, m, c, per = uniq(host, boards, stats=stats, passes=True)
    bad = np.nonzero((o != once).any(1) | (m != marks).any(1) | (c != count))[0]
    assert len(bad) == 0, [(names[i], int(c[i]), int(count[i])) for i in bad[:8]]
    only, none_m, none_c = uniq(host, boards, marks=False, count=False)  # d_marks = d_count = NULL: the same once
    assert np.array_equal(only, once) and none_m is None and none_c is None
    print("passes/board", stats["passes"] / len(boards), "in the sweep", stats["sweep_passes"] / len(boards),
          "searches/board", stats["searches"] / len(boards), "deepest stack level", stats["deepest"],
          "most passes", stats["worst"], names[int(per.argmax())])
    assert 0 < stats["deepest"] < COMPILED_DEPTH
    assert stats["searches"] > 0 and 0 < stats["sweep_passes"] < stats["passes"]
    # the cost condition of the fixture (uniq_cases.py): no board over the budget
    assert int(per.max()) == stats["worst"] <= U.PASS_BUDGET


@pytest.mark.parametrize("defines", [("SDK_UNIQ_SWEEP=2",), ("SDK_UNIQ_SWEEP=4096",), ("SDK_UNIQ_DESCEND=1",),
                                     ("SDK_UNIQ_SWEEP=2", "SDK_UNIQ_DESCEND=1")])
def test_schedule_of_the_searches_does_not_matter(fixture, defines):
    """The sweep's cap at 2 and at 4096 completions, and the targets taken
    from the highest open bit down: the fixture's arrays and counts."""
    _, boards, once, marks, count = fixture
    stats = {}
    o, m, c = uniq(native_build.host_lib("uniq_host", defines=defines), boards, stats=stats)
    assert np.array_equal(o, once) and np.array_equal(m, marks) and np.array_equal(c, count)
    assert stats["searches"] > 0  # the targeted phase really ran


def test_small_stack_faults_never_reports_an_answer(host, fixture):
    """max_depth = 2: exactly the boards whose searches go deeper report
    SDK_FAULT (-3) with zero arrays; every other board its answer."""
    names, boards, once, marks, count = fixture
    deep = np.zeros(len(boards), dtype=bool)
    for k in range(len(boards)):
        st = {}
        uniq(host, boards[k], stats=st)
        deep[k] = st["deepest"] > 2
    o, m, c = uniq(host, boards, max_depth=2)
    assert deep.sum() > 20 and (~deep).sum() > 20
    assert (c[deep] == K.FAULT).all() and not o[deep].any() and not m[deep].any()
    assert np.array_equal(c[~deep], count[~deep]) and np.array_equal(o[~deep], once[~deep])
    assert np.array_equal(m[~deep], marks[~deep])


def test_boards_answered_without_a_search(host, fixture):
    names, boards, _, _, _ = fixture
    sel = [names.index(n) for n in ("f_full_one_cell_changed", "f_clash_with_open_cells", "f_byte_10")]
    o, m, c = uniq(host, boards[sel])
    assert not o.any() and not m.any() and c.tolist() == [0, 0, K.INVALID]


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_unique_candidates_batch, L.sdk_unique_candidates_scratch_bytes
    need = sb(100, 2)
    assert need == 256 + 2 * WAVE_BYTES
    assert f(16, None, 16, 16, 100, 16, need, 2, None) == -2       # d_once is NULL
    assert f(16, 16, 16, 16, -1, 16, need, 2, None) == -2          # negative n
    assert f(16, 16, 16, 16, 100, 16, need, -1, None) == -2        # negative max_waves
    assert f(16, 17, 16, 16, 100, 16, need, 2, None) == -2         # d_once at an odd address
    assert f(16, 16, 17, 16, 100, 16, need, 2, None) == -2         # d_marks at an odd address
    assert f(16, 16, 16, 18, 100, 16, need, 2, None) == -2         # d_count at 2 mod 4
    assert f(16, 16, 16, 16, 100, 20, need, 2, None) == -2         # the scratch at 4 mod 8
    assert f(16, 16, 16, 16, 100, 16, need - 1, 2, None) == -2     # scratch one byte short
    assert f(None, 16, 16, 16, 100, 16, need, 2, None) == -2       # the other required pointers
    assert f(16, 16, 16, 16, 100, None, need, 2, None) == -2
    assert f(None, None, None, None, 0, None, 0, 0, None) == 0     # n == 0
    assert f(None, None, None, None, 0, None, 0, -1, None) == -2   # ... still checks max_waves


def test_scratch_bytes_shape(L):
    sb = L.sdk_unique_candidates_scratch_bytes
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(-1, -1) == 0
    assert sb(0, 4) == 256
    assert sb(1, 4) == sb(64, 4) == 256 + WAVE_BYTES               # whole waves
    assert [sb(1 << 20, w) - sb(1 << 20, w - 1) for w in (2, 3, 17)] == [WAVE_BYTES] * 3
    assert sb(65, 4) - sb(64, 4) == WAVE_BYTES and sb(1 << 20, 4) == sb(257, 4) == 256 + 4 * WAVE_BYTES
