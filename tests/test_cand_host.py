"""CPU checks of the exact candidates (csrc/plane_cand.h, what cand_kernel's
lanes run): the header compiled for the host (tests/native/cand_host.cpp)
against the fixture tests/golden/cand_cases.json (the oracle's counter asked
once per cell and digit); that nothing depends on the schedule of the searches
or on a symmetry of the board; the stack-depth fault; and the C ABI's argument
checks through ctypes (no GPU).  Every check is an equality."""
import ctypes

import numpy as np
import pytest

import cand_cases as K
import native_build

_vp = ctypes.c_void_p
# in, marks, count (NULL ok), n, max_depth, sweep (0: as compiled), stats (NULL ok)
native_build.PROTOS.setdefault("cand_host", {
    "cand_host_batch": ([_vp, _vp, _vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, _vp], None)})

COMPILED_DEPTH = 81  # plane::COUNT_MAX_DEPTH
WAVE_BYTES = 64 * 83 * 128


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("cand_host")


@pytest.fixture(scope="module")
def fixture():
    return K.load_fixture()


def cand(lib, boards, count=True, max_depth=COMPILED_DEPTH, sweep=0, stats=None):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    m = np.full((n, 81), 0xFFFF, dtype=np.uint16)
    c = np.full(n, 12345, dtype=np.int32) if count else None
    st = (ctypes.c_uint64 * 3)()
    lib.cand_host_batch(boards.ctypes.data, m.ctypes.data, c.ctypes.data if count else None, n, max_depth, sweep, st)
    if stats is not None:
        stats.update(passes=st[0], searches=st[1], deepest=st[2])
    return m, c


def test_fixture_is_what_the_issue_lists(fixture):
    """The recorded answers themselves: the sets' sizes, a's single bits, e's
    zeros, the single boards, and counts that follow from the marks."""
    names, boards, marks, count = fixture
    sizes = {p: sum(n.startswith(p) for n in names) for p in ("a_", "b_", "c_", "d_", "e_", "f_", "rate5_")}
    assert sizes == {"a_": 32, "b_": 16, "c_": 64, "d_": 64, "e_": 16, "f_": 5, "rate5_": 8}
    at = {n: k for k, n in enumerate(names)}
    for k, n in enumerate(names):
        if n != "f_byte_10":
            assert count[k] == K.count_of(marks[k]), n
            given = boards[k] != 0
            if count[k] > 0:  # a given's own bit
                assert (marks[k][given] == 1 << (boards[k][given].astype(np.int64) - 1)).all(), n
        if n.startswith("a_"):
            assert count[k] == 1
        if n.startswith("b_"):
            assert count[k] == 2
        if n.startswith("e_"):
            assert count[k] == 0 and not marks[k].any()
    assert (marks[at["f_empty"]] == K.ALL).all() and count[at["f_empty"]] == 2
    assert count[at["f_full"]] == 1 and count[at["f_full_one_cell_changed"]] == 0
    assert count[at["f_clash_with_open_cells"]] == 0 and not marks[at["f_clash_with_open_cells"]].any()
    assert count[at["f_byte_10"]] == K.INVALID and not marks[at["f_byte_10"]].any()
    cd = [k for k, n in enumerate(names) if n[:2] in ("c_", "d_")]
    assert sum(count[k] == 2 for k in cd) >= 64  # boards whose ambiguity is really compared


def test_host_matches_fixture(host, fixture):
    names, boards, marks, count = fixture
    stats = {}
    m, c = cand(host, boards, stats=stats)
    bad = np.nonzero((m != marks).any(1) | (c != count))[0]
    assert len(bad) == 0, [(names[i], int(c[i]), int(count[i])) for i in bad[:8]]
    only, none = cand(host, boards, count=False)  # count = NULL: the same marks
    assert np.array_equal(only, marks) and none is None
    print("passes/board", stats["passes"] / len(boards), "searches/board", stats["searches"] / len(boards),
          "deepest stack level", stats["deepest"])
    assert 0 < stats["deepest"] < COMPILED_DEPTH
    heavy = {}
    cand(host, boards[names.index(f"b_{K.HEAVY_B}")], stats=heavy)
    assert heavy["passes"] > 20000  # the board a wave waits for is among the 16 of set b


@pytest.mark.parametrize("defines", [("SDK_CAND_SWEEP=1",), ("SDK_CAND_SWEEP=2",), ("SDK_CAND_SWEEP=64",),
                                     ("SDK_CAND_DESCEND=1",)])
def test_schedule_of_the_searches_does_not_matter(fixture, defines):
    """The sweep's cap at 1, 2 and 64 completions, and the targets taken from
    the highest unwitnessed bit down: the fixture's marks and counts."""
    _, boards, marks, count = fixture
    stats = {}
    m, c = cand(native_build.host_lib("cand_host", defines=defines), boards, stats=stats)
    assert np.array_equal(m, marks) and np.array_equal(c, count)
    assert stats["searches"] > 0  # the targeted phase really ran


def _image(board, marks):
    """One fixed symmetry image of a board and of its marks, in plain numpy:
    transposed, rows 3 and 5 swapped (inside the middle band), the stacks
    permuted (2, 0, 1), digits relabelled by PI."""
    PI = np.array([0, 4, 7, 1, 9, 2, 8, 3, 5, 6])  # digit x -> PI[x]
    cells = np.arange(81).reshape(9, 9).T.copy()   # image (i, j) <- source cell
    cells[[3, 5]] = cells[[5, 3]]
    cells = cells[:, [6, 7, 8, 0, 1, 2, 3, 4, 5]].reshape(81)
    b = PI[board[cells].astype(np.int64)].astype(np.uint8)
    src = marks[cells].astype(np.int64)
    m = np.zeros(81, dtype=np.int64)
    for d in range(1, 10):
        m |= ((src >> (d - 1)) & 1) << (PI[d] - 1)
    return b, m.astype(np.uint16)


def test_symmetry_images_have_the_image_of_the_marks(host, fixture):
    """32 fixture boards with several completions (sets b, c, d and the
    rating-5 boards): the marks of the image are the image of the marks."""
    names, boards, marks, count = fixture
    sel = ([k for k, n in enumerate(names) if n.startswith("b_")][:4] +
           [k for k, n in enumerate(names) if n[:2] in ("c_", "d_") and count[k] == 2][:22] +
           [k for k, n in enumerate(names) if n.startswith("rate5_")][:6])
    assert len(sel) == 32
    images = [_image(boards[k], marks[k]) for k in sel]
    m, c = cand(host, np.stack([b for b, _ in images]))
    assert np.array_equal(m, np.stack([w for _, w in images]))
    assert np.array_equal(c, count[sel])
    assert any((w != marks[k]).any() for (_, w), k in zip(images, sel))  # the image really moves the marks


def test_small_stack_faults_never_reports_marks(host, fixture):
    """max_depth = 2: exactly the boards whose searches go deeper report
    SDK_FAULT (-3) with zero marks; every other board its answer."""
    names, boards, marks, count = fixture
    deep = np.zeros(len(boards), dtype=bool)
    for k in range(len(boards)):
        st = {}
        cand(host, boards[k], stats=st)
        deep[k] = st["deepest"] > 2
    m, c = cand(host, boards, max_depth=2)
    assert deep.sum() > 20 and (~deep).sum() > 20
    assert (c[deep] == K.FAULT).all() and not m[deep].any()
    assert np.array_equal(c[~deep], count[~deep]) and np.array_equal(m[~deep], marks[~deep])


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_candidates_batch, L.sdk_candidates_scratch_bytes
    need = sb(100, 2)
    assert need == 256 + 2 * WAVE_BYTES
    assert f(16, None, 16, 100, 16, need, 2, None) == -2       # d_marks is NULL
    assert f(16, 16, 16, -1, 16, need, 2, None) == -2          # negative n
    assert f(16, 16, 16, 100, 16, need, -1, None) == -2        # negative max_waves
    assert f(16, 17, 16, 100, 16, need, 2, None) == -2         # d_marks at an odd address
    assert f(16, 16, 16, 100, 16, need - 1, 2, None) == -2     # scratch one byte short
    assert f(None, 16, 16, 100, 16, need, 2, None) == -2       # the other required pointers
    assert f(16, 16, 16, 100, None, need, 2, None) == -2
    assert f(None, None, None, 0, None, 0, 0, None) == 0       # n == 0
    assert f(None, None, None, 0, None, 0, -1, None) == -2     # ... still checks max_waves


def test_scratch_bytes_shape(L):
    sb = L.sdk_candidates_scratch_bytes
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(-1, -1) == 0
    assert sb(0, 4) == 256
    assert sb(1, 4) == sb(64, 4) == 256 + WAVE_BYTES           # whole waves
    assert [sb(1 << 20, w) - sb(1 << 20, w - 1) for w in (2, 3, 17)] == [WAVE_BYTES] * 3
    assert sb(65, 4) - sb(64, 4) == WAVE_BYTES and sb(1 << 20, 4) == sb(257, 4) == 256 + 4 * WAVE_BYTES
