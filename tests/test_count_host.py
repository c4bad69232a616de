"""CPU checks of the capped completion count (csrc/plane_count.h, what
count_kernel's lanes run): the header compiled for the host
(tests/native/count_host.cpp, built by native_build.py) against the oracle's counter on the sets of
count_cases.py, and the C ABI's argument checks through ctypes (no GPU)."""
import ctypes

import numpy as np
import pytest

import count_cases as C
from native_build import host_lib

COMPILED_DEPTH = 81  # plane::COUNT_MAX_DEPTH


@pytest.fixture(scope="module")
def host():
    return host_lib("count_host")


def _count(lib, boards, limit, first=True, max_depth=COMPILED_DEPTH, stats=None):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    cnt = np.full(len(boards), 12345, dtype=np.int32)
    out = np.full_like(boards, 77) if first else None
    p, d = ctypes.c_uint64(), ctypes.c_uint32()
    lib.count_host_batch(boards.ctypes.data, cnt.ctypes.data, out.ctypes.data if first else None, len(boards),
                         limit, max_depth, ctypes.byref(p), ctypes.byref(d))
    if stats is not None:
        stats.update(passes=p.value, deepest=d.value)
    return cnt, out


def test_sets_are_what_they_claim():
    """The oracle alone: a unique, b at the limit for every limit <= 64, e
    none, and at limit 64 at least 64 boards of c and d strictly between 1 and
    64, so that exact mid-range counts are really compared."""
    _, _, _, _, names = C.pool()
    for limit in (1, 2, 3, 64):
        w = C.expected(limit)
        assert (w[names == "a"] == 1).all() and (w[names == "e"] == 0).all()
        assert (w[names == "b"] == limit).all()
    w = C.expected(64)
    cd = (names == "c") | (names == "d")
    assert ((w > 1) & (w < 64) & cd).sum() >= 64
    assert list(C.expected(1024)[names == "f"]) == [1024, 1, 0, 0, -1]


@pytest.mark.parametrize("limit", C.LIMITS)
def test_counts_and_first_match_oracle(host, limit):
    boards, _, uniq, is_unique, names = C.pool()
    stats = {}
    cnt, first = _count(host, boards, limit, stats=stats)
    want = C.expected(limit)
    bad = np.nonzero(cnt != want)[0]
    assert len(bad) == 0, [(int(i), names[i], int(cnt[i]), int(want[i])) for i in bad[:10]]
    C.check_first(boards, cnt, first, uniq, is_unique)
    cnt2, _ = _count(host, boards, limit, first=False)  # d_first = NULL: the same counts
    assert np.array_equal(cnt2, cnt)
    print("limit", limit, "passes/board", stats["passes"] / len(boards), "deepest stack level", stats["deepest"])
    assert 0 < stats["deepest"] < COMPILED_DEPTH


def test_small_stack_faults_never_miscounts(host):
    """max_depth = 2: exactly the boards whose search goes deeper report
    SDK_FAULT (-3); every other board its count."""
    boards, _, _, _, names = C.pool()
    sel = np.nonzero((names == "a") | (names == "d") | (names == "f"))[0]
    want = C.expected(2)[sel]
    deep = np.zeros(len(sel), dtype=bool)
    for k, i in enumerate(sel):
        st = {}
        c, _ = _count(host, boards[i], 2, stats=st)
        assert c[0] == want[k]
        deep[k] = st["deepest"] > 2
    cnt, first = _count(host, boards[sel], 2, max_depth=2)
    assert deep.sum() > 20 and (~deep).sum() > 20
    assert (cnt[deep] == -3).all()
    assert np.array_equal(cnt[~deep], want[~deep])
    assert np.array_equal(first[deep], boards[sel][deep])  # no completion shown for a fault


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_count_solutions_batch, L.sdk_count_scratch_bytes
    need = sb(100, 0)
    assert need > 0
    assert f(16, 16, None, 100, 0, 16, need, 0, None) == -2      # limit 0
    assert f(16, 16, None, 100, 1025, 16, need, 0, None) == -2   # limit past SDK_COUNT_MAX_LIMIT
    assert f(16, 16, None, -1, 2, 16, need, 0, None) == -2       # negative n
    assert f(16, 16, None, 100, 2, 16, need, -1, None) == -2     # negative max_waves
    assert f(16, 16, None, 100, 2, 16, need - 1, 0, None) == -2  # scratch one byte short
    assert f(None, 16, None, 100, 2, 16, need, 0, None) == -2    # a required pointer is NULL
    assert f(16, None, None, 100, 2, 16, need, 0, None) == -2
    assert f(16, 16, None, 100, 2, None, need, 0, None) == -2
    assert f(None, None, None, 0, 2, None, 0, 0, None) == 0      # n == 0
    assert f(None, None, None, 0, 0, None, 0, 0, None) == -2     # ... still checks the limit
    from sudoku_solver_distributed_amd import _lib
    assert _lib.SDK_COUNT_MAX_LIMIT == 1024


def test_scratch_bytes_shape(L):
    sb = L.sdk_count_scratch_bytes
    full_lanes = L.sdk_device_cu_count() * 16 * 64  # at most four waves on each of a CU's four SIMDs
    ns = [0, 1, 63, 64, 65, 4096, 4097, 1 << 16, full_lanes - 1, full_lanes, full_lanes + 1, 4 * full_lanes, 1 << 30]
    sizes = [sb(n, 0) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))          # monotone in n
    assert sizes[1] == sizes[2] == sizes[3] < sizes[4]            # whole waves
    assert sizes[-4] == sizes[-3] == sizes[-2] == sizes[-1]       # constant past a full grid
    per_wave = sizes[4] - sizes[3]
    assert per_wave == 64 * 81 * 128                              # 81 lines of 128 bytes per lane
    assert sb(1 << 20, 2) == sizes[0] + 2 * per_wave and sb(1, 2) == sizes[0] + per_wave
    assert sb(-1, 0) == 0 and sb(1, -1) == 0
