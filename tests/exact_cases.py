"""What the exact-count tests share (test_exact_host.py on the CPU,
test_gpu_exact.py on the GPU): the host model's entry
(tests/native/exact_host.cpp), the fixture tests/golden/exact_cases.json
(recorded by tests/golden/make_exact_cases.py from the oracle's counter), the
two heavy boards and the pool of boards with their exact counts.  Built once
per process and shared, never modified.
"""
import ctypes
import functools
import json
import os

import numpy as np

import count_cases as C
import native_build
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "exact_cases.json")
DONE, PARTIAL, INVALID, FAULT = 1, 2, -1, -3  # SDK_EXACT_DONE, SDK_EXACT_PARTIAL, SDK_INVALID, SDK_FAULT
LEVELS = 81    # plane::COUNT_MAX_DEPTH
RUN_MAX = 82   # plane::EXACT_RUN_MAX: DESIGN.md §20's bound on a lane's passes past `slice` in one round
NO_LIMIT = 2 ** 31 - 1
H1_ERASED, H1_COUNT = 62, 885469
H2_ERASED, H2_COUNT = 63, 7299350
# the knobs the tests run: name -> (slice or None for the default, max_tasks); SLICE_DEFAULT is the product's
KNOBS = {"default": (None, 0), "slice1": (1, 0), "tiny-list": (8, 64)}

_vp, _i64, _int, _i32, _u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32
native_build.PROTOS.setdefault("exact_host", {
    # in, count, status, n, waves, slice, max_rounds, max_tasks, max_depth, stats (4 x int64, NULL ok) -> 0 / -2
    "exact_host_batch": ([_vp, _vp, _vp, _i64, _int, _i32, _int, _i64, _u32, _vp], _int)})


def heavy(k):
    """The oracle's solve of the empty board with the cells
    default_rng(1).permutation(81)[:k] erased."""
    ok, full = O.solve(np.zeros(81, dtype=np.uint8))
    assert ok
    g = full.copy()
    g[np.random.default_rng(1).permutation(81)[:k]] = 0
    g.setflags(write=False)
    return g


def host_exact(lib, boards, waves=1, slice=4096, max_rounds=1 << 20, max_tasks=0, max_depth=LEVELS):
    """The host model's answer: (count (n,) int64, status (n,) int32, stats
    dict of rounds, donated, parks, max_passes)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    count = np.full(len(boards), -12345, dtype=np.int64)
    status = np.full(len(boards), 12345, dtype=np.int32)
    st = np.zeros(4, dtype=np.int64)
    rc = lib.exact_host_batch(boards.ctypes.data, count.ctypes.data, status.ctypes.data, len(boards), waves, slice,
                              max_rounds, max_tasks, max_depth, st.ctypes.data)
    assert rc == 0, rc
    return count, status, dict(zip(("rounds", "donated", "parks", "max_passes"), (int(v) for v in st)))


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/exact_cases.json: {"b": (256,) int64 exact counts of
    count_cases.sets()["b"], "h1", "h2": (board (81,) uint8, count)}."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    b = np.array(doc["b"], dtype=np.int64)
    b.setflags(write=False)
    out = {"b": b}
    for key in ("h1", "h2"):
        g = np.array([int(ch) for ch in doc[key]["board"]], dtype=np.uint8)
        g.setflags(write=False)
        out[key] = (g, int(doc[key]["count"]))
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """Sets b-f of count_cases with the empty board left out: (boards (k, 81)
    uint8, count (k,) int64, status (k,) int32), read-only.  b's counts come
    from the fixture (checked against its boards' number), c-f's from the
    oracle, live; a byte > 9 expects count 0 / INVALID, clashing givens 0 /
    DONE."""
    s = C.sets()
    fx = load_fixture()
    assert len(fx["b"]) == len(s["b"])
    boards, count, status = [], [], []
    for key in "bcdef":
        for i, g in enumerate(s[key]):
            if not g.any():
                continue  # the empty board: no exact count to compare with
            boards.append(g)
            if (g > 9).any():
                count.append(0)
                status.append(INVALID)
            else:
                status.append(DONE)
                count.append(int(fx["b"][i]) if key == "b" else
                             0 if C.givens_clash(g) else O.count_solutions(g, NO_LIMIT))
    out = (np.ascontiguousarray(np.stack(boards)), np.array(count, dtype=np.int64), np.array(status, dtype=np.int32))
    for v in out:
        v.setflags(write=False)
    return out


def mixed(n):
    """n boards of the pool, shuffled so that the lanes of a wave diverge
    (every pool board at least once when n allows), and their pool indices --
    test_gpu_count.py's _mixed over this pool."""
    k = len(pool()[0])
    rng = np.random.default_rng(1000 + n)
    idx = np.concatenate([rng.permutation(k), rng.integers(0, k, size=max(0, n - k))])[:n]
    rng.shuffle(idx)
    return np.ascontiguousarray(pool()[0][idx]), idx


def check_path(name, stats):
    """The statistics show that the path a knob setting is there for ran."""
    if name == "slice1":
        assert stats["donated"] > 0 and stats["rounds"] > 1, stats
    if name == "tiny-list":
        assert stats["parks"] > 0 and stats["rounds"] > 1, stats
