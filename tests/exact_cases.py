"""What the exact-count tests share (test_exact_host.py and
test_exact_props_host.py on the CPU, test_gpu_exact.py and
test_gpu_exact_props.py on the GPU): the host model's entry
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


# ---- what the property tests share (test_exact_props_host.py, test_gpu_exact_props.py)
MANY = 1 << 20  # a round budget no case comes near
# "tiny": the tiny-list knobs confined to two waves, so that lanes donate and park
TINY = dict(slice=8, max_tasks=64, max_waves=2, max_rounds=MANY)
native_build.PROTOS["exact_host"]["exact_ring_sweep"] = ([ctypes.c_uint64, _int, _u32, _u32], _i64)
# 3(a): H1 alone on one wave; 3(b): set b among light boards on two waves -- chosen on the host model
# (test_exact_props_host.py asserts what they are there for)
H1_BUDGET = dict(slice=32, max_rounds=8, max_waves=1)
MIX_BUDGET = dict(slice=8192, max_rounds=24, max_waves=2)
SYM_BUDGET, SYM_TINY_BUDGET = 12_000_000, 1_500_000  # completions of a symmetry launch, boards and images
SYM_IMAGES, SYM_SEED = 3, 20270
H2_CELLS = (3, 17, 40)  # of H2's empty cells, in cell order
PLACE_BOARDS = 16       # boards of set d whose every placement is counted


def pass_bound(slice, max_rounds, max_waves, **_):
    """More passes than a call can run (fewer than slice +
    RUN_MAX a lane and round), so more completions than it can count."""
    return max_rounds * (slice + RUN_MAX) * 64 * max_waves


def host_knobs(slice, max_rounds=MANY, max_waves=1, max_tasks=0):
    """count_exact's keywords as host_exact's."""
    return dict(slice=slice, max_rounds=max_rounds, waves=max_waves, max_tasks=max_tasks)


@functools.lru_cache(maxsize=None)
def pool_sets():
    """The set (b..f) of every board of pool()."""
    s = C.sets()
    out = np.array([key for key in "bcdef" for g in s[key] if g.any()])
    assert len(out) == len(pool()[0])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def light(k, sets="cdef"):
    """Pool indices of k boards of `sets` with valid bytes and at most 1022
    completions (the capped count knows them too), the first k of one seeded
    order."""
    _, count, status = pool()
    ok = np.nonzero(np.isin(pool_sets(), list(sets)) & (count <= 1022) & (status == DONE))[0]
    idx = np.random.default_rng(77).permutation(ok)[:k]
    assert len(idx) == k
    idx.setflags(write=False)
    return idx


def check_bounds(count, status, want, want_status=None):
    """What the contract says of every board whatever the budget: DONE =>
    the exact count, PARTIAL => a lower bound, INVALID where expected, nothing
    else.  Returns the PARTIAL mask."""
    count, status, want = np.asarray(count), np.asarray(status), np.asarray(want)
    invalid = np.zeros(len(want), dtype=bool) if want_status is None else np.asarray(want_status) == INVALID
    assert np.array_equal(status == INVALID, invalid)
    done, part = status == DONE, status == PARTIAL
    assert (done | part | invalid).all(), sorted(set(status.tolist()))
    bad = np.nonzero((done & (count != want)) | (part & ((count < 0) | (count > want))) | (invalid & (count != 0)))[0]
    assert len(bad) == 0, [(int(i), int(count[i]), int(want[i]), int(status[i])) for i in bad[:10]]
    return part


@functools.lru_cache(maxsize=None)
def budget_mix():
    """3(b): set b's 256 boards shuffled with 64 boards of sets c and d:
    (boards, want, is_b), read-only."""
    boards, count, _ = pool()
    idx = np.concatenate([np.nonzero(pool_sets() == "b")[0], light(64, "cd")])
    idx = np.random.default_rng(31).permutation(idx)
    out = (np.ascontiguousarray(boards[idx]), count[idx].copy(), pool_sets()[idx] == "b")
    for v in out:
        v.setflags(write=False)
    return out


def with_clue(board, cells):
    """The 9 ** len(cells) boards `board` plus a digit in each of `cells`,
    digits ascending, the last cell's fastest."""
    out = np.repeat(np.asarray(board, dtype=np.uint8)[None], 9 ** len(cells), axis=0)
    for k, c in enumerate(cells):
        out[:, c] = 1 + (np.arange(len(out)) // 9 ** (len(cells) - 1 - k)) % 9
    return out


def clue_clashes(board, cell, d):
    """Does digit d in `cell` repeat a given of the cell's row, column or box?"""
    g = np.asarray(board).reshape(9, 9)
    r, c = divmod(int(cell), 9)
    return bool(d in g[r] or d in g[:, c] or d in g[r - r % 3:r - r % 3 + 3, c - c % 3:c - c % 3 + 3])


@functools.lru_cache(maxsize=None)
def symmetry_selection(budget):
    """Pool indices of a symmetry launch: all of sets c-f, and before them, in
    pool order, the boards of set b for as long as the launch's completions --
    every board counted SYM_IMAGES + 1 times, from the fixture's and the
    oracle's counts alone -- stay within `budget`.  (The pool starts with set
    b, which holds 34.85 of its 34.87 million completions: the light sets are
    paid for first, or no budget would ever reach them.)"""
    _, count, _ = pool()
    is_b = pool_sets() == "b"
    per = (SYM_IMAGES + 1) * count
    room = budget - int(per[~is_b].sum())
    take = np.cumsum(per[is_b]) <= room
    k = int(take.sum()) if take.all() else int(np.argmin(take))
    idx = np.concatenate([np.nonzero(is_b)[0][:k], np.nonzero(~is_b)[0]])
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def symmetry_rows(budget):
    """The boards of symmetry_selection(budget) and their seeded images in
    one shuffled order: (boards (m, 81), source (m,): the pool index of every
    row, syms: row -> (src, pi) for the image rows), read-only.  A board with
    a byte > 9 has no image."""
    import symmetry_cases as S
    boards = pool()[0]
    rng = np.random.default_rng(SYM_SEED)
    rows, source, syms = [], [], []
    for i in symmetry_selection(budget):
        rows.append(boards[i])
        source.append(i)
        syms.append(None)
        if (boards[i] > 9).any():
            continue
        for _ in range(SYM_IMAGES):
            s = S.random_symmetry(rng)
            rows.append(S.image_board(boards[i], s))
            source.append(i)
            syms.append(s)
    order = rng.permutation(len(rows))
    out = np.ascontiguousarray(np.stack(rows)[order]), np.array(source)[order]
    for v in out:
        v.setflags(write=False)
    return out + ({int(r): syms[k] for r, k in enumerate(order) if syms[k] is not None},)


@functools.lru_cache(maxsize=None)
def placements():
    """Item 6's boards: of set d, the 12 with the fewest completions from 2
    up (where a clue that leaves exactly one is common: a board with dozens of
    completions has next to none) and the first 4 in pool order with 24..64,
    and every board "one of them plus (c, d)" for its empty cells c and
    d = 1..9: (pool indices (16,), children (m, 81), parent (m,): position in
    those 16, cell (m,), digit (m,)), read-only."""
    boards, count, _ = pool()
    d = np.nonzero(pool_sets() == "d")[0]
    few = d[count[d] >= 2]
    few = few[np.argsort(count[few], kind="stable")][:PLACE_BOARDS - 4]
    sel = np.concatenate([few, d[(count[d] >= 24) & (count[d] <= 64)][:4]])
    assert len(sel) == PLACE_BOARDS == len(set(sel.tolist()))
    kids, parent, cell, digit = [], [], [], []
    for k, i in enumerate(sel):
        for c in np.nonzero(boards[i] == 0)[0]:
            kids.append(with_clue(boards[i], (int(c),)))
            parent += [k] * 9
            cell += [int(c)] * 9
            digit += list(range(1, 10))
    out = (sel, np.ascontiguousarray(np.concatenate(kids)), np.array(parent), np.array(cell), np.array(digit))
    for v in out:
        v.setflags(write=False)
    return out


def check_placements(child, once, marks, own):
    """Item 6's identities on placements(): child (m,) the children's exact
    counts, once / marks (16, 81) the boards' unique_candidates, own (16,)
    their exact counts.  Returns (placements with one completion, with
    several)."""
    _, _, parent, cell, digit = placements()
    child = np.asarray(child, dtype=np.int64)
    bit = lambda a: (np.asarray(a).astype(np.int64)[parent, cell] >> (digit - 1)) & 1
    assert np.array_equal(child > 0, bit(marks) == 1)
    assert np.array_equal(child == 1, bit(once) == 1)
    sums = np.zeros((PLACE_BOARDS, 81), dtype=np.int64)
    np.add.at(sums, (parent, cell), child)
    filled = np.zeros((PLACE_BOARDS, 81), dtype=bool)
    filled[parent, cell] = True
    assert np.array_equal(sums[filled], np.broadcast_to(np.asarray(own)[:, None], sums.shape)[filled])
    return int((child == 1).sum()), int((child >= 2).sum())


def placed(n, heavy_board, at, idx):
    """An n-board batch of the pool's boards `idx` with `heavy_board` at the
    positions `at` (negative: from the end): (boards, pool index or -1)."""
    boards = pool()[0]
    at = sorted(a % n for a in at)
    src = np.full(n, -1, dtype=np.int64)
    src[np.setdiff1d(np.arange(n), at)] = idx[:n - len(at)]
    out = np.where((src >= 0)[:, None], boards[np.maximum(src, 0)], np.asarray(heavy_board)[None])
    return np.ascontiguousarray(out, dtype=np.uint8), src
