"""What the random-completion tests share (test_sample_host.py on the CPU,
test_gpu_sample.py on the GPU): the choice rule of include/sudoku_hip.h
restated in Python, the host model's entries (tests/native/sample_host.cpp),
and the fixture tests/golden/sample_cases.json, which
tests/golden/make_sample_cases.py records from the host model in its default
build.  Loaded once per process and shared, never modified.
"""
import ctypes
import functools
import json
import os

import numpy as np

import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sample_cases.json")
INVALID = -1  # SDK_INVALID
FAULT = -3    # SDK_FAULT
LEVELS = 81   # plane::COUNT_MAX_DEPTH: a lane's stack lines
WAVE_BYTES = 64 * LEVELS * 128
M64 = (1 << 64) - 1
# group -> (boards of count_cases.sets() or None for NULL boards, rows of them, per_board, first_key); one seed
# for all, so that rows of different groups can share one call.  The key ranges overlap on purpose: a call that
# mixes the groups puts a row where its key falls.
SEED = 1
GROUPS = {"z": (None, 64, 1, 0), "a": ("a", 32, 1, 3), "b": ("b", 32, 1, 16), "d": ("d", 32, 4, 40),
          "e": ("e", 8, 1, 5), "f": ("f", 5, 1, 7)}
F_STATUS = (1, 1, 0, 0, INVALID)

_vp, _u64, _u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
native_build.PROTOS.setdefault("sample_host", {
    # in (NULL: empty boards), out, status, n, per_board, seed, first_key, max_depth, passes, deepest, draws (NULL ok)
    "sample_host_batch": ([_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _u64, _u64, _u32, _vp, _vp, _vp], None),
    "sample_host_pick": ([_u32, _u64, _u64, _u32], _u32)})  # mask, seed, key, t -> digit bit


def mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def pick(mask, seed, key, t):
    """The rule's choose(mask) for draw t of item (seed, key): the digit bit."""
    h = mix((mix(seed & M64) + key) & M64)
    r = mix((h + (t + 1) * 0x9E3779B97F4A7C15) & M64)
    index = ((r >> 32) * bin(mask).count("1")) >> 32
    bits = [1 << k for k in range(9) if (mask >> k) & 1]
    return bits[index]


def host_sample(lib, boards, seed=0, per_board=1, first_key=0, n=None, max_depth=LEVELS, stats=None):
    """The host model's answer: (out (items, 81) uint8, status (items,) int32).
    boards None: n empty boards, passed as NULL.  stats: a dict that receives
    the per-item arrays passes, deepest and draws."""
    if boards is not None:
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
        n = len(boards)
    items = n * per_board
    out = np.full((items, 81), 0xEE, dtype=np.uint8)
    status = np.full(items, 12345, dtype=np.int32)
    passes = np.zeros(items, dtype=np.uint64)
    deepest, draws = np.zeros(items, dtype=np.uint32), np.zeros(items, dtype=np.uint32)
    lib.sample_host_batch(None if boards is None else boards.ctypes.data, out.ctypes.data, status.ctypes.data, n,
                          per_board, seed & M64, first_key & M64, max_depth, passes.ctypes.data, deepest.ctypes.data,
                          draws.ctypes.data)
    if stats is not None:
        stats.update(passes=passes, deepest=deepest, draws=draws)
    return out, status


def board_text(board):
    """81 values as 81 hex digits (a byte of 10 is 'a')."""
    return "".join("%x" % int(v) for v in board)


def board_from_text(s):
    return np.array([int(ch, 16) for ch in s], dtype=np.uint8)


def group_boards(name):
    """The input boards of a fixture group (None for the NULL-board group)."""
    import count_cases as C
    src, rows, _, _ = GROUPS[name]
    return None if src is None else C.sets()[src][:rows]


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/sample_cases.json: group -> {"seed", "first_key",
    "per_board", "boards" (k, 81) uint8 (zeros for the NULL-board group),
    "null" (bool), "out" (k * per_board, 81) uint8, "status" (k * per_board,)
    int32}, read-only arrays."""
    with open(FIXTURE) as f:
        doc = json.load(f)["groups"]
    fx = {}
    for name, g in doc.items():
        out = np.array([board_from_text(s) for s in g["out"]], dtype=np.uint8)
        null = g["boards"] is None
        boards = (np.zeros((len(out) // g["per_board"], 81), dtype=np.uint8) if null else
                  np.array([board_from_text(s) for s in g["boards"]], dtype=np.uint8))
        status = np.array(g["status"], dtype=np.int32)
        for v in (out, boards, status):
            v.setflags(write=False)
        fx[name] = {"seed": int(g["seed"]), "first_key": int(g["first_key"]), "per_board": int(g["per_board"]),
                    "boards": boards, "null": null, "out": out, "status": status}
    return fx


@functools.lru_cache(maxsize=None)
def rows():
    """The fixture row by row: a dict of names (list), board (r, 81), key
    (r,) int64, out (r, 81), status (r,), key_free (r,) bool -- True where the
    row's answer is the same under every key (one completion, none, or a byte
    > 9), so that the row may stand anywhere in a call."""
    fx = load_fixture()
    names, board, key, out, status, free = [], [], [], [], [], []
    for name, g in fx.items():
        for q in range(len(g["out"])):
            names.append(f"{name}_{q}")
            board.append(g["boards"][q // g["per_board"]])
            key.append(g["first_key"] + q)
            out.append(g["out"][q])
            status.append(g["status"][q])
            free.append(name in ("a", "e") or (name == "f" and q >= 1))
    r = {"names": names, "board": np.array(board, dtype=np.uint8), "key": np.array(key, dtype=np.int64),
         "out": np.array(out, dtype=np.uint8), "status": np.array(status, dtype=np.int32), "key_free": np.array(free)}
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def mixed_call(n, turn, seed):
    """Fixture row numbers for the n items of one call at first_key 0 and
    per_board 1: item j, whose key is j, takes candidate (turn + j) % 3 of the
    key-bound rows that have key j (z, b, d and f's empty board: at most three
    a key), and where there is none a key-free row (a, e, the rest of f) from a
    seeded shuffle that goes through all of them before one repeats.  Over
    turns 0, 1, 2 every key-bound row with a key below n is taken once."""
    r = rows()
    rng = np.random.default_rng(seed)
    free = np.nonzero(r["key_free"])[0]
    cycle = np.concatenate([rng.permutation(free) for _ in range(-(-n // len(free)))])
    bound = {}
    for i in np.nonzero(~r["key_free"])[0]:
        bound.setdefault(int(r["key"][i]), []).append(int(i))
    assert max(len(v) for v in bound.values()) <= 3
    idx, used = [], 0
    for j in range(n):
        cand = bound.get(j, [])
        k = (turn + j) % 3
        if k < len(cand):
            idx.append(cand[k])
        else:
            idx.append(int(cycle[used]))
            used += 1
    return np.array(idx, dtype=np.int64)
