"""CPU checks of the random completion (csrc/plane_sample.h, what
sample_kernel's lanes run): the header compiled for the host
(tests/native/sample_host.cpp) against the choice rule restated here in Python
(sample_cases.pick), against the fixture tests/golden/sample_cases.json, and
against the oracle for everything the oracle can say about a row; the key
semantics; the empty board; the stack-depth fault; and the C ABI's argument
checks through ctypes (no GPU)."""
import random

import numpy as np
import pytest

import count_cases as C
import native_build
import sample_cases as S
from oracle import oracle as O

# set d boards that the oracle counts at 2..6 completions and on which keys
# 0..255 under seed 1 reach every completion (test_reach)
REACH = (1, 2, 3, 8, 9, 10, 11, 29)


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("sample_host")


@pytest.fixture(scope="module")
def fx():
    return S.load_fixture()


# ---- 1. the choice rule

def test_pick_equals_the_rule_restated(host):
    rng = random.Random(17)
    tuples = [(1 << k, rng.getrandbits(64), rng.getrandbits(64), t) for k in range(9) for t in (0, 1, 80)]
    tuples += [(0x1FF, rng.getrandbits(64), rng.getrandbits(64), rng.randrange(200)) for _ in range(100)]
    tuples += [(rng.randrange(1, 512), rng.getrandbits(64), rng.getrandbits(64), rng.randrange(5000)) for _ in range(300)]
    tuples += [(m, s, k, t) for m in (0x1FF, 0x101, 0x003) for s in (0, 1, S.M64) for k in (0, 1, S.M64)
               for t in (0, 1, 0xFFFFFFFE)]
    for mask, seed, key, t in tuples:
        got = host.sample_host_pick(mask, seed, key, t)
        assert got == S.pick(mask, seed, key, t), (hex(mask), seed, key, t)
        assert got & mask == got and bin(got).count("1") == 1


def test_pick_is_even_over_keys(host):
    """Keys 0..4607, mask 0x1FF, t = 0: 512 expected per digit, sigma =
    sqrt(4608 * 1/9 * 8/9) = 21.3, band 512 +- 6 sigma = [384, 640]."""
    for seed in (0, 1):
        counts = np.bincount([host.sample_host_pick(0x1FF, seed, key, 0).bit_length() - 1 for key in range(4608)],
                             minlength=9)
        print("seed", seed, "digit counts", counts.tolist())
        assert counts.sum() == 4608 and counts.min() >= 384 and counts.max() <= 640


# ---- 2. the fixture

def test_fixture_is_what_the_issue_lists(fx):
    assert {k: (len(g["out"]), g["per_board"], g["null"]) for k, g in fx.items()} == {
        "z": (64, 1, True), "a": (32, 1, False), "b": (32, 1, False), "d": (128, 4, False), "e": (8, 1, False),
        "f": (5, 1, False)}
    for name, (_, rows, per_board, first_key) in S.GROUPS.items():
        g = fx[name]
        assert (g["seed"], g["first_key"], g["per_board"], len(g["boards"])) == (S.SEED, first_key, per_board, rows)
        if not g["null"]:
            assert np.array_equal(g["boards"], S.group_boards(name)), name
    assert fx["z"]["first_key"] == 0 and not fx["z"]["boards"].any()
    assert tuple(fx["f"]["status"]) == S.F_STATUS
    assert not fx["e"]["status"].any() and np.array_equal(fx["e"]["out"], fx["e"]["boards"])
    assert all((fx[k]["status"] == 1).all() for k in "zabd")


@pytest.mark.skipif(bool(native_build.HOST_FLAGS), reason="SDK_HOST_CFLAGS selects a rule variant: other grids")
def test_host_matches_fixture(host, fx):
    for name, g in fx.items():
        out, status = S.host_sample(host, None if g["null"] else g["boards"], g["seed"], g["per_board"], g["first_key"],
                                    n=len(g["boards"]))
        assert np.array_equal(status, g["status"]), name
        assert np.array_equal(out, g["out"]), name


# ---- 3. what the oracle says about every row

def test_properties_against_the_oracle(host):
    boards, fixed, uniq, is_unique, _ = C.pool()
    has = C.expected(1) == 1  # O.count_solutions(board, 1) on clean givens, 0 / -1 otherwise
    per_board = 3
    for seed in (1, 2026):
        out, status = S.host_sample(host, boards, seed, per_board, first_key=11)
        assert len(out) == per_board * len(boards)
        for q in range(len(out)):
            i = q // per_board
            if has[i]:
                assert status[q] == 1, (seed, q)
                assert O.check(out[q]) and (out[q][boards[i] != 0] == boards[i][boards[i] != 0]).all(), (seed, q)
                if is_unique[i]:
                    assert np.array_equal(out[q], uniq[i]), (seed, q)
            else:
                assert status[q] == (S.INVALID if fixed[i] == -1 else 0), (seed, q)
                assert np.array_equal(out[q], boards[i]), (seed, q)


# ---- 4. every completion can come out

def completions(board):
    """Every completion of a board, from the oracle alone: its counter says
    whether there are none, one (solve_unique_batch shows it) or more; then
    the first empty cell is fixed to each digit in turn."""
    n = O.count_solutions(board, 2)
    if n == 0:
        return []
    if n == 1:
        return [O.solve_unique_batch(board[None])[0][0]]
    cell = int(np.nonzero(board == 0)[0][0])
    out = []
    for v in range(1, 10):
        if O.is_valid(board, cell // 9, cell % 9, v):
            trial = board.copy()
            trial[cell] = v
            out += completions(trial)
    return out


def test_reach(host):
    d = C.sets()["d"]
    for i in REACH:
        want = {g.tobytes() for g in completions(d[i].copy())}
        assert 2 <= len(want) <= 6 and len(want) == O.count_solutions(d[i], 7), i
        out, status = S.host_sample(host, d[i], S.SEED, per_board=256)
        assert (status == 1).all()
        got = {g.tobytes() for g in out}
        assert got == want, (i, len(got), len(want))  # each at least once, and nothing else


# ---- 5. keys and seeds

def test_key_semantics(host):
    b = C.sets()["b"][:24]
    for per_board in (1, 3):
        whole, st = S.host_sample(host, b, 5, per_board, first_key=1000)
        for k in (1, 7, 23):
            tail, st2 = S.host_sample(host, b[k:], 5, per_board, first_key=1000 + k * per_board)
            assert np.array_equal(tail, whole[k * per_board:]) and np.array_equal(st2, st[k * per_board:])
    other, _ = S.host_sample(host, b, 6, 1, first_key=1000)
    one, _ = S.host_sample(host, b, 5, 1, first_key=1000)
    assert (other != one).any(1).sum() >= 1
    # keys wrap mod 2^64, and NULL boards are the empty board
    hi, _ = S.host_sample(host, None, 5, 1, first_key=S.M64, n=2)
    lo, _ = S.host_sample(host, np.zeros((1, 81), np.uint8), 5, 1, first_key=0)
    assert np.array_equal(hi[1], lo[0])


# ---- 6. the empty board

def test_empty_board_keys_0_to_4607(host):
    st = {}
    out, status = S.host_sample(host, None, S.SEED, 1, 0, n=4608, stats=st)
    assert (status == 1).all() and all(O.check(g) for g in out)
    assert len({g.tobytes() for g in out}) == 4608
    seen = np.zeros((81, 10), dtype=bool)
    seen[np.arange(81)[None, :], out] = True
    assert seen[:, 1:].all() and not seen[:, 0].any()
    print("empty board, 4608 keys: passes per grid mean %.2f max %d, deepest level %d, draws mean %.2f max %d"
          % (st["passes"].mean(), st["passes"].max(), st["deepest"].max(), st["draws"].mean(), st["draws"].max()))
    assert 0 < st["deepest"].max() <= S.LEVELS


# ---- 7. the depth fault

def test_small_stack_faults_with_the_input_back(host):
    b = C.sets()["b"][:16]
    st = {}
    full, status = S.host_sample(host, b, 3, 2, stats=st)
    assert (status == 1).all()
    out, status2 = S.host_sample(host, b, 3, 2, max_depth=2)
    deep = st["deepest"] > 2
    assert deep.sum() >= 8
    for q in range(len(out)):
        if deep[q]:
            assert status2[q] == S.FAULT and np.array_equal(out[q], b[q // 2]), q
        else:
            assert status2[q] == 1 and np.array_equal(out[q], full[q]), q
    out, status = S.host_sample(host, None, 3, 1, n=4, max_depth=2)  # NULL boards: the empty board back
    assert (status == S.FAULT).all() and not out.any()


# ---- 8. the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_sample_batch, L.sdk_sample_scratch_bytes
    need = sb(300, 2)
    assert need == 256 + 2 * S.WAVE_BYTES
    # d_boards, d_out, d_status, n, per_board, seed, first_key, d_scratch, scratch_bytes, max_waves, stream
    assert f(16, 8192, 64, -1, 3, 0, 0, 128, need, 2, None) == -2      # negative n
    assert f(16, 8192, 64, 100, 3, 0, 0, 128, need, -1, None) == -2    # negative max_waves
    assert f(16, 8192, 64, 100, 0, 0, 0, 128, need, 2, None) == -2     # per_board < 1
    assert f(16, 8192, 64, 100, -2, 0, 0, 128, need, 2, None) == -2
    assert f(16, 8192, 64, 1 << 30, 2, 0, 0, 128, 1 << 40, 2, None) == -2  # 2^31 items
    assert f(16, 8192, 64, 1 << 31, 1, 0, 0, 128, 1 << 40, 2, None) == -2
    assert f(16, 8192, 64, 1 << 40, 1 << 30, 0, 0, 128, 1 << 40, 2, None) == -2  # n * per_board past 2^64
    assert f(16, None, 64, 100, 3, 0, 0, 128, need, 2, None) == -2     # NULL d_out, d_status, scratch
    assert f(16, 8192, None, 100, 3, 0, 0, 128, need, 2, None) == -2
    assert f(16, 8192, 64, 100, 3, 0, 0, None, need, 2, None) == -2
    assert f(16, 8192, 66, 100, 3, 0, 0, 128, need, 2, None) == -2     # d_status misaligned
    assert f(16, 8192, 64, 100, 3, 0, 0, 132, need, 2, None) == -2     # scratch misaligned
    assert f(16, 16, 64, 100, 3, 0, 0, 128, need, 2, None) == -2       # d_out == d_boards
    assert f(16, 8192, 64, 100, 3, 0, 0, 128, need - 1, 2, None) == -2  # scratch one byte short
    assert f(None, 8192, 64, 100, 3, 0, 0, 128, need - 1, 2, None) == -2  # ... with NULL boards too
    assert f(None, None, None, 0, -7, 0, 0, None, 0, -1, None) == 0    # n == 0 before anything else


def test_scratch_bytes_shape(L):
    sb = L.sdk_sample_scratch_bytes
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(-1, -1) == 0
    assert sb(0, 4) == 256
    assert sb(1, 4) == sb(64, 4) == 256 + S.WAVE_BYTES           # whole waves
    assert sb(67, 4) == 256 + 2 * S.WAVE_BYTES
    assert sb(65, 4) - sb(64, 4) == S.WAVE_BYTES and sb(1 << 20, 4) == sb(257, 4) == 256 + 4 * S.WAVE_BYTES
    assert sb((1 << 31) - 1, 3) == 256 + 3 * S.WAVE_BYTES
