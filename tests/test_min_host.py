"""CPU checks of the minimisation (csrc/plane_min.h, what min_kernel's lanes
run): the header compiled for the host (tests/native/min_host.cpp) against the
fixture tests/golden/min_cases.json (the definition as the plain loop over the
oracle's counter); the results' properties straight from the oracle; the
stack-depth fault; and the C ABI's argument checks through ctypes (no GPU).
Every check is an equality, but for the recorded host-model passes."""
import ctypes

import numpy as np
import pytest

import count_cases as C
import min_cases as M
import native_build
from oracle import oracle as O

_vp = ctypes.c_void_p
# in, order (NULL ok), out, status, removed (NULL ok), n, mode, max_empty, max_depth, stats (NULL ok)
native_build.PROTOS.setdefault("min_host", {
    "min_host_batch": ([_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _vp], None)})

COMPILED_DEPTH = 81  # plane::COUNT_MAX_DEPTH
WAVE_BYTES = 64 * M.MIN_LEVELS * 128


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("min_host")


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


def minimize(lib, boards, order=None, mode=M.GREEDY, max_empty=81, removed=True, max_depth=COMPILED_DEPTH, stats=None):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.uint8).reshape(n, 81)
    out = np.full((n, 81), 0xEE, dtype=np.uint8)
    status = np.full(n, 12345, dtype=np.int32)
    rm = np.full(n, 12345, dtype=np.int32) if removed else None
    st = (ctypes.c_uint64 * 3)()
    lib.min_host_batch(boards.ctypes.data, None if order is None else order.ctypes.data, out.ctypes.data,
                       status.ctypes.data, rm.ctypes.data if removed else None, n, mode, max_empty, max_depth, st)
    if stats is not None:
        stats.update(passes=st[0], tests=st[1], deepest=st[2])
    return out, status, rm


def run_case(lib, fx, k, **kw):
    """The host build's answer for fixture case k, its order NULL where the case says so."""
    order = fx["order"][k] if fx["has_order"][k] else None
    return minimize(lib, fx["boards"][k], order, int(fx["mode"][k]), int(fx["max_empty"][k]), **kw)


def test_fixture_is_what_the_issue_lists(fx):
    names, status, removed = fx["names"], fx["status"], fx["removed"]
    at = {n: k for k, n in enumerate(names)}
    assert len(names) == 263 and len(at) == 263
    sizes = {p: sum(n.startswith(p) for n in names) for p in ("g_", "c_", "a_", "h_", "b_", "e_", "f_")}
    assert sizes == {"g_": 50, "c_": 128, "a_": 32, "h_": 32, "b_": 8, "e_": 8, "f_": 5}
    c_greedy = [at[f"c_{i}"] for i in range(64)]
    assert sum(status[k] == 1 for k in c_greedy) >= 32 and sum(status[k] == 2 for k in c_greedy) >= 16
    for k, n in enumerate(names):
        same = np.array_equal(fx["out"][k], fx["boards"][k])
        assert (fx["out"][k] == 0).sum() - (fx["boards"][k] == 0).sum() == removed[k], n
        if status[k] != 1 or n.startswith("a_"):
            assert same and removed[k] == 0, n  # 17-clue puzzles are minimal
        if n.startswith(("g_", "a_", "h_")):
            assert status[k] == 1, n
        if n.startswith("b_"):
            assert status[k] == 2
        if n.startswith("e_"):
            assert status[k] == 0
        if n.endswith("_max40"):
            assert (fx["out"][k] == 0).sum() == 40 and fx["max_empty"][k] == 40
        if n.endswith("_probe"):
            assert fx["mode"][k] == M.PROBE and not fx["has_order"][k]
    assert removed[at["g_0_cell40"]] == 1 and fx["out"][at["g_0_cell40"]][40] == 0
    assert (fx["order"][at["g_1_skip40"]][:40] > 80).all() and removed[at["g_1_skip40"]] > 20
    assert sum(removed[at[f"h_{i}"]] >= 1 for i in range(16)) >= 8
    assert status[at["f_empty"]] == 2 and status[at["f_full"]] == 1 and removed[at["f_full"]] >= 53
    assert status[at["f_full_one_cell_changed"]] == 0 and status[at["f_clash_with_open_cells"]] == 0
    assert status[at["f_byte_10"]] == M.INVALID


def test_host_matches_fixture(host, fx):
    """Case by case (each has its own mode, max_empty and NULL or given order):
    out, status and removed; and the same out and status with removed = NULL."""
    bad = []
    total = {"passes": 0, "tests": 0, "deepest": 0}
    for k, name in enumerate(fx["names"]):
        st = {}
        out, status, rm = run_case(host, fx, k, stats=st)
        if not (np.array_equal(out[0], fx["out"][k]) and status[0] == fx["status"][k] and rm[0] == fx["removed"][k]):
            bad.append((name, int(status[0]), int(fx["status"][k]), int(rm[0]), int(fx["removed"][k])))
        out2, status2, none = run_case(host, fx, k, removed=False)
        assert none is None and np.array_equal(out2, out) and status2[0] == status[0], name
        total = {"passes": total["passes"] + st["passes"], "tests": total["tests"] + st["tests"],
                 "deepest": max(total["deepest"], st["deepest"])}
    assert not bad, bad[:8]
    print("passes/case", total["passes"] / len(fx["names"]), "tests/case", total["tests"] / len(fx["names"]),
          "deepest stack level", total["deepest"])
    assert 0 < total["deepest"] < COMPILED_DEPTH


def test_one_call_many_boards(host, fx):
    """A batch in one call: the greedy cases at max_empty 81 with their orders
    (identity where NULL), and the probe cases."""
    for mode in (M.GREEDY, M.PROBE):
        sel = np.nonzero((fx["mode"] == mode) & (fx["max_empty"] == 81))[0]
        out, status, rm = minimize(host, fx["boards"][sel], fx["order"][sel], mode)
        assert np.array_equal(out, fx["out"][sel]) and np.array_equal(status, fx["status"][sel])
        assert np.array_equal(rm, fx["removed"][sel])


def test_greedy_results_are_minimal_proper_puzzles(host, fx):
    """Independently of the fixture: every status-1 greedy result at max_empty
    81 whose order names every given has one completion, and two once any
    single clue is erased."""
    seen = 0
    for k, name in enumerate(fx["names"]):
        order = fx["order"][k] if fx["has_order"][k] else None
        if fx["mode"][k] != M.GREEDY or fx["max_empty"][k] != 81 or fx["status"][k] != 1:
            continue
        if not M.names_every_given(fx["boards"][k], order):
            continue
        out, status, _ = run_case(host, fx, k)
        assert status[0] == 1 and O.count_solutions(out[0], 2) == 1, name
        for c in np.nonzero(out[0])[0]:
            trial = out[0].copy()
            trial[c] = 0
            assert O.count_solutions(trial, 2) == 2, (name, int(c))
        seen += 1
    assert seen >= 32 + 8 + 32 + 16 + 16  # g, its NULL orders, c's unique boards, a, h


def test_out_differs_from_the_input_by_zeros_only(host, fx):
    for k, name in enumerate(fx["names"]):
        out, _, rm = run_case(host, fx, k)
        changed = out[0] != fx["boards"][k]
        assert not out[0][changed].any() and changed.sum() == rm[0], name


def test_probe_erases_greedys_first_removal(host, fx):
    """Greedy's first removal is a given that is redundant in the input board,
    so probe erases it too."""
    sel = [k for k, n in enumerate(fx["names"]) if fx["mode"][k] == M.GREEDY and fx["removed"][k] > 0]
    assert len(sel) >= 64
    for k in sel:
        order = fx["order"][k]
        greedy, _, _ = run_case(host, fx, k)
        first = next(int(c) for c in order if c <= 80 and fx["boards"][k][c] and not greedy[0][c])
        probe, status, _ = minimize(host, fx["boards"][k], None, M.PROBE)
        assert status[0] == 1 and probe[0][first] == 0, fx["names"][k]


def test_small_stack_faults_with_the_input_back(host, fx):
    """max_depth = 2: a board whose searches go deeper reports SDK_FAULT (-3)
    with out = input and removed = 0, never a partial result; a full grid,
    whose tests need no deeper stack, its normal answer."""
    at = {n: k for k, n in enumerate(fx["names"])}
    faulted = 0
    for name in [f"h_{i}" for i in range(16)] + [f"a_{i}" for i in range(8)] + ["g_0", "g_1", "f_full"]:
        k = at[name]
        st = {}
        run_case(host, fx, k, stats=st)
        out, status, rm = run_case(host, fx, k, max_depth=2)
        if st["deepest"] > 2:
            assert status[0] == M.FAULT and rm[0] == 0 and np.array_equal(out[0], fx["boards"][k]), name
            faulted += 1
        else:
            assert status[0] == fx["status"][k] and rm[0] == fx["removed"][k], name
            assert np.array_equal(out[0], fx["out"][k]), name
    assert faulted >= 8
    out, status, rm = run_case(host, fx, at["g_0_cell40"], max_depth=2)  # one test of a full grid: no search
    assert status[0] == 1 and rm[0] == 1 and np.array_equal(out[0], fx["out"][at["g_0_cell40"]])


def test_host_model_passes_fused_against_81_counts(host, fx):
    """Recorded, not bounded: the fused loop's passes per board on the 32 g
    grids against unique_batch's 81 rounds of the count's host model at limit
    2 on the same grids and orders (profiles/min_rate.json)."""
    count_lib = native_build.host_lib("count_host")
    sel = [k for k, n in enumerate(fx["names"]) if n.startswith("g_") and n[2:].isdigit()]
    assert len(sel) == 32
    st = {}
    out, status, _ = minimize(host, fx["boards"][sel], fx["order"][sel], M.GREEDY, stats=st)
    assert np.array_equal(out, fx["out"][sel])
    rounds = 0
    puzzle = fx["boards"][sel].copy()
    for t in range(81):
        trial = puzzle.copy()
        trial[np.arange(32), fx["order"][sel][:, t]] = 0
        cnt = np.zeros(32, dtype=np.int32)
        passes, deepest = ctypes.c_uint64(0), ctypes.c_uint32(0)
        count_lib.count_host_batch(trial.ctypes.data, cnt.ctypes.data, None, 32, 2, COMPILED_DEPTH,
                                   ctypes.byref(passes), ctypes.byref(deepest))
        rounds += passes.value
        puzzle = np.where((cnt == 1)[:, None], trial, puzzle)
    assert np.array_equal(puzzle, out)  # the loop the fused call replaces gives the same puzzles
    print("host-model passes per board: fused", st["passes"] / 32, "81 counts at limit 2", rounds / 32,
          "ratio", rounds / st["passes"])


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    f, sb = L.sdk_minimize_batch, L.sdk_minimize_scratch_bytes
    need = sb(100, 2)
    assert need == 256 + 2 * WAVE_BYTES
    # d_boards, d_order, d_out, d_status, d_removed, n, mode, max_empty, d_scratch, scratch_bytes, max_waves, stream
    assert f(16, None, 8192, 64, None, 100, 2, 81, 128, need, 2, None) == -2    # a mode out of range
    assert f(16, None, 8192, 64, None, 100, -1, 81, 128, need, 2, None) == -2
    assert f(16, None, 8192, 64, None, 100, 0, -1, 128, need, 2, None) == -2    # max_empty
    assert f(16, None, 8192, 64, None, 100, 0, 82, 128, need, 2, None) == -2
    assert f(16, None, 8192, 64, None, -1, 0, 81, 128, need, 2, None) == -2     # negative n
    assert f(16, None, 8192, 64, None, 100, 0, 81, 128, need, -1, None) == -2   # negative max_waves
    assert f(None, None, 8192, 64, None, 100, 0, 81, 128, need, 2, None) == -2  # NULL d_boards, d_out, d_status
    assert f(16, None, None, 64, None, 100, 0, 81, 128, need, 2, None) == -2
    assert f(16, None, 8192, None, None, 100, 0, 81, 128, need, 2, None) == -2
    assert f(16, None, 8192, 66, None, 100, 0, 81, 128, need, 2, None) == -2    # d_status misaligned
    assert f(16, None, 8192, 64, 66, 100, 0, 81, 128, need, 2, None) == -2      # d_removed misaligned
    assert f(16, None, 8192, 64, None, 100, 0, 81, 132, need, 2, None) == -2    # scratch misaligned
    assert f(16, None, 8192, 64, None, 100, 0, 81, None, need, 2, None) == -2
    assert f(16, None, 8192, 64, None, 100, 0, 81, 128, need - 1, 2, None) == -2  # scratch one byte short
    assert f(16, None, 16, 64, None, 100, 0, 81, 128, need, 2, None) == -2      # d_out == d_boards
    assert f(None, None, None, None, None, 0, 7, -5, None, 0, -1, None) == 0    # n == 0 before anything else


def test_scratch_bytes_shape(L):
    sb = L.sdk_minimize_scratch_bytes
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(-1, -1) == 0
    assert sb(0, 4) == 256
    assert sb(1, 4) == sb(64, 4) == 256 + WAVE_BYTES           # whole waves
    assert sb(67, 4) == 256 + 2 * WAVE_BYTES
    assert sb(65, 4) - sb(64, 4) == WAVE_BYTES and sb(1 << 20, 4) == sb(257, 4) == 256 + 4 * WAVE_BYTES
