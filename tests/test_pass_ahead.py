"""CPU checks of the look-ahead pass (csrc/plane_solver.h: pass_ahead,
search_step_ahead -- what the plane kernel's lane loop runs):
rule A moved from the head of a pass to its tail, so a pass reports DEAD and
STUCK itself instead of leaving it to one more pass.  The header compiled for
the host (tests/native/ahead_host.cpp over csrc/host_model.h): pass by pass
against plane::pass, as a solver against the plane::pass solver and the
oracle, handed over to the wave-wide solver, and for the passes it saves."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, b81
from native_build import host_lib
from oracle import oracle as O

FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"


@pytest.fixture(scope="module")
def ahead():
    return host_lib("ahead_host")


def _solve(lib, boards, ahead, node_order=0, mrv_after=0, max_depth=81, stats=None):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.zeros_like(boards)
    st = np.zeros(len(boards), dtype=np.int32)
    g, p = ctypes.c_uint64(), ctypes.c_uint64()
    lib.ahead_solve_batch(boards.ctypes.data, out.ctypes.data, st.ctypes.data, len(boards), node_order, max_depth,
                          mrv_after, int(ahead), ctypes.byref(g), ctypes.byref(p))
    if stats is not None:
        stats.update(guesses=g.value, passes=p.value)
    return out, st


def _gen_style(n, empties, seed):
    """gen.py-style boards on the CPU: complete grids with cells erased"""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    grids, _ = O.solve_unique_batch(hard17_batch(n, seed=seed).numpy())
    rng = np.random.default_rng(seed)
    for g in grids:
        g[rng.choice(81, empties, replace=False)] = 0
    return grids


@pytest.fixture(scope="module")
def corpus():
    """hard17_batch(1500, seed=31), hard_search_batch(300, seed=32) and their
    unique completions from the oracle, computed once"""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    h17 = hard17_batch(1500, seed=31).numpy()
    hs = hard_search_batch(300, seed=32).numpy()
    boards = np.ascontiguousarray(np.concatenate([h17, hs]))
    want, cnt = O.solve_unique_batch(boards)
    assert (cnt == 1).all()
    return boards, want


def test_pass_ahead_lockstep_with_pass(ahead):
    """From the same planes and nd = single & ~Det, pass_ahead leaves the
    planes plane::pass leaves, returns that pass's verdict upgraded by rule A
    on the result (DEAD on an empty cell, STUCK when no cell became
    determined), and its und' / nd' are what the next plane::pass computes:
    along the searches of hard 17-clue, search-heavy and generated boards, and
    from 200 000 random plane states (ahead_host.cpp ahead_check_pass)."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    boards = np.ascontiguousarray(np.concatenate([hard17_batch(300, seed=11).numpy(),
                                                  hard_search_batch(300, seed=12).numpy(),
                                                  _gen_style(200, 50, 13)]))
    assert ahead.ahead_check_pass(boards.ctypes.data, len(boards), 200_000, 99) == 0


@pytest.mark.parametrize("mrv_after", [0, 64, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
def test_solve_ahead_hard_boards(ahead, corpus, order, mrv_after):
    """The 17-clue and search-heavy boards: plane::solve's and the oracle's
    answers (unique completions: every walk finds them)."""
    boards, want = corpus
    no = int(order == "node")
    got, gst = _solve(ahead, boards, True, node_order=no, mrv_after=mrv_after)
    ref, rst = _solve(ahead, boards, False, node_order=no, mrv_after=mrv_after)
    assert np.array_equal(gst, rst) and np.array_equal(got, ref)
    assert (gst == 1).all() and np.array_equal(got, want)


@pytest.mark.parametrize("mrv_after", [0, 64, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
def test_solve_ahead_random_generated(ahead, order, mrv_after):
    """tests/golden/random_generated.npz: boards with many completions, where
    the answer is the walk's first in the given order."""
    z = np.load(os.path.join(GOLDEN, "random_generated.npz"))
    no = int(order == "node")
    for empties, _n in z["cases"]:
        e = int(empties)
        puzzles = z[f"puzzles_{e}"]
        got, gst = _solve(ahead, puzzles, True, node_order=no, mrv_after=mrv_after)
        ref, rst = _solve(ahead, puzzles, False, node_order=no, mrv_after=mrv_after)
        assert np.array_equal(gst, rst) and np.array_equal(got, ref), e
        mine = gst != 2
        assert np.array_equal(gst[mine], z[f"{order}_status_{e}"][mine]), e
        assert np.array_equal(got[mine], z[f"{order}_solutions_{e}"][mine]), e


@pytest.mark.parametrize("mrv_after", [0, 64, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
def test_solve_ahead_edge_cases(ahead, order, mrv_after):
    no = int(order == "node")
    dup = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
    dead = np.zeros(81, np.uint8)  # cell (8, 8) has no candidate: row 8 holds 2..9, column 8 a 1
    dead[72:80] = [2, 3, 4, 5, 6, 7, 8, 9]
    dead[63 + 8] = 1
    boards = np.array([b81("0" * 81), b81(FULL), b81(FULL[:40] + "0" + FULL[41:]), dead, b81("5" * 81), b81(dup)],
                      dtype=np.uint8)
    got, gst = _solve(ahead, boards, True, node_order=no, mrv_after=mrv_after)
    ref, rst = _solve(ahead, boards, False, node_order=no, mrv_after=mrv_after)
    assert np.array_equal(gst, rst) and np.array_equal(got, ref)
    assert gst[4] == 2 and gst[5] == 2  # clashing givens: the wave kernel's
    assert gst[3] == 0 and np.array_equal(got[3], dead)
    want, wst = O.solve_batch(boards[:3], order=order)
    assert np.array_equal(gst[:3], wst) and np.array_equal(got[:3], want)
    if order == "gen":  # the gen.py walk starts at the dead cell (node.py's would run for hours)
        want, wst = O.solve_batch(boards[3:4], order=order)
        assert wst[0] == 0 and np.array_equal(got[3:4], want)
    # depth overflow hands the board on
    _, st = _solve(ahead, np.zeros((1, 81), np.uint8), True, node_order=no, mrv_after=mrv_after, max_depth=3)
    assert st[0] == 2


@pytest.mark.parametrize("mrv_after", [0, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
@pytest.mark.parametrize("lane_guesses", [0, 1, 3])
def test_ahead_hand_over_to_wide(ahead, order, lane_guesses, mrv_after):
    """A lane phase of 0, 1 or 3 guesses on the look-ahead path, then the
    wave-wide solver from the same planes and stack (it never reads a line's
    und words): the lane solver's answers and statuses."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    boards = np.ascontiguousarray(np.concatenate([hard17_batch(150, seed=22).numpy(),
                                                  hard_search_batch(150, seed=23).numpy(), _gen_style(150, 56, 21),
                                                  np.zeros((1, 81), np.uint8)]))
    no = int(order == "node")
    want, wst = _solve(ahead, boards, False, node_order=no, mrv_after=mrv_after)
    got = np.zeros_like(boards)
    gst = np.zeros(len(boards), dtype=np.int32)
    pl, pw = ctypes.c_uint64(), ctypes.c_uint64()
    ahead.ahead_wide_batch(boards.ctypes.data, got.ctypes.data, gst.ctypes.data, len(boards), no, 81, mrv_after,
                           lane_guesses, ctypes.byref(pl), ctypes.byref(pw))
    assert np.array_equal(gst, wst) and np.array_equal(got, want)
    assert pw.value > 0 and (pl.value == 0) == (lane_guesses == 0)


def test_ahead_saves_passes(ahead, corpus):
    """The point of the change: on the 17-clue corpus fewer than 0.95 x the
    passes of plane::solve (0.9325 on 20 000 boards), branch nodes within
    1 %."""
    boards, _ = corpus
    new, old = {}, {}
    _solve(ahead, boards[:1500], True, mrv_after=128, stats=new)
    _solve(ahead, boards[:1500], False, mrv_after=128, stats=old)
    print("passes/board", old["passes"] / 1500, "->", new["passes"] / 1500, "ratio", new["passes"] / old["passes"],
          "guesses/board", old["guesses"] / 1500, "->", new["guesses"] / 1500)
    assert new["passes"] < 0.95 * old["passes"]
    assert abs(new["guesses"] - old["guesses"]) <= 0.01 * old["guesses"]
