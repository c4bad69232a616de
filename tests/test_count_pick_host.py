"""CPU checks of the count mode's branch rule (csrc/plane_solver.h
pick_count_masks: in search mode M_COUNT the solve path branches in the band
with the fewest two-candidate cells, ties to the most undetermined cells, then
the lowest band).  The header compiled for the host
(tests/native/count_pick_host.cpp over csrc/host_model.h): the lane pick and
the wave-wide solver's pick against a plain per-cell loop, the solvers that
branch on it against the oracle and the recorded walks, the lane -> wide
hand-over, two mutants of the rule, and the analysis headers' untouched rule."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, b81
from count_pick_native import lib as _lib
from oracle import oracle as O

LANE_ONLY = 0xFFFFFFFF
FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"


@pytest.fixture(scope="module")
def lib():
    return _lib()


def _check(lib, n=200_000, seed=7):
    bad = np.zeros(2, np.int64)
    seen = np.zeros(6, np.int64)
    lib.pick_check(n, seed, bad.ctypes.data, seen.ctypes.data)
    return bad, seen


def _solve(lib, boards, order="gen", mrv_after=128, ahead=1, lane_guesses=LANE_ONLY, max_depth=81, stats=None):
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    out = np.zeros_like(boards)
    st = np.zeros(len(boards), dtype=np.int32)
    g, pl, pw = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.pick_solve_batch(boards.ctypes.data, out.ctypes.data, st.ctypes.data, len(boards), int(order == "node"),
                         max_depth, mrv_after, ahead, lane_guesses, ctypes.byref(g), ctypes.byref(pl), ctypes.byref(pw))
    if stats is not None:
        stats.update(guesses=g.value, passes_lane=pl.value, passes_wide=pw.value)
    return out, st


@pytest.fixture(scope="module")
def corpus():
    """The suites of tests/test_plane_solver.py, computed once: 17-clue and
    search-heavy boards with their unique completions from the oracle, and
    generated boards (complete grids with 55 cells erased: many completions)
    plus the edge boards, with the literal walk's answers in both orders."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    hard = np.ascontiguousarray(np.concatenate([hard17_batch(256, seed=7).numpy(),
                                                hard_search_batch(100, seed=12).numpy()]))
    want, cnt = O.solve_unique_batch(hard)
    assert (cnt == 1).all()
    grids, _ = O.solve_unique_batch(hard17_batch(200, seed=4321).numpy())
    rng = np.random.default_rng(4321)
    for g in grids:
        g[rng.choice(81, 55, replace=False)] = 0
    dup = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
    edge = np.array([b81(x) for x in (FULL, "5" * 81, dup, "0" * 81)], dtype=np.uint8)
    gen = np.ascontiguousarray(np.concatenate([grids, edge]))
    walks = {order: O.solve_batch(gen, order=order) for order in ("gen", "node")}
    return {"hard": hard, "hard_want": want, "gen": gen, "walks": walks}


# ---- the rule itself

def test_count_pick_matches_plain_loop(lib):
    """plane::pick_count on 200 000 random plane states picks the cell the
    rule names when it is applied cell by cell (count_pick_host.cpp
    plain_pick); the states include every kind the rule distinguishes."""
    bad, seen = _check(lib)
    print("states: with a pair, only triples, neither, tie in key 1, tie in both keys, one open cell:", seen.tolist())
    assert (seen >= 2000).all(), seen.tolist()
    assert bad[0] == 0


def test_wide_pick_equals_lane_pick(lib):
    """The wave-wide solver's pick (wide::pick_count over the emulated wave of
    host_model.h) names the same cell from the same planes: both equal the
    plain loop on every state."""
    bad, _ = _check(lib, seed=11)
    assert bad[0] == 0 and bad[1] == 0


@pytest.mark.parametrize("variant,what", [(1, "most instead of fewest"), (2, "tie-break reversed")])
def test_mutants_fail_the_plain_loop_check(variant, what):
    """A rule that takes the band with the MOST cells, and one that breaks
    ties by the FEWEST undetermined cells, both fail
    test_count_pick_matches_plain_loop's comparison (lane and wide)."""
    bad, _ = _check(_lib(variant), n=50_000)
    assert bad[0] > 500 and bad[1] > 500, (what, bad.tolist())


# ---- the solvers that branch on it

@pytest.mark.parametrize("ahead", [0, 1], ids=["pass", "ahead"])
@pytest.mark.parametrize("mrv_after", [0, 1, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
def test_answers_equal_the_oracle(lib, corpus, order, mrv_after, ahead):
    """Unique completions (17-clue, search-heavy): the oracle's.  Generated
    boards with many completions, a full grid, clashing givens and the empty
    board: the literal walk's first completion in the given order -- count
    mode meets a second completion and must hand the board to the final walk."""
    got, st = _solve(lib, corpus["hard"], order, mrv_after, ahead)
    assert (st == 1).all() and np.array_equal(got, corpus["hard_want"])
    got, st = _solve(lib, corpus["gen"], order, mrv_after, ahead)
    want, wst = corpus["walks"][order]
    mine = st != 2
    assert st[-3] == 2 and st[-2] == 2 and mine.sum() == len(st) - 2  # "5" * 81 and dup: clashing givens
    assert np.array_equal(st[mine], wst[mine]) and np.array_equal(got[mine], want[mine])


@pytest.mark.parametrize("mrv_after", [1, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
def test_recorded_walks_many_completions_and_none(lib, order, mrv_after):
    """tests/golden/random_generated.npz: boards with two or more completions
    (the recorded answer is the walk's first: count mode must end in the final
    walk) and boards with none (reported unsolvable, the input back)."""
    z = np.load(os.path.join(GOLDEN, "random_generated.npz"))
    none = 0
    for empties, _n in z["cases"]:
        e = int(empties)
        puzzles = z[f"puzzles_{e}"]
        got, st = _solve(lib, puzzles, order, mrv_after)
        mine = st != 2
        assert np.array_equal(st[mine], z[f"{order}_status_{e}"][mine]), e
        assert np.array_equal(got[mine], z[f"{order}_solutions_{e}"][mine]), e
        dead = mine & (st == 0)
        assert np.array_equal(got[dead], puzzles[dead])
        none += int(dead.sum())
    print("boards without a completion:", none)


def test_unsolvable_in_count_mode(lib):
    """17-clue boards with one more clue their completion does not hold: no
    completion (or clashing givens, the wave kernel's), in count mode from the
    first pass on."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    rng = np.random.default_rng(11)
    b = hard17_batch(300, seed=12).numpy()
    sols, _ = O.solve_unique_batch(b)
    for i in range(len(b)):
        c = rng.choice(np.nonzero(b[i] == 0)[0])
        b[i, c] = 1 + (sols[i, c] + rng.integers(0, 8)) % 9
    for mrv_after in (1, 128):
        got, st = _solve(lib, b, "gen", mrv_after)
        mine = st != 2
        assert mine.sum() > 50 and (st[mine] == 0).all() and np.array_equal(got[mine], b[mine])


def test_walk_never_reaches_the_rule(corpus):
    """mrv_after = 0: the search never enters count mode, so the rule is not
    called and passes and guesses equal those of the rule before
    (plane::pick_mrv_masks); with the switch on it is called."""
    counting, before = _lib(3), _lib(4)
    boards = np.concatenate([corpus["hard"], corpus["gen"]])
    for order in ("gen", "node"):
        new, old = {}, {}
        c0 = counting.pick_calls()
        a, ast = _solve(counting, boards, order, 0, stats=new)
        assert counting.pick_calls() == c0
        b, bst = _solve(before, boards, order, 0, stats=old)
        assert new == old and np.array_equal(a, b) and np.array_equal(ast, bst)
    _solve(counting, corpus["hard"], "gen", 128)
    assert counting.pick_calls() > c0


@pytest.mark.parametrize("mrv_after", [1, 128], ids=lambda k: f"mrv{k}")
@pytest.mark.parametrize("order", ["gen", "node"])
@pytest.mark.parametrize("lane_guesses", [0, 1, 3])
def test_hand_over_to_wide_same_answers(lib, corpus, order, lane_guesses, mrv_after):
    """0, 1 or 3 guesses on the look-ahead lane path, then the wave-wide
    solver from the same planes, stack and search mode: the lane solver's
    answers and statuses, which are the oracle's."""
    boards = np.concatenate([corpus["hard"], corpus["gen"]])
    want, wst = _solve(lib, boards, order, mrv_after)
    s = {}
    got, gst = _solve(lib, boards, order, mrv_after, lane_guesses=lane_guesses, stats=s)
    assert np.array_equal(gst, wst) and np.array_equal(got, want)
    assert s["passes_wide"] > 0 and (s["passes_lane"] == 0) == (lane_guesses == 0)
    n = len(corpus["hard"])
    assert np.array_equal(got[:n], corpus["hard_want"])


def test_rule_saves_passes_on_the_17_clue_corpus(lib):
    """The point of the rule.  scripts/pick_study.py on 20 000 boards per
    seed: 6.0 % fewer passes and 14 % fewer branch nodes than the rule
    before; on these 3000 boards it has to keep more than half of either."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    boards = hard17_batch(3000, seed=3).numpy()
    new, old = {}, {}
    a, ast = _solve(lib, boards, "gen", 128, max_depth=32, stats=new)
    b, bst = _solve(_lib(4), boards, "gen", 128, max_depth=32, stats=old)
    assert np.array_equal(a, b) and np.array_equal(ast, bst)
    print("passes/board", old["passes_lane"] / 3000, "->", new["passes_lane"] / 3000,
          "guesses/board", old["guesses"] / 3000, "->", new["guesses"] / 3000)
    assert new["passes_lane"] < 0.97 * old["passes_lane"]
    assert new["guesses"] < 0.93 * old["guesses"]


# ---- the analysis headers keep the rule before

def test_analysis_headers_keep_pick_mrv():
    """plane_count.h and plane_sample.h (and through them the exact, list,
    candidates, minimise and unique kernels) call plane::pick_mrv, whose rule
    is untouched: their fixtures pin its visiting order, and their host tests
    (tests/test_count_host.py, tests/test_sample_host.py, ...) pass unchanged."""
    csrc = os.path.join(os.path.dirname(GOLDEN), "..", "sudoku_solver_distributed_amd", "csrc")
    for name in os.listdir(csrc):
        text = open(os.path.join(csrc, name)).read()
        if name in ("plane_solver.h", "plane_wide.h"):
            continue
        assert "pick_count" not in text and "SDK_PLANE_COUNT_PICK" not in text, name
    for name in ("plane_count.h", "plane_sample.h"):
        assert "pick_mrv(B, und, band, pos)" in open(os.path.join(csrc, name)).read(), name
    # and the rule before, still first-band-first on a state where the new rule leaves band 0
    lib4, lib0 = _lib(4), _lib()
    bad4, _ = _check(lib4, n=20_000)
    bad0, _ = _check(lib0, n=20_000)
    assert bad0[0] == 0 and bad4[0] > 1000
