"""CPU checks of the root rule (csrc/plane_solver.h search_step_impl's
root_full: a board whose root is all single after an OPEN pass is taken as
solved without its verifying pass, and plane::grid_complete tests the answer,
as the plane kernel's outbox flush does), on the host model
(tests/native/rootfull_host.cpp over csrc/host_model.h)."""
import os

import numpy as np
import pytest

import root_full_cases as R
from conftest import GOLDEN
from oracle import oracle as O

FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"


def _sets():
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    z = np.load(os.path.join(GOLDEN, "random_generated.npz"))
    out = {"hard17": hard17_batch(20000, seed=3).numpy(), "hard_search": hard_search_batch(4096, seed=21).numpy()}
    for empties, _n in z["cases"]:
        out[f"random_{int(empties)}"] = z[f"puzzles_{int(empties)}"]
    return out


@pytest.fixture(scope="module")
def sets():
    return _sets()


@pytest.fixture(scope="module", params=["gen", "node"])
def runs(request, sets):
    """rootfull_compare on every set, once per order"""
    no = int(request.param == "node")
    return {k: R.compare(v, node_order=no) for k, v in sets.items()}


def test_grid_complete_predicate():
    """Completions pass; a grid with one cell changed, with two cells of a row
    swapped across boxes, or with a 9 turned into a digit its units already
    hold (every digit 1..8 still present in every unit: why all nine digits
    are tested) fails."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    grids, cnt = O.solve_unique_batch(hard17_batch(200, seed=5).numpy())
    assert (cnt == 1).all() and R.grid_complete(grids).all()
    rng = np.random.default_rng(7)
    bad = []
    for g in grids:
        a = g.copy()
        c = int(rng.integers(81))
        a[c] = a[c] % 9 + 1
        b = g.copy()
        r = int(rng.integers(9))
        b[[9 * r + 2, 9 * r + 3]] = b[[9 * r + 3, 9 * r + 2]]
        n = g.copy()
        nine = np.nonzero(n == 9)[0]
        n[nine[int(rng.integers(9))]] = int(rng.integers(1, 9))
        bad += [a, b, n]
    assert not R.grid_complete(np.array(bad)).any()
    full = np.array([int(c) for c in FULL], np.uint8)
    assert R.grid_complete(full)[0]


def test_fixture_keeps_its_teeth():
    """Every fixture board: the host model takes the rule, the predicate
    rejects the all-single root (status 2: the wave kernel's), and the board
    has no completion -- the oracle's count, and the host model's own answer
    with the verifying pass."""
    boards = R.load_fixture()
    assert len(boards) >= 32
    _, cnt = O.solve_unique_batch(boards)
    assert (cnt == 0).all()
    for no in (0, 1):
        r = R.compare(boards, node_order=no)
        assert (r["by_rule"] == 1).all() and (r["rejected"] == 1).all()
        assert (r["st_on"] == 2).all() and (r["st_off"] == 0).all()
        assert np.array_equal(r["out_on"], boards) and np.array_equal(r["out_off"], boards)
        assert (r["passes_on"] < r["passes_off"]).all()


def test_answers_identical(runs):
    for k, r in runs.items():
        assert np.array_equal(r["st_on"], r["st_off"]), k
        assert np.array_equal(r["out_on"], r["out_off"]), k
        assert not r["rejected"].any(), k


def test_passes_saved_are_the_rule_boards(runs):
    """A board that ends by the rule saves exactly its verifying pass; every
    other board's passes are unchanged."""
    for k, r in runs.items():
        saved = r["passes_off"].astype(np.int64) - r["passes_on"].astype(np.int64)
        assert (saved >= 0).all(), k
        assert np.array_equal(saved, r["by_rule"].astype(np.int64)), k
    h = runs["hard17"]
    n = len(h["by_rule"])
    print("hard17: by rule", int(h["by_rule"].sum()), "of", n, "passes/board", h["passes_off"].sum() / n, "->",
          h["passes_on"].sum() / n)
    # the flagship's boards: more than half end at the root
    assert h["by_rule"].sum() > 0.5 * n


def test_answers_against_oracle(sets, runs):
    for k in ("hard17", "hard_search"):
        want, cnt = O.solve_unique_batch(sets[k][:2000])
        assert (cnt == 1).all()
        assert (runs[k]["st_on"][:2000] == 1).all() and np.array_equal(runs[k]["out_on"][:2000], want), k


def test_solve_ahead_with_the_rule(sets):
    """plane::solve_ahead, the lane solver's own driver: the same answers with
    the rule, -1 (the wave kernel's board) on the fixture."""
    lib = R.lib()
    boards = np.ascontiguousarray(np.concatenate([sets["hard17"][:1500], sets["hard_search"][:300], R.load_fixture()]))
    nf = len(R.load_fixture())
    res = []
    for rule in (0, 1):
        out, st = np.zeros_like(boards), np.zeros(len(boards), np.int32)
        lib.rootfull_solve_ahead(boards.ctypes.data, out.ctypes.data, st.ctypes.data, len(boards), 0, 32, 128, rule)
        res.append((out, st))
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1][:-nf], res[1][1][:-nf]) and (res[1][1][:-nf] == 1).all()
    assert (res[0][1][-nf:] == 0).all() and (res[1][1][-nf:] == -1).all()
