"""GPU checks of the batched completion count (count_kernel through
BatchSolver.count_solutions) against the oracle's counter on the mixed sets
of count_cases.py, and of the unique-puzzle generator built on it."""
import numpy as np
import pytest
import torch

import count_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4097)  # partial waves, one wave, a wave and a lane, many claims per wave


def _mixed(n):
    """n boards of the pool, shuffled so that the lanes of a wave diverge
    (every pool board at least once when n allows), and their pool indices."""
    k = len(C.pool()[0])
    rng = np.random.default_rng(1000 + n)
    idx = np.concatenate([rng.permutation(k), rng.integers(0, k, size=max(0, n - k))])[:n]
    rng.shuffle(idx)
    return np.ascontiguousarray(C.pool()[0][idx]), idx


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("limit,max_waves", [(2, 0), (64, 0), (2, 2)], ids=["limit2", "limit64", "limit2-waves2"])
def test_counts_and_first_match_oracle(solver, n, limit, max_waves):
    """With two waves every lane takes about 32 of the 4097 boards from the
    queue: claim, refill and drain all run."""
    _, _, uniq, is_unique, _ = C.pool()
    boards, idx = _mixed(n)
    cnt, first = solver.count_solutions(torch.from_numpy(boards), limit=limit, return_first=True, max_waves=max_waves)
    cnt, first = cnt.cpu().numpy(), first.cpu().numpy()
    want = C.expected(limit)[idx]
    bad = np.nonzero(cnt != want)[0]
    assert len(bad) == 0, [(int(i), int(idx[i]), int(cnt[i]), int(want[i])) for i in bad[:10]]
    C.check_first(boards, cnt, first, uniq[idx], is_unique[idx])
    only = solver.count_solutions(torch.from_numpy(boards), limit=limit, max_waves=max_waves)  # d_first = NULL
    assert np.array_equal(only.cpu().numpy(), cnt)


def test_single_boards_every_limit(solver):
    """Set f (the empty board reaches every limit, 1024 included) and a few
    boards of every other set at each limit of the CPU test."""
    boards, fixed, _, _, names = C.pool()
    sel = np.concatenate([np.nonzero(names == k)[0][:6] for k in "abcdef"])
    for limit in C.LIMITS:
        cnt = solver.count_solutions(torch.from_numpy(np.ascontiguousarray(boards[sel])), limit=limit).cpu().numpy()
        want = [O.count_solutions(boards[i], limit) if fixed[i] == 1 else fixed[i] for i in sel]  # these boards only
        assert list(cnt) == want, limit
        if limit == 1024:
            assert want[-5:] == [1024, 1, 0, 0, -1]
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            solver.count_solutions(torch.from_numpy(boards[:1].copy()), limit=bad)
    assert solver.count_solutions(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0,)


def test_back_to_back_calls_share_one_scratch(solver):
    """Two calls on one stream with the one cached scratch, nothing between
    them: the second call's queue head is re-armed in stream order."""
    boards, idx = _mixed(4097)
    d = torch.from_numpy(boards).to(solver.device)
    solver.count_solutions(d, limit=2)  # the scratch is sized now
    a = solver.count_solutions(d, limit=2)
    b = solver.count_solutions(d, limit=2)
    c = solver.count_solutions(d[:65], limit=2)
    want = C.expected(2)[idx]
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    assert np.array_equal(c.cpu().numpy(), want[:65])
    solver.verify()  # the solve workspace's accounting is untouched


def _restated_removals(full, order, empty_boxes):
    """unique_batch's removal loop with the oracle's counts."""
    puzzle = full.copy()
    for i in range(len(puzzle)):
        empties = 0
        for t in range(81):
            if empties >= empty_boxes:
                break
            trial = puzzle[i].copy()
            trial[order[i, t]] = 0
            if O.count_solutions(trial, 2) == 1:
                puzzle[i] = trial
                empties += 1
    return puzzle


def test_unique_batch_minimal(solver):
    from sudoku_solver_distributed_amd.gen import generate_batch, unique_batch
    n, seed = 32, 5
    puzzles, full = unique_batch(n, 81, seed=seed, return_solutions=True)
    assert puzzles.shape == (n, 81) and puzzles.dtype == torch.uint8 and puzzles.is_cuda
    puzzles, full = puzzles.cpu().numpy(), full.cpu().numpy()
    assert np.array_equal(full, generate_batch(n, 0, seed).cpu().numpy())
    sols, cnt = O.solve_unique_batch(puzzles)
    assert (cnt == 1).all() and np.array_equal(sols, full)
    for g in puzzles:
        assert O.count_solutions(g, 2) == 1
        for cell in np.nonzero(g)[0]:  # minimal: no clue can go
            t = g.copy()
            t[cell] = 0
            assert O.count_solutions(t, 2) == 2
    order = np.argsort(np.random.default_rng(seed).random((n, 81)), axis=1)
    assert np.array_equal(puzzles, _restated_removals(full, order, 81))
    assert np.array_equal(unique_batch(n, 81, seed=seed).cpu().numpy(), puzzles)


def test_unique_batch_capped_empties(solver):
    from sudoku_solver_distributed_amd.gen import unique_batch
    n, seed = 32, 5
    puzzles, full = unique_batch(n, 40, seed=seed, return_solutions=True)
    puzzles, full = puzzles.cpu().numpy(), full.cpu().numpy()
    assert ((puzzles == 0).sum(axis=1) <= 40).all()
    sols, cnt = O.solve_unique_batch(puzzles)
    assert (cnt == 1).all() and np.array_equal(sols, full)
    order = np.argsort(np.random.default_rng(seed).random((n, 81)), axis=1)
    assert np.array_equal(puzzles, _restated_removals(full, order, 40))
