"""GPU checks of the exact completion count (exact_kernel through
BatchSolver.count_exact) against the recorded fixture and the oracle's counter
on the pool of exact_cases.py: the sharing paths (donate, park, resume, the
board queue behind the task ring), the round budget, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as E

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 1025)  # one lane, a partial wave, a wave and a lane, the whole pool
MANY = 1 << 20             # a round budget no case comes near
# name -> count_exact's keywords; "default" runs the product's own slice and round budget
CONFIGS = {"default": {}, "slice1": dict(slice=1, max_rounds=MANY), "tiny-list": dict(slice=8, max_tasks=64, max_rounds=MANY),
           "waves2": dict(max_waves=2, max_rounds=MANY)}


def _run(solver, boards, **kw):
    count, status, stats = solver.count_exact(torch.from_numpy(np.ascontiguousarray(boards)), return_status=True,
                                              return_stats=True, **kw)
    return count.cpu().numpy(), status.cpu().numpy(), stats


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_counts_match_fixture_and_oracle(solver, n, config):
    """Bytes > 9 (count 0, SDK_INVALID) and clashing givens (count 0, DONE)
    are in the pool (set f) and come up from n = 63 on."""
    _, want, want_status = E.pool()
    boards, idx = E.mixed(n)
    count, status, stats = _run(solver, boards, **CONFIGS[config])
    print(n, config, stats)
    assert count.dtype == np.int64 and status.dtype == np.int32
    bad = np.nonzero((count != want[idx]) | (status != want_status[idx]))[0]
    assert len(bad) == 0, [(int(i), int(idx[i]), int(count[i]), int(want[idx[i]]), int(status[i])) for i in bad[:10]]
    slice_ = CONFIGS[config].get("slice")
    if slice_ is not None:
        assert stats["max_passes"] <= slice_ + E.RUN_MAX
    # a board with more completions than `slice` passes must stop at least once, and the first stop finds the ring
    # empty; 63 boards' levels after 8 passes overflow a ring of 128 lines
    if config == "slice1" and want[idx].max() >= 1024:
        E.check_path("slice1", stats)
    if config == "tiny-list" and n >= 63:
        E.check_path("tiny-list", stats)
    if n == 1025:
        assert (status == E.INVALID).any() and ((count == 0) & (status == E.DONE)).sum() > 200


def test_h1_alone_and_among_light_boards(solver):
    h1, want = E.load_fixture()["h1"]
    count, status, stats = _run(solver, h1[None])
    print("h1 alone", stats)
    assert (int(count[0]), int(status[0])) == (want, E.DONE)
    assert stats["rounds"] > 1 and stats["donated"] > 0  # one lane could not do it in one round: the work was shared
    boards, pool_want, _ = E.pool()
    light = np.nonzero((pool_want > 0) & (pool_want < 1024))[0][:64]
    batch = np.concatenate([boards[light[:40]], h1[None], boards[light[40:]]])
    count, status, _ = _run(solver, batch)
    assert (status == E.DONE).all()
    assert int(count[40]) == want
    assert np.array_equal(np.delete(count, 40), pool_want[light])
    plain = solver.count_exact(torch.from_numpy(batch))  # no status asked for: the counts alone, nothing raised
    assert plain.dtype == torch.int64 and np.array_equal(plain.cpu().numpy(), count)


def test_round_budget_gives_partial_and_returns(solver):
    """The empty board cannot finish in four rounds of 32 passes: PARTIAL with
    a lower bound, its neighbours DONE and exact, and without return_status
    the call raises."""
    from sudoku_solver_distributed_amd.solver import SudokuHipError
    boards, want, _ = E.pool()
    sel = np.nonzero((want == 1) | (want == 2))[0][:40]  # (light enough for any four rounds: 41 givens, set c)
    assert len(sel) == 40
    batch = np.concatenate([boards[sel[:20]], np.zeros((1, 81), np.uint8), boards[sel[20:]]])
    count, status, stats = _run(solver, batch, slice=32, max_rounds=4)
    assert stats["rounds"] == 4 and stats["max_passes"] <= 32 + E.RUN_MAX
    assert status[20] == E.PARTIAL and count[20] >= 0
    rest = np.arange(len(batch)) != 20
    assert (status[rest] == E.DONE).all() and np.array_equal(count[rest], want[sel])
    with pytest.raises(SudokuHipError):
        solver.count_exact(torch.from_numpy(batch), slice=32, max_rounds=4)


def test_back_to_back_calls_share_one_scratch(solver):
    """Two calls on one stream with the one cached scratch, the second
    smaller: each arms the scratch itself."""
    _, want, want_status = E.pool()
    boards, idx = E.mixed(65)
    d = torch.from_numpy(boards).to(solver.device)
    a = solver.count_exact(d, return_status=True, slice=8, max_tasks=64, max_rounds=MANY)
    b = solver.count_exact(d[:17], return_status=True, slice=8, max_tasks=64, max_rounds=MANY)
    assert np.array_equal(a[0].cpu().numpy(), want[idx]) and np.array_equal(a[1].cpu().numpy(), want_status[idx])
    assert np.array_equal(b[0].cpu().numpy(), want[idx[:17]]) and np.array_equal(b[1].cpu().numpy(), want_status[idx[:17]])
    assert solver.count_exact(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0,)
    solver.verify()  # the solve workspace's accounting is untouched


def test_argument_checks_on_device_buffers(solver):
    """-2 for each bad argument, before any launch: the buffers keep their
    bytes."""
    L = solver.lib
    n = 100
    boards = torch.zeros((n, 81), dtype=torch.uint8, device=solver.device)
    count = torch.full((n + 1,), 77, dtype=torch.int64, device=solver.device)
    status = torch.full((n + 1,), 77, dtype=torch.int32, device=solver.device)
    need = int(L.sdk_count_exact_scratch_bytes(n, 2, 64))
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=solver.device)
    st = (ctypes.c_int64 * 4)(*([5] * 4))
    ok = dict(boards=boards.data_ptr(), count=count.data_ptr(), status=status.data_ptr(), n=n, slice=8, rounds=4, tasks=64,
              scratch=scratch.data_ptr(), size=need, waves=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.sdk_count_exact_batch(a["boards"], a["count"], a["status"], a["n"], a["slice"], a["rounds"], a["tasks"],
                                       a["scratch"], a["size"], a["waves"], None, st)

    for bad in (dict(slice=0), dict(rounds=0), dict(tasks=-1), dict(n=-1), dict(waves=-1), dict(n=2 ** 31),
                dict(boards=None), dict(count=None), dict(status=None), dict(scratch=None),
                dict(count=count.data_ptr() + 4), dict(status=status.data_ptr() + 2), dict(scratch=scratch.data_ptr() + 8),
                dict(size=need - 1), dict(slice=2 ** 31 - 1, rounds=2 ** 31 - 1)):
        assert call(**bad) == -2, bad
    assert L.sdk_count_exact_batch(None, None, None, 0, 0, 0, -1, None, 0, -1, None, None) == 0  # n == 0 first
    torch.cuda.synchronize()
    assert bool((count == 77).all()) and bool((status == 77).all()) and list(st) == [5] * 4
    assert call() == 0  # and the same arguments, all good, run: n empty boards after four rounds of 8 passes
    assert bool((status[:n] == E.PARTIAL).all()) and int(status[n]) == 77 and int(count[n]) == 77
    assert st[0] == 4
