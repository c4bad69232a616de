"""The plane kernel with rule C's column table (csrc/plane_kernel.h with
SDK_PLANE_COLTBL: a second LDS table beside the lock table, paid for with the
staging area's spare dword; tests/test_gpu_lock_table.py checks the pass's
answers and lane-loop totals) at the store path's outbox boundary: waves whose
lanes all finish in one iteration (64 copies of a board that needs no guess,
64 complete grids) and one board repeated cap-1, cap, cap+1, 2 cap+1 and 129
times, cap = the outbox's records; through plane_kernel, plane_kernel_multi
(split 1 / 63 / rest) and in place; every byte and status against the oracle,
nothing outside the n boards written.  And the full grid still holds 16 waves
per CU: the table's kilobyte did not cost the workgroup its LDS slot."""
import ctypes

import numpy as np
import pytest
import torch

import count_pick_native
from oracle import oracle as O

pytestmark = pytest.mark.gpu
CAP = 64              # csrc/plane_kernel.h PLANE_OUTBOX: records of a wave's outbox
PLANE_MAX_DEPTH = 32  # csrc/common.h
GUARD = 3             # guard rows before and after an output
MARK, SMARK = 0xEE, 77
FULL = "534678912672195348198342567859761423426853791713924856961537284287419635345286179"


def b81(s):
    return np.frombuffer(s.encode(), np.uint8) - ord("0")


@pytest.fixture(scope="module")
def corpus():
    """a 17-clue board the lanes solve without a guess, with its answer; 64
    different complete grids; a board without a completion and one with
    clashing givens, with the oracle's word on both.  Computed once."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    hard = hard17_batch(64, seed=51).numpy()
    grids, cnt = O.solve_unique_batch(hard)
    assert (cnt == 1).all()
    lib = count_pick_native.lib()
    root = None
    out, hst, one = np.zeros((1, 81), np.uint8), np.zeros(1, np.int32), np.zeros(1, np.uint32)
    for i in range(len(hard)):
        g, ps = ctypes.c_uint64(), ctypes.c_uint64()
        lib.pick_lane_totals(hard[i:i + 1].ctypes.data, out.ctypes.data, hst.ctypes.data, 1, 0, PLANE_MAX_DEPTH, 128,
                             ctypes.byref(g), ctypes.byref(ps), one.ctypes.data)
        if g.value == 0 and hst[0] == 1:
            root = i
            break
    assert root is not None
    dead = np.zeros(81, np.uint8)  # cell (8, 8) has no candidate: row 8 holds 2..9, column 8 a 1
    dead[72:80] = [2, 3, 4, 5, 6, 7, 8, 9]
    dead[63 + 8] = 1
    odd = np.array([dead, b81("88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:])], np.uint8)
    odd_want, odd_st = O.solve_batch(odd)
    return {"board": hard[root].copy(), "answer": grids[root].copy(), "grids": np.ascontiguousarray(grids),
            "odd": odd, "odd_want": odd_want, "odd_st": odd_st}


@pytest.fixture
def plane(solver):
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    yield solver
    solver.lib.sdk_set_solve_kernel(prev)


def _guarded(n):
    out = torch.full((n + 2 * GUARD, 81), MARK, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 2 * GUARD,), SMARK, dtype=torch.int32, device="cuda")
    return out, st


def _guards_clean(out, st, n):
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert (o[:GUARD] == MARK).all() and (o[GUARD + n:] == MARK).all()
    assert (s[:GUARD] == SMARK).all() and (s[GUARD + n:] == SMARK).all()


def _run_all_ways(solver, boards, want, wst, clean=True):
    """plane_kernel, plane_kernel_multi split 1 / 63 / rest, and in place"""
    n = len(boards)
    dev = torch.from_numpy(np.ascontiguousarray(boards)).cuda()

    def totals():
        s = solver.stats()
        if clean:
            assert s["finished"] == n and s["solved"] == n and s["deferred"] == 0
        solver.verify()

    # one batch
    out, st = _guarded(n)
    solver.stats(reset=True)
    solver.solve(dev, out=out[GUARD:GUARD + n], status=st[GUARD:GUARD + n])
    torch.cuda.synchronize()
    assert np.array_equal(st[GUARD:GUARD + n].cpu().numpy(), wst)
    assert np.array_equal(out[GUARD:GUARD + n].cpu().numpy(), want)
    _guards_clean(out, st, n)
    totals()
    # several batches in one launch
    cuts = [c for c in ((0, 1), (1, 64), (64, n)) if c[0] < min(c[1], n)]
    cuts = [(a, min(b, n)) for a, b in cuts]
    bufs = [_guarded(b - a) for a, b in cuts]
    solver.stats(reset=True)
    solver.solve_batches([dev[a:b] for a, b in cuts], [o[GUARD:GUARD + b - a] for (a, b), (o, _) in zip(cuts, bufs)],
                         [s[GUARD:GUARD + b - a] for (a, b), (_, s) in zip(cuts, bufs)])
    torch.cuda.synchronize()
    for (a, b), (o, s) in zip(cuts, bufs):
        assert np.array_equal(s[GUARD:GUARD + b - a].cpu().numpy(), wst[a:b])
        assert np.array_equal(o[GUARD:GUARD + b - a].cpu().numpy(), want[a:b])
        _guards_clean(o, s, b - a)
    totals()
    # in place
    io, st = _guarded(n)
    io[GUARD:GUARD + n] = dev
    solver.stats(reset=True)
    sols, _ = solver.solve(io[GUARD:GUARD + n], out=io[GUARD:GUARD + n], status=st[GUARD:GUARD + n])
    torch.cuda.synchronize()
    assert sols.data_ptr() == io[GUARD:GUARD + n].data_ptr()
    assert np.array_equal(st[GUARD:GUARD + n].cpu().numpy(), wst)
    assert np.array_equal(io[GUARD:GUARD + n].cpu().numpy(), want)
    _guards_clean(io, st, n)
    totals()


@pytest.mark.parametrize("n", [CAP - 1, CAP, CAP + 1, 2 * CAP + 1, 129])
def test_one_board_repeated(plane, corpus, n):
    boards = np.repeat(corpus["board"][None], n, 0)
    _run_all_ways(plane, boards, np.repeat(corpus["answer"][None], n, 0), np.ones(n, np.int32))


def test_a_wave_of_complete_grids(plane, corpus):
    g = corpus["grids"]
    assert len(g) == 64
    _run_all_ways(plane, g, g, np.ones(64, np.int32))


@pytest.mark.parametrize("n", [CAP, 2 * CAP + 1])
def test_copies_with_an_unsolvable_and_a_clashing_board_among_them(plane, corpus, n):
    boards = np.repeat(corpus["board"][None], n, 0)
    want = np.repeat(corpus["answer"][None], n, 0)
    wst = np.ones(n, np.int32)
    for k, at in enumerate((n // 3, n - 2)):
        boards[at], want[at], wst[at] = corpus["odd"][k], corpus["odd_want"][k], corpus["odd_st"][k]
    _run_all_ways(plane, boards, want, wst, clean=False)


def test_full_grid_holds_sixteen_waves_per_cu(plane):
    """the workspace's stacks are sized for the full grid (sdk_workspace_bytes:
    a stack per lane of it, PLANE_MAX_DEPTH lines of 128 bytes, after 256
    bytes of counters and before the 2^20-entry deferred list and the tail
    pool): its lanes are 16 waves on every CU"""
    pool = 8 * (32 + 16384 * (36 + 1)) * 4  # common.h PLANE_POOL_BYTES
    stacks = int(plane.lib.sdk_workspace_bytes()) - 256 - (1 << 20) * 8 - pool
    assert stacks % (PLANE_MAX_DEPTH * 128) == 0
    lanes = stacks // (PLANE_MAX_DEPTH * 128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("lanes of the full grid", lanes, "CUs", cus)
    assert lanes == cus * 16 * 64
