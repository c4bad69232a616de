"""The count mode's branch rule on the GPU (csrc/plane_solver.h
pick_count_masks: the band with the fewest two-candidate cells, in the lane
loop's search step and in the wave-wide tail solver): hard 17-clue boards
forced onto the plane kernel, one wave per SIMD, every byte and status against
the oracle -- through one launch, the queue with refills and a drain, the
wide solver alone, count mode from the first pass, sdk_solve_batches, the XCD
pool and an in-place solve -- and the launch's guesses and sweeps against the
host model where only the lane loop runs."""
import ctypes

import numpy as np
import pytest
import torch

import count_pick_native
from oracle import oracle as O

pytestmark = pytest.mark.gpu
PLANE_MAX_DEPTH = 32  # csrc/common.h


@pytest.fixture(scope="module")
def hard4096():
    """4096 hard 17-clue boards (about a quarter keep >= 58 open cells at the
    propagated root and start in count mode) and their unique completions
    from the oracle, computed once."""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    p = np.ascontiguousarray(hard17_batch(4096, seed=97).numpy())
    want, cnt = O.solve_unique_batch(p)
    assert (cnt == 1).all()
    return p, want


@pytest.fixture
def plane_kernel(solver):
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    yield solver
    solver.lib.sdk_set_plane_tuning(-1, -1, -1, -1)
    solver.lib.sdk_set_plane_search(-1)
    solver.lib.sdk_set_solve_kernel(prev)


def _same(sols, st, want):
    assert (st.cpu().numpy() == 1).all()
    assert np.array_equal(sols.cpu().numpy(), want)


def test_one_launch(plane_kernel, hard4096):
    solver = plane_kernel
    p, want = hard4096
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), grid_waves=1)
    _same(sols, st, want)
    s = solver.stats()
    assert s["finished"] == 4096 and s["solved"] == 4096 and s["deferred"] == 0
    solver.verify()


def test_lane_loop_totals_equal_host_model(plane_kernel, hard4096):
    """Tail 0: the lanes keep every board to its end, so the launch runs the
    lane loop alone and its guesses and sweeps are the host model's totals
    (host_model.h's driver on the look-ahead path with the root rule, depth
    32, the default switch at 128).  With the default tail, tail mode 2 or
    fewer boards than the tail threshold, the wave-wide solver finishes some
    boards on its own pass, which places a pass's hidden singles at once: those
    launches' totals differ by design and are not compared."""
    solver = plane_kernel
    p, want = hard4096
    lib = count_pick_native.lib()
    out = np.zeros_like(p)
    hst = np.zeros(len(p), np.int32)
    per = np.zeros(len(p), np.uint32)
    g, ps = ctypes.c_uint64(), ctypes.c_uint64()
    lib.pick_lane_totals(p.ctypes.data, out.ctypes.data, hst.ctypes.data, len(p), 0, PLANE_MAX_DEPTH, 128,
                         ctypes.byref(g), ctypes.byref(ps), per.ctypes.data)
    assert (hst == 1).all() and np.array_equal(out, want)
    assert solver.lib.sdk_set_plane_tuning(-1, 0, -1, -1) == 0
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), grid_waves=1)
    _same(sols, st, want)
    s = solver.stats()
    print("guesses", s["guesses"], "host", g.value, "sweeps", s["sweeps"], "host", ps.value)
    assert s["deferred"] == 0
    assert s["guesses"] == g.value and s["sweeps"] == ps.value


def test_queue_refills_and_drain(plane_kernel, hard4096):
    """65 536 + 4097 boards (the 4096 in shuffled rounds): more than one wave
    per SIMD holds, so the queue refills lanes and drains."""
    solver = plane_kernel
    p, want = hard4096
    n = 65536 + 4097
    idx = np.concatenate([np.random.default_rng(k).permutation(4096) for k in range(18)])[:n]
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(np.ascontiguousarray(p[idx])).cuda(), grid_waves=1)
    _same(sols, st, want[idx])
    assert solver.stats()["finished"] == n
    solver.verify()


def test_five_boards_all_wide(plane_kernel, hard4096):
    """5 boards: the wave is below the tail threshold at once, the whole
    search runs on the wave-wide solver (count-mode roots among them)."""
    solver = plane_kernel
    p, want = hard4096
    for lo in (0, 5, 10):
        sols, st = solver.solve(torch.from_numpy(p[lo:lo + 5].copy()).cuda(), grid_waves=1)
        _same(sols, st, want[lo:lo + 5])


def test_every_searching_board_counts(plane_kernel, hard4096):
    """sdk_set_plane_search(1): every board that searches at all counts its
    completions from its first stuck pass."""
    solver = plane_kernel
    p, want = hard4096
    assert solver.lib.sdk_set_plane_search(1) >= 0
    sols, st = solver.solve(torch.from_numpy(p[:64].copy()).cuda(), grid_waves=1)
    _same(sols, st, want[:64])


def test_three_unequal_batches(plane_kernel, hard4096):
    solver = plane_kernel
    p, want = hard4096
    cuts = [(0, 700), (700, 764), (764, 4096)]
    batches = [torch.from_numpy(p[a:b].copy()).cuda() for a, b in cuts]
    outs = [torch.full_like(b, 0xEE) for b in batches]
    sts = [torch.full((b.shape[0],), 77, dtype=torch.int32, device=b.device) for b in batches]
    solver.stats(reset=True)
    got = solver.solve_batches(batches, outs, sts, grid_waves=1)
    torch.cuda.synchronize()
    for (a, b), (s, t) in zip(cuts, got):
        _same(s, t, want[a:b])
    assert solver.stats()["finished"] == 4096
    solver.verify()


def test_tail_pool(plane_kernel, hard4096):
    """Tail mode 2: a wave's last boards continue on the wave-wide solver
    through the XCD pool, in the tree the lanes began."""
    solver = plane_kernel
    p, want = hard4096
    assert solver.lib.sdk_set_plane_tuning(-1, 8, 2, -1) == 0
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), grid_waves=1)
    _same(sols, st, want)
    assert solver.stats()["finished"] == 4096
    solver.verify()


def test_in_place(plane_kernel, hard4096):
    solver = plane_kernel
    p, want = hard4096
    io = torch.from_numpy(p.copy()).cuda()
    sols, st = solver.solve(io, out=io, grid_waves=1)
    assert sols.data_ptr() == io.data_ptr()
    _same(io, st, want)
