"""Rule D's box -> row table on the GPU (csrc/plane_kernel.h with
SDK_PLANE_LOCKTBL: one 512-entry table in LDS per four-wave workgroup, filled
at the kernel's start behind the kernel's only workgroup barrier): the plane
kernel pinned, every byte and status against the oracle, and -- with the tail
off, so that the launch runs the lane loop alone -- the launch's sweeps and
guesses against the host model's totals, which a wrong table entry changes even
where the answer survives.  Sizes: a mix of 4096 boards, one board, 65 (a wave
with one board beside sibling waves with none: every wave must still reach the
barrier), 257 (a second workgroup with one board), three unequal batches in one
launch, and an in-place solve."""
import ctypes

import numpy as np
import pytest
import torch

import count_pick_native
from oracle import oracle as O

pytestmark = pytest.mark.gpu
PLANE_MAX_DEPTH = 32  # csrc/common.h


def _gen_style(n, empties, seed):
    """gen.py-style boards on the CPU: complete grids with cells erased"""
    from sudoku_solver_distributed_amd.gen import hard17_batch
    grids, _ = O.solve_unique_batch(hard17_batch(n, seed=seed).numpy())
    rng = np.random.default_rng(seed)
    for g in grids:
        g[rng.choice(81, empties, replace=False)] = 0
    return grids


@pytest.fixture(scope="module")
def mixed():
    """4096 boards, shuffled: 2048 hard 17-clue, 1024 search-heavy and 1024
    gen-style ones; the walk's answers from the oracle; and per board the host
    model's lane-loop passes and guesses (host_model.h's driver on the
    look-ahead path with the root rule, depth 32, the switch at 128).
    Computed once."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    hard = np.concatenate([hard17_batch(2048, seed=41).numpy(), hard_search_batch(1024, seed=42).numpy()])
    want_h, cnt = O.solve_unique_batch(hard)  # one completion each: the walk's answer
    assert (cnt == 1).all()
    easy = _gen_style(1024, 50, 43)
    want_e, wst = O.solve_batch(easy)  # many completions: the literal walk
    assert (wst == 1).all()
    perm = np.random.default_rng(44).permutation(4096)
    p = np.ascontiguousarray(np.concatenate([hard, easy])[perm])
    want = np.ascontiguousarray(np.concatenate([want_h, want_e])[perm])
    lib = count_pick_native.lib()
    out = np.zeros_like(p)
    hst = np.zeros(len(p), np.int32)
    passes = np.zeros(len(p), np.uint32)
    guesses = np.zeros(len(p), np.uint64)
    g, ps = ctypes.c_uint64(), ctypes.c_uint64()
    lib.pick_lane_totals(p.ctypes.data, out.ctypes.data, hst.ctypes.data, len(p), 0, PLANE_MAX_DEPTH, 128,
                         ctypes.byref(g), ctypes.byref(ps), passes.ctypes.data)
    assert (hst == 1).all() and np.array_equal(out, want)
    assert int(passes.sum()) == ps.value
    # guesses per board: the totals of the one-board runs (cheap: the passes are known, the guesses are not returned)
    one = np.zeros(1, np.uint32)
    for i in range(len(p)):
        gi, pi = ctypes.c_uint64(), ctypes.c_uint64()
        lib.pick_lane_totals(p[i:i + 1].ctypes.data, out[i:i + 1].ctypes.data, hst[i:i + 1].ctypes.data, 1, 0,
                             PLANE_MAX_DEPTH, 128, ctypes.byref(gi), ctypes.byref(pi), one.ctypes.data)
        guesses[i] = gi.value
    assert int(guesses.sum()) == g.value
    return p, want, passes.astype(np.uint64), guesses


@pytest.fixture
def lane_loop_only(solver):
    """the plane kernel pinned, its tail off: the lanes keep every board to its end"""
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    assert solver.lib.sdk_set_plane_tuning(-1, 0, -1, -1) == 0
    yield solver
    solver.lib.sdk_set_plane_tuning(-1, -1, -1, -1)
    solver.lib.sdk_set_solve_kernel(prev)


def _check(solver, sols, st, want, passes, guesses, n):
    assert (st.cpu().numpy() == 1).all()
    assert np.array_equal(sols.cpu().numpy(), want)
    s = solver.stats()
    print("n", n, "sweeps", s["sweeps"], "host", int(passes.sum()), "guesses", s["guesses"], "host", int(guesses.sum()))
    assert s["finished"] == n and s["solved"] == n and s["deferred"] == 0
    assert s["sweeps"] == int(passes.sum()) and s["guesses"] == int(guesses.sum())
    solver.verify()


@pytest.mark.parametrize("n", [4096, 1, 65, 257])
def test_answers_and_lane_loop_totals(lane_loop_only, mixed, n):
    solver = lane_loop_only
    p, want, passes, guesses = mixed
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p[:n].copy()).cuda())
    _check(solver, sols, st, want[:n], passes[:n], guesses[:n], n)


def test_default_tail(solver, mixed):
    """the shipped launch shape (wave-wide tail on): answers only, the tail's
    passes are its own"""
    from sudoku_solver_distributed_amd import _lib
    p, want, _, _ = mixed
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    try:
        solver.stats(reset=True)
        sols, st = solver.solve(torch.from_numpy(p).cuda())
        assert (st.cpu().numpy() == 1).all() and np.array_equal(sols.cpu().numpy(), want)
        assert solver.stats()["finished"] == len(p)
    finally:
        solver.lib.sdk_set_solve_kernel(prev)


def test_three_unequal_batches(lane_loop_only, mixed):
    """one sdk_solve_batches launch (plane_kernel_multi) over batches of 1, 63 and 4097 boards"""
    solver = lane_loop_only
    p, want, passes, guesses = mixed
    idx = np.concatenate([np.arange(4096), np.arange(65)])  # 4161 boards
    cuts = [(0, 1), (1, 64), (64, 4161)]
    batches = [torch.from_numpy(np.ascontiguousarray(p[idx[a:b]])).cuda() for a, b in cuts]
    outs = [torch.full_like(b, 0xEE) for b in batches]
    sts = [torch.full((b.shape[0],), 77, dtype=torch.int32, device=b.device) for b in batches]
    solver.stats(reset=True)
    got = solver.solve_batches(batches, outs, sts)
    torch.cuda.synchronize()
    for (a, b), (s, t) in zip(cuts, got):
        assert (t.cpu().numpy() == 1).all() and np.array_equal(s.cpu().numpy(), want[idx[a:b]])
    s = solver.stats()
    assert s["finished"] == len(idx) and s["deferred"] == 0
    assert s["sweeps"] == int(passes[idx].sum()) and s["guesses"] == int(guesses[idx].sum())
    solver.verify()


def test_in_place(lane_loop_only, mixed):
    solver = lane_loop_only
    p, want, passes, guesses = mixed
    io = torch.from_numpy(p.copy()).cuda()
    solver.stats(reset=True)
    sols, st = solver.solve(io, out=io)
    assert sols.data_ptr() == io.data_ptr()
    _check(solver, io, st, want, passes, guesses, len(p))
