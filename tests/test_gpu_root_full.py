"""The plane kernel's root rule on the GPU (csrc/plane_kernel.h,
SDK_PLANE_ROOTFULL): an unordered launch's lanes take an all-single root as
solved without its verifying pass, and the outbox flush tests every board it
stores (plane::grid_complete, a board per lane), writes the status word and
defers a board that is no completion to the wave kernel.  Small mixed batches
forced onto the plane kernel, with the boards of
tests/golden/root_full_cases.json (all-single roots that are no completion)
among them, against the oracle.  Ordered mode keeps the verifying pass: the
frontier tests cover it."""
import numpy as np
import pytest
import torch

import root_full_cases as R
from conftest import b81
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"
# givens repeating a digit in a row (rules B/C unsound: the deferred list)
CLASH = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
DEAD = "123456780000000009" + "0" * 63  # cell (0, 8) has no candidate
ORDERS = ("gen", "node")


def _mix(n, seed):
    """n >= 64 boards: hard 17-clue and search-heavy boards interleaved, every
    fixture board spread evenly among them, an unsolvable board, a
    clashing-givens board and a byte > 9.  Returns the boards, the fixture
    boards' rows and the three single rows."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    fix = R.load_fixture()
    k = n // 2
    p = np.empty((n, 81), np.uint8)
    p[0::2] = hard17_batch(n - k, seed=seed).numpy()
    p[1::2] = hard_search_batch(k, seed=seed + 1).numpy()
    rows = (np.arange(len(fix)) * (n - 8) // len(fix)) + 4  # distinct for n >= 64: 40 rows in 4 .. n - 5
    assert len(np.unique(rows)) == len(fix)
    p[rows] = fix
    free = [i for i in range(n) if i not in set(rows.tolist())]
    special = {"dead": free[1], "clash": free[len(free) // 2], "bad": free[-2]}
    p[special["dead"]] = b81(DEAD)
    p[special["clash"]] = b81(CLASH)
    p[special["bad"], 40] = 12
    return p, rows, special


def _want(p, rows, special):
    """The oracle's answers per order: unique completions for the hard boards,
    the input back with status 0 for the fixture boards (no completion) and
    the unsolvable board, the literal walk for the clashing givens, status -1
    for the invalid byte."""
    want, cnt = O.solve_unique_batch(np.where(p > 9, 0, p).astype(np.uint8))
    wst = np.ones(len(p), np.int32)
    hard = np.ones(len(p), bool)
    hard[rows] = False
    hard[list(special.values())] = False
    assert (cnt[hard] == 1).all() and (cnt[rows] == 0).all()
    want[rows], wst[rows] = p[rows], 0
    want[special["dead"]], wst[special["dead"]] = p[special["dead"]], 0
    want[special["bad"]], wst[special["bad"]] = p[special["bad"]], -1
    out = {}
    for order in ORDERS:
        w, s = want.copy(), wst.copy()
        i = special["clash"]
        cw, cs = O.solve_batch(p[i:i + 1], order=order)
        w[i], s[i] = cw[0], cs[0]
        out[order] = (w, s)
    return out


@pytest.fixture(scope="module")
def batch2049():
    p, rows, special = _mix(2049, 71)
    return p, rows, _want(p, rows, special)


@pytest.fixture(scope="module")
def three_batches():
    parts = [_mix(n, 80 + i) for i, n in enumerate((700, 64, 1301))]
    return [(p, _want(p, rows, special)) for p, rows, special in parts]


@pytest.fixture
def plane_kernel(solver):
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    yield solver
    solver.lib.sdk_set_plane_tuning(-1, -1, -1, -1)
    solver.lib.sdk_set_solve_kernel(prev)


def _check_stats(solver, n, wst, nfix):
    s = solver.stats()
    assert s["finished"] == n
    assert s["solved"] == int((wst == 1).sum())
    assert s["deferred"] >= nfix
    solver.verify()


@pytest.mark.parametrize("order", ORDERS)
def test_mix_vs_oracle(plane_kernel, batch2049, order):
    solver = plane_kernel
    p, rows, want = batch2049
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), order=order, grid_waves=1)
    assert np.array_equal(st.cpu().numpy(), want[order][1])
    assert np.array_equal(sols.cpu().numpy(), want[order][0])
    _check_stats(solver, len(p), want[order][1], len(rows))


@pytest.mark.parametrize("order", ORDERS)
def test_mix_in_place(plane_kernel, batch2049, order):
    """Solutions over the puzzles: the flush is the only writer of a solved
    board's bytes, and a rejected board's bytes are still its input when the
    wave kernel reads them."""
    solver = plane_kernel
    p, rows, want = batch2049
    io = torch.from_numpy(p).cuda()
    solver.stats(reset=True)
    sols, st = solver.solve(io, out=io, order=order, grid_waves=1)
    assert sols.data_ptr() == io.data_ptr()
    assert np.array_equal(st.cpu().numpy(), want[order][1])
    assert np.array_equal(io.cpu().numpy(), want[order][0])
    _check_stats(solver, len(p), want[order][1], len(rows))


@pytest.mark.parametrize("order", ORDERS)
def test_three_batches_vs_oracle(plane_kernel, three_batches, order):
    """sdk_solve_batches over batches of 700, 64 and 1 301 boards of the mix
    (plane_kernel_multi)."""
    solver = plane_kernel
    batches = [torch.from_numpy(p).cuda() for p, _ in three_batches]
    outs = [torch.full_like(b, 0xEE) for b in batches]
    sts = [torch.full((b.shape[0],), 77, dtype=torch.int32, device=b.device) for b in batches]
    solver.stats(reset=True)
    got = solver.solve_batches(batches, outs, sts, order=order, grid_waves=1)
    torch.cuda.synchronize()
    for (p, want), (s, t) in zip(three_batches, got):
        assert np.array_equal(t.cpu().numpy(), want[order][1])
        assert np.array_equal(s.cpu().numpy(), want[order][0])
    wst = np.concatenate([want[order][1] for _, want in three_batches])
    _check_stats(solver, 700 + 64 + 1301, wst, 3 * len(R.load_fixture()))


def test_mix_tail_pool(plane_kernel, batch2049):
    """Tail mode 2: the waves' last boards continue on the wave-wide solver
    through the XCD pool, which keeps its own verifying passes."""
    solver = plane_kernel
    p, rows, want = batch2049
    assert solver.lib.sdk_set_plane_tuning(-1, 8, 2, -1) == 0
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), order="gen", grid_waves=1)
    assert np.array_equal(st.cpu().numpy(), want["gen"][1])
    assert np.array_equal(sols.cpu().numpy(), want["gen"][0])
    _check_stats(solver, len(p), want["gen"][1], len(rows))


def test_every_lane_rejects(plane_kernel):
    """Only fixture boards, 128 of them by repetition: whole flushes in which
    every lane rejects its board; nothing is stored as solved, every board is
    deferred and answered "no completion" with its input back.  (Tail 0: the
    lanes keep a wave's last boards, which the wave-wide solver would
    otherwise answer itself, with its own verifying pass and no deferral.)"""
    solver = plane_kernel
    assert solver.lib.sdk_set_plane_tuning(-1, 0, -1, -1) == 0
    fix = R.load_fixture()
    p = np.ascontiguousarray(np.concatenate([fix] * 4)[:128])
    out = torch.full((128, 81), 0xEE, dtype=torch.uint8, device="cuda")
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), out=out, grid_waves=1)
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(sols.cpu().numpy(), p)
    s = solver.stats()
    assert s["finished"] == 128 and s["solved"] == 0 and s["deferred"] == 128
    solver.verify()
