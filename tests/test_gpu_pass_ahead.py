"""The plane kernel's lane loop on the look-ahead pass (plane::pass_ahead,
search_step_ahead; a stack level keeps its undetermined cells in an eighth
quad of its line): small mixed batches forced onto the plane kernel, so that
lanes guess, pop several levels deep, switch to the completion count, defer
and drain, against the oracle."""
import numpy as np
import pytest
import torch

from conftest import b81
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"
# givens repeating a digit in a row (rules B/C unsound: the deferred list)
CLASH = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
DEAD = "123456780000000009" + "0" * 63  # cell (0, 8) has no candidate


def _mix(n, seed):
    """n boards: hard 17-clue and search-heavy boards (pops several levels
    deep, the switch to the count), interleaved; an unsolvable board, a
    clashing-givens board and a byte > 9 where the batch is long enough."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    k = n // 2
    p = np.empty((n, 81), np.uint8)
    p[0::2] = hard17_batch(n - k, seed=seed).numpy()
    p[1::2] = hard_search_batch(k, seed=seed + 1).numpy()
    special = {}
    if n >= 64:
        p[7] = b81(DEAD)
        p[n // 2 + 1] = b81(CLASH)
        p[n - 3, 40] = 12
        special = {"dead": 7, "clash": n // 2 + 1, "bad": n - 3}
    return p, special


def _want(p, special, order):
    """The oracle's answers: unique completions for the hard boards, the
    literal walk for the clashing givens, the input back (status 0 / -1) for
    the unsolvable board and the invalid byte."""
    want, cnt = O.solve_unique_batch(np.where(p > 9, 0, p).astype(np.uint8))
    wst = np.ones(len(p), np.int32)
    hard = np.ones(len(p), bool)
    for i in special.values():
        hard[i] = False
    assert (cnt[hard] == 1).all()
    if special:
        i = special["dead"]
        want[i], wst[i] = p[i], 0
        i = special["clash"]
        w, s = O.solve_batch(p[i:i + 1], order=order)
        want[i], wst[i] = w[0], s[0]
        i = special["bad"]
        want[i], wst[i] = p[i], -1
    return want, wst


@pytest.fixture(scope="module")
def batch2049():
    p, special = _mix(2049, 41)
    return p, special, {o: _want(p, special, o) for o in ("gen", "node")}


@pytest.fixture
def plane_kernel(solver):
    from sudoku_solver_distributed_amd import _lib
    prev = solver.lib.sdk_set_solve_kernel(_lib.SDK_KERNELS["plane"])
    yield solver
    solver.lib.sdk_set_plane_tuning(-1, -1, -1, -1)
    solver.lib.sdk_set_solve_kernel(prev)


@pytest.mark.parametrize("order", ["gen", "node"])
def test_one_batch_vs_oracle(plane_kernel, batch2049, order):
    solver = plane_kernel
    p, _, want = batch2049
    solver.stats(reset=True)
    sols, st = solver.solve(torch.from_numpy(p).cuda(), order=order, grid_waves=1)
    assert np.array_equal(st.cpu().numpy(), want[order][1])
    assert np.array_equal(sols.cpu().numpy(), want[order][0])
    s = solver.stats()
    assert s["guesses"] > 2049 and s["sweeps"] > 10 * 2049  # the lanes searched


@pytest.mark.parametrize("order", ["gen", "node"])
def test_one_batch_tail_pool(plane_kernel, batch2049, order):
    """The same input through tail mode 2: the waves' last boards go to the
    XCD pool as records (planes, depth, stack line, mode) and continue on the
    wave-wide solver from lane-written stack lines."""
    solver = plane_kernel
    p, _, want = batch2049
    for tail in (8, 40):
        assert solver.lib.sdk_set_plane_tuning(-1, tail, 2, -1) == 0
        sols, st = solver.solve(torch.from_numpy(p).cuda(), order=order, grid_waves=1)
        assert np.array_equal(st.cpu().numpy(), want[order][1]), tail
        assert np.array_equal(sols.cpu().numpy(), want[order][0]), tail


def test_several_batches_vs_oracle(plane_kernel):
    """sdk_solve_batches over three batches of 700, 64 and 1 301 boards of the
    same mix."""
    solver = plane_kernel
    parts = [_mix(n, 50 + i) for i, n in enumerate((700, 64, 1301))]
    batches = [torch.from_numpy(p).cuda() for p, _ in parts]
    outs = [torch.full_like(b, 0xEE) for b in batches]
    sts = [torch.full((b.shape[0],), 77, dtype=torch.int32, device=b.device) for b in batches]
    solver.stats(reset=True)
    got = solver.solve_batches(batches, outs, sts, grid_waves=1)
    torch.cuda.synchronize()
    for (p, special), (s, t) in zip(parts, got):
        want, wst = _want(p, special, "gen")
        assert np.array_equal(t.cpu().numpy(), wst)
        assert np.array_equal(s.cpu().numpy(), want)
    assert solver.stats()["finished"] == 700 + 64 + 1301
    solver.verify()


def test_refilled_lanes_vs_oracle(plane_kernel):
    """More boards than a grid of one wave per SIMD has lanes, so the last
    ones arrive by chunk-record refills into lanes that carried another
    board's und / nd: those boards and a sample of the first against the
    oracle, and every answer a completion of its (unique-completion) puzzle."""
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    solver = plane_kernel
    lanes = solver.lib.sdk_device_cu_count() * 4 * 64
    n = lanes + 3001
    p = torch.cat([hard17_batch(n - 1500, seed=61), hard_search_batch(1500, seed=62)])
    sols, st = solver.solve(p.cuda(), grid_waves=1)
    sols, st, pn = sols.cpu().numpy(), st.cpu().numpy(), p.numpy()
    assert (st == 1).all()
    assert (sols[pn != 0] == pn[pn != 0]).all()
    g = sols.reshape(n, 9, 9).astype(np.int64)
    bits = 1 << g
    full = 0x3FE
    assert (np.bitwise_or.reduce(bits, axis=2) == full).all() and (np.bitwise_or.reduce(bits, axis=1) == full).all()
    boxes = bits.reshape(n, 3, 3, 3, 3).transpose(0, 1, 3, 2, 4).reshape(n, 9, 9)
    assert (np.bitwise_or.reduce(boxes, axis=2) == full).all()
    idx = np.concatenate([np.arange(0, 1000), np.arange(lanes - 200, n)])
    want, cnt = O.solve_unique_batch(pn[idx])
    assert (cnt == 1).all() and np.array_equal(sols[idx], want)
