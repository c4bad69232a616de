"""GPU checks of the random completion (sample_kernel through
BatchSolver.sample / random_grids and the C ABI) against the fixture
tests/golden/sample_cases.json, which the host build of the same header made
(test_sample_host.py re-derives it and checks it against the oracle); of
gen.unique_batch's grids="random" path; and of the buffer contracts.  Every
check is an equality."""
import numpy as np
import pytest
import torch

import sample_cases as S
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return S.load_fixture()


@pytest.fixture(scope="module")
def rows():
    return S.rows()


def gpu_sample(solver, boards, **kw):
    d = None if boards is None else torch.from_numpy(np.array(boards, dtype=np.uint8)).to(solver.device)
    out, status = solver.sample(d, **kw)
    assert out.dtype == torch.uint8 and status.dtype == torch.int32 and out.shape == (status.shape[0], 81)
    return out.cpu().numpy(), status.cpu().numpy()


def assert_rows(rows, idx, out, status):
    bad = np.nonzero((out != rows["out"][idx]).any(1) | (status != rows["status"][idx]))[0]
    assert len(bad) == 0, [(int(i), rows["names"][idx[i]], int(status[i]), int(rows["status"][idx[i]])) for i in bad[:8]]


@pytest.mark.parametrize("n,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (513, 2)])
def test_fixture_equality(solver, rows, n, max_waves):
    """A partial wave, a wave less a lane, a wave, a wave and a lane; and 513
    items on two waves, about four items a lane: claim, refill and drain.
    Three calls a size (sample_cases.mixed_call): the fixture's rows mixed in
    a seeded order, each key-bound row where its key falls, so that a wave's
    lanes are at different depths and unique, ambiguous, dead and invalid
    boards sit side by side."""
    seen = set()
    for turn in range(3):
        idx = S.mixed_call(n, turn, seed=100 * turn + n)
        seen.update(idx.tolist())
        out, status = gpu_sample(solver, rows["board"][idx], seed=S.SEED, max_waves=max_waves)
        assert_rows(rows, idx, out, status)
    if n == 513:
        assert len(seen) == len(rows["names"]) == 269  # every fixture row


def test_groups_as_recorded(solver, fx):
    """Every group as the fixture made it: its per_board and first_key, the z
    rows from NULL boards."""
    for name, g in fx.items():
        out, status = gpu_sample(solver, None if g["null"] else g["boards"], seed=g["seed"],
                                 per_board=len(g["out"]) if g["null"] else g["per_board"], first_key=g["first_key"])
        assert np.array_equal(status, g["status"]) and np.array_equal(out, g["out"]), name


def test_one_wave_equals_the_full_grid(solver, rows):
    idx = S.mixed_call(300, 1, seed=9)
    a = gpu_sample(solver, rows["board"][idx], seed=77, per_board=2, first_key=5, max_waves=0)
    b = gpu_sample(solver, rows["board"][idx], seed=77, per_board=2, first_key=5, max_waves=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_null_boards_equal_zero_boards(solver):
    null = gpu_sample(solver, None, seed=3, per_board=200, first_key=40)
    zero = gpu_sample(solver, np.zeros((200, 81), dtype=np.uint8), seed=3, first_key=40)
    assert (null[1] == 1).all() and np.array_equal(null[0], zero[0]) and np.array_equal(null[1], zero[1])
    one = gpu_sample(solver, np.zeros((1, 81), dtype=np.uint8), seed=3, per_board=200, first_key=40)
    assert np.array_equal(one[0], null[0])


def test_key_split_identity(solver, fx):
    b = np.concatenate([fx["b"]["boards"], fx["d"]["boards"], fx["f"]["boards"]])
    for per_board in (1, 3):
        whole = gpu_sample(solver, b, seed=5, per_board=per_board, first_key=1000)
        for k in (1, 37, 68):
            tail = gpu_sample(solver, b[k:], seed=5, per_board=per_board, first_key=1000 + k * per_board)
            assert np.array_equal(tail[0], whole[0][k * per_board:]) and np.array_equal(tail[1], whole[1][k * per_board:])
    one = gpu_sample(solver, fx["b"]["boards"], seed=5)
    other = gpu_sample(solver, fx["b"]["boards"], seed=6)
    assert (one[0] != other[0]).any(1).sum() >= 1
    hi = solver.random_grids(2, seed=5, first_key=S.M64)  # keys wrap mod 2^64
    assert torch.equal(hi[1], solver.random_grids(1, seed=5)[0])


def test_random_grids(solver, fx):
    g = solver.random_grids(4608, seed=1)
    assert g.dtype == torch.uint8 and g.shape == (4608, 81)
    assert bool(solver.check(g).all())
    assert torch.unique(g, dim=0).shape[0] == 4608
    assert np.array_equal(g[:64].cpu().numpy(), fx["z"]["out"])
    assert fx["z"]["seed"] == 1 and fx["z"]["first_key"] == 0
    from sudoku_solver_distributed_amd.gen import random_grids
    assert torch.equal(random_grids(100, seed=1), g[:100])
    assert torch.equal(solver.random_grids(100, seed=1, first_key=4508), g[4508:])
    a, b = random_grids(8), random_grids(8)  # a seed drawn from `random` each
    assert bool(solver.check(torch.cat([a, b])).all()) and not torch.equal(a, b)
    assert solver.random_grids(0).shape == (0, 81)


def test_generator_path(solver):
    from sudoku_solver_distributed_amd.gen import random_grids, rated_batch, unique_batch
    p0, f0 = unique_batch(32, seed=5, grids="random", return_solutions=True)
    p1, f1 = unique_batch(32, seed=5, grids="random", return_solutions=True, fused=True)
    assert torch.equal(p0, p1) and torch.equal(f0, f1)
    assert torch.equal(f1, random_grids(32, 5))
    assert bool((solver.count_solutions(p1, limit=2) == 1).all())
    again, status, removed = solver.minimize(p1, probe=True, return_removed=True)
    assert bool((status == 1).all()) and not bool(removed.any()) and torch.equal(again, p1)
    cnt, first = solver.count_solutions(p1, limit=2, return_first=True)
    assert torch.equal(first, f1)  # the puzzle's one completion is the grid it was cut from
    # "walk" is the path as it was
    assert torch.equal(unique_batch(32, seed=5, grids="walk"), unique_batch(32, seed=5))
    assert torch.equal(unique_batch(32, seed=5, grids="walk", fused=True), unique_batch(32, seed=5, fused=True))
    assert not torch.equal(unique_batch(32, seed=5, fused=True), p1)
    pz, rating, full = rated_batch(32, seed=5, grids="random", return_solutions=True)
    assert torch.equal(pz, p1) and torch.equal(full, f1) and torch.equal(rating, solver.rate(p1))
    with pytest.raises(ValueError):
        unique_batch(4, seed=5, grids="other")


def test_back_to_back_calls_share_one_scratch(solver, rows):
    """Two calls on one stream with the one cached scratch, nothing between
    them, then a 65-item call: the queue head is re-armed in stream order.
    The solve workspace is not involved (verify() is clean)."""
    idx = S.mixed_call(130, 0, seed=7)
    d = torch.from_numpy(rows["board"][idx]).to(solver.device)
    solver.sample(d, seed=S.SEED)  # the scratch is sized now
    a = solver.sample(d, seed=S.SEED)
    b = solver.sample(d, seed=S.SEED)
    e = solver.sample(d[:65], seed=S.SEED)
    for res, sel in ((a, idx), (b, idx), (e, idx[:65])):
        assert_rows(rows, sel, res[0].cpu().numpy(), res[1].cpu().numpy())
    solver.verify()


def test_byte_offset_buffers_and_guard_bytes(solver, rows):
    """d_boards at an odd address inside an arena of bytes > 9; d_out at an odd
    address, d_status and the scratch inside arenas whose other bytes must not
    change; the inputs unchanged; the -2 cases on device pointers."""
    n = 67
    idx = S.mixed_call(n, 2, seed=41)
    dev, L = solver.device, solver.lib
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 15), Arena(dev, OUT_FILL, 1 << 17), Arena(dev, OUT_FILL, 1 << 22)
    d = inputs.boards(n, offset_mod4=1, name="boards")
    d.copy_(torch.from_numpy(rows["board"][idx]))
    need = int(L.sdk_sample_scratch_bytes(n, 0))
    assert need == 256 + 2 * S.WAVE_BYTES
    out = outs.boards(n, offset_mod4=3, name="out")
    status = outs.carve(4 * n, itemsize=4, name="status")
    sc = scratch.carve(need, name="scratch", align=8)
    assert d.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    with torch.cuda.device(dev):
        st = int(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.sdk_sample_batch(d.data_ptr(), out.data_ptr(), status.data_ptr(), n, 1, S.SEED, 0, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_rows(rows, idx, out.cpu().numpy(), status.cpu().numpy())
        # per_board 2 at another pair of offsets, and NULL boards, on the same scratch
        m = 33
        d2 = inputs.boards(m, offset_mod4=2, name="boards2")
        d2.copy_(torch.from_numpy(rows["board"][idx[:m]]))
        out2 = outs.boards(2 * m, offset_mod4=1, name="out2")
        status2 = outs.carve(8 * m, itemsize=4, name="status2")
        rc = L.sdk_sample_batch(d2.data_ptr(), out2.data_ptr(), status2.data_ptr(), m, 2, 9, 70, sc.data_ptr(), need, 0, st)
        out3 = outs.boards(n, offset_mod4=2, name="out3")
        status3 = outs.carve(4 * n, itemsize=4, name="status3")
        rc3 = L.sdk_sample_batch(None, out3.data_ptr(), status3.data_ptr(), 1, n, 9, 70, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0 and rc3 == 0
        want2 = solver.sample(torch.from_numpy(rows["board"][idx[:m]]), seed=9, per_board=2, first_key=70)
        assert torch.equal(out2, want2[0]) and torch.equal(status2, want2[1])
        assert torch.equal(out3, solver.random_grids(n, seed=9, first_key=70)) and bool((status3 == 1).all())
        ok = (d.data_ptr(), out.data_ptr(), status.data_ptr(), n, 1, S.SEED, 0, sc.data_ptr(), need, 0, st)
        for at, value in ((2, status.data_ptr() + 2), (7, sc.data_ptr() + 4), (8, need - 1), (1, d.data_ptr()),
                          (3, -1), (4, 0), (9, -1), (1, None), (2, None), (7, None)):
            bad = list(ok)
            bad[at] = value
            assert L.sdk_sample_batch(*bad) == -2, at
        torch.cuda.synchronize(dev)
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), rows["board"][idx]) and np.array_equal(d2.cpu().numpy(), rows["board"][idx[:m]])
    assert_rows(rows, idx, out.cpu().numpy(), status.cpu().numpy())  # the refused calls wrote nothing


def test_empty_batch_and_arguments(solver):
    out, status = solver.sample(torch.zeros((0, 81), dtype=torch.uint8))
    assert out.shape == (0, 81) and status.shape == (0,)
    one = torch.zeros((1, 81), dtype=torch.uint8)
    for kw in ({"max_waves": -1}, {"per_board": 0}, {"per_board": -3}, {"per_board": 2 ** 31}):
        with pytest.raises(ValueError):
            solver.sample(one, **kw)
    with pytest.raises(ValueError):
        solver.random_grids(-1)
    with pytest.raises(ValueError):
        solver.sample(torch.zeros((1, 80), dtype=torch.uint8))
