"""GPU checks of the minimisation (min_kernel through BatchSolver.minimize and
the C ABI) against the fixture tests/golden/min_cases.json, which the oracle's
counter made as the plain loop of the definition; of gen.unique_batch's fused
path against its 81-round loop; and of the buffer contracts.  Every check is
an equality."""
import numpy as np
import pytest
import torch

import count_cases as C
import min_cases as M
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu

# one call has one mode, one max_empty and one order array: the fixture's cases
# by call (a NULL order is turn t -> cell t, which the "null" group passes as
# NULL and the others as the row 0..80)
GROUPS = ("greedy81", "greedy40", "probe", "null")


@pytest.fixture(scope="module")
def fx():
    f = dict(M.load_fixture())
    greedy = f["mode"] == M.GREEDY
    f["groups"] = {"greedy81": np.nonzero(greedy & (f["max_empty"] == 81))[0],
                   "greedy40": np.nonzero(greedy & (f["max_empty"] == 40))[0],
                   "probe": np.nonzero(f["mode"] == M.PROBE)[0],
                   "null": np.nonzero(greedy & (f["max_empty"] == 81) & ~f["has_order"])[0]}
    return f


def shuffled(fx, group, n, seed):
    """Fixture indices of n cases of a group in a seeded order, the whole group
    in turn before any case repeats, so that a wave's lanes are in different
    turns and phases."""
    rng = np.random.default_rng(seed)
    src = fx["groups"][group]
    return np.concatenate([rng.permutation(src) for _ in range(-(-n // len(src)))])[:n]


def gpu_min(solver, fx, group, idx, removed=True, **kw):
    d = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    order = None if group == "null" else torch.from_numpy(fx["order"][idx]).to(solver.device)
    res = solver.minimize(d, order, max_empty=40 if group == "greedy40" else 81, probe=group == "probe",
                          return_removed=removed, **kw)
    out, status = res[0], res[1]
    assert out.dtype == torch.uint8 and out.shape == (len(idx), 81)
    assert status.dtype == torch.int32 and status.shape == (len(idx),)
    assert not removed or (res[2].dtype == torch.int32 and res[2].shape == (len(idx),))
    return out.cpu().numpy(), status.cpu().numpy(), res[2].cpu().numpy() if removed else None


def assert_same(fx, idx, out, status, removed):
    bad = np.nonzero((out != fx["out"][idx]).any(1) | (status != fx["status"][idx]) |
                     ((removed != fx["removed"][idx]) if removed is not None else False))[0]
    assert len(bad) == 0, [(fx["names"][idx[i]], int(status[i]), int(fx["status"][idx[i]]),
                            None if removed is None else int(removed[i]), int(fx["removed"][idx[i]]))
                           for i in bad[:8]]


@pytest.mark.parametrize("n,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (513, 2)])
def test_fixture_equality(solver, fx, n, max_waves):
    """A partial wave, a wave less a lane, a wave, a wave and a lane; and 513
    boards on two waves, about four boards a lane: claim, refill and drain.
    Each of the fixture's four kinds of call at that size."""
    seen = set()
    for g, group in enumerate(GROUPS):
        idx = shuffled(fx, group, n, seed=100 * g + n)
        seen.update(idx.tolist())
        assert_same(fx, idx, *gpu_min(solver, fx, group, idx, max_waves=max_waves))
        out, status, none = gpu_min(solver, fx, group, idx, removed=False, max_waves=max_waves)  # d_removed = NULL
        assert_same(fx, idx, out, status, None)
    if n == 513:
        assert len(seen) == len(fx["names"])  # every fixture case


def test_fused_unique_batch_equals_the_81_rounds(solver):
    from sudoku_solver_distributed_amd.gen import unique_batch
    for empty in (81, 40):
        p0, f0 = unique_batch(32, empty, seed=5, return_solutions=True)
        p1, f1 = unique_batch(32, empty, seed=5, return_solutions=True, fused=True)
        assert torch.equal(p0, p1) and torch.equal(f0, f1), empty
        assert p1.dtype == torch.uint8 and bool(((p1 == 0).sum(1) <= empty).all())
        assert torch.equal(unique_batch(32, empty, seed=5, fused=True), p0)  # without the full grids


def test_chaining_after_make_unique(solver):
    """make_unique's proper puzzles minimised: status 1, and nothing left that
    probe could remove."""
    from sudoku_solver_distributed_amd.gen import make_unique
    proper, _ = make_unique(torch.from_numpy(C.sets()["d"][:16].copy()))
    small, status, removed = solver.minimize(proper, return_removed=True)
    assert bool((status == 1).all()) and bool((removed > 0).any())
    assert torch.equal((small == 0).sum(1) - (proper == 0).sum(1), removed.to(torch.int64))
    again, status2, removed2 = solver.minimize(small, probe=True, return_removed=True)
    assert bool((status2 == 1).all()) and not bool(removed2.any()) and torch.equal(again, small)


def test_back_to_back_calls_share_one_scratch(solver, fx):
    """Two calls on one stream with the one cached scratch, nothing between
    them, then a 65-board call: the queue head is re-armed in stream order.
    The solve workspace is not involved (verify() is clean)."""
    idx = shuffled(fx, "greedy81", 130, seed=7)
    d = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    order = torch.from_numpy(fx["order"][idx]).to(solver.device)
    solver.minimize(d, order)  # the scratch is sized now
    a = solver.minimize(d, order, return_removed=True)
    b = solver.minimize(d, order, return_removed=True)
    e = solver.minimize(d[:65], order[:65], return_removed=True)
    for res, sel in ((a, idx), (b, idx), (e, idx[:65])):
        assert_same(fx, sel, *(t.cpu().numpy() for t in res))
    solver.verify()


def test_byte_offset_buffers_and_guard_bytes(solver, fx):
    """d_boards and d_order at odd addresses inside an arena of bytes > 9;
    d_out at an odd address, d_status, d_removed and the scratch inside arenas
    whose other bytes must not change; the inputs unchanged."""
    n = 67
    idx = shuffled(fx, "greedy81", n, seed=41)
    dev, L = solver.device, solver.lib
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 15), Arena(dev, OUT_FILL, 1 << 16), Arena(dev, OUT_FILL, 1 << 21)
    d = inputs.boards(n, offset_mod4=1, name="boards")
    d.copy_(torch.from_numpy(fx["boards"][idx]))
    order = inputs.boards(n, offset_mod4=3, name="order")
    order.copy_(torch.from_numpy(fx["order"][idx]))
    need = int(L.sdk_minimize_scratch_bytes(n, 0))
    assert need == 256 + 2 * 64 * M.MIN_LEVELS * 128
    out = outs.boards(n, offset_mod4=3, name="out")
    status = outs.carve(4 * n, itemsize=4, name="status")
    removed = outs.carve(4 * n, itemsize=4, name="removed")
    sc = scratch.carve(need, name="scratch", align=8)
    assert d.data_ptr() % 2 == 1 and order.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    with torch.cuda.device(dev):
        st = int(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.sdk_minimize_batch(d.data_ptr(), order.data_ptr(), out.data_ptr(), status.data_ptr(), removed.data_ptr(),
                                  n, M.GREEDY, 81, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_same(fx, idx, out.cpu().numpy(), status.cpu().numpy(), removed.cpu().numpy())
        out2 = outs.boards(n, offset_mod4=2, name="out2")
        status2 = outs.carve(4 * n, itemsize=4, name="status2")
        rc = L.sdk_minimize_batch(d.data_ptr(), None, out2.data_ptr(), status2.data_ptr(), None,
                                  n, M.PROBE, 0, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        probe = np.array([M.oracle_minimize(fx["boards"][k], None, M.PROBE, 81)[0] for k in idx[:8]])
        assert np.array_equal(out2.cpu().numpy()[:8], probe)
        assert np.array_equal(status2.cpu().numpy(), fx["status"][idx])
        for kw in ((d.data_ptr(), None, out.data_ptr(), status.data_ptr() + 2, None, n, 0, 81, sc.data_ptr(), need, 0, st),
                   (d.data_ptr(), None, out.data_ptr(), status.data_ptr(), None, n, 0, 81, sc.data_ptr() + 4, need, 0, st),
                   (d.data_ptr(), None, out.data_ptr(), status.data_ptr(), None, n, 0, 81, sc.data_ptr(), need - 1, 0, st),
                   (d.data_ptr(), None, d.data_ptr(), status.data_ptr(), None, n, 0, 81, sc.data_ptr(), need, 0, st)):
            assert L.sdk_minimize_batch(*kw) == -2
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), fx["boards"][idx]) and np.array_equal(order.cpu().numpy(), fx["order"][idx])


def test_empty_batch_and_arguments(solver):
    out, status, removed = solver.minimize(torch.zeros((0, 81), dtype=torch.uint8), return_removed=True)
    assert out.shape == (0, 81) and status.shape == (0,) and removed.shape == (0,)
    one = torch.zeros((1, 81), dtype=torch.uint8)
    for kw in ({"max_waves": -1}, {"max_empty": -1}, {"max_empty": 82},
               {"order": torch.zeros((1, 80), dtype=torch.uint8)}, {"order": torch.zeros((2, 81), dtype=torch.uint8)}):
        with pytest.raises(ValueError):
            solver.minimize(one, **kw)
