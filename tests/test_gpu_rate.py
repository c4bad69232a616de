"""GPU checks of the puzzle rating (rate_kernel and rate_trial_kernel through
BatchSolver.rate and the C ABI) against the fixture tests/golden/rate_cases.json,
which the plain-Python definition of rate_cases.py made, against the rest of the
library, and of the rated generator built on it.  Every check is an equality."""
import numpy as np
import pytest
import torch

import rate_cases as R
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # a partial wave, a wave less a lane, a wave, a wave and a lane, several claims


@pytest.fixture(scope="module")
def fx():
    names, boards, rating, opens, marks = R.load_fixture()
    for a in (boards, rating, opens, marks):
        a.setflags(write=False)
    return {"names": names, "boards": boards, "rating": rating, "open": opens, "marks": marks}


def gpu_rate(solver, boards, max_level=4):
    r, o, m = solver.rate(torch.from_numpy(np.array(boards, dtype=np.uint8)), max_level=max_level, return_open=True,
                          return_marks=True)
    return r.cpu().numpy(), o.cpu().numpy(), m.cpu().numpy().view(np.uint16)


def assert_same(names, got, want):
    r, o, m = got
    rating, opens, marks = want
    bad = np.nonzero((r != rating) | (o != opens).any(1) | (m != marks).any(1))[0]
    assert len(bad) == 0, [(names[i], int(r[i]), int(rating[i]), o[i].tolist(), opens[i].tolist(),
                            int((m[i] != marks[i]).sum())) for i in bad[:8]]


def mix(fx, n, seed=0):
    """Fixture indices of n boards drawn cyclically from a mix of all ratings
    (rating k at positions = k mod 6), so a wave's lanes end on different levels."""
    by = [np.nonzero(fx["rating"] == k)[0] for k in range(6)]
    rng = np.random.default_rng(seed)
    by = [rng.permutation(b) for b in by]
    return np.array([by[j % 6][(j // 6) % len(by[j % 6])] for j in range(n)])


def test_fixture_at_level_4(solver, fx):
    """Every fixture board, with all outputs and with each optional output
    left out."""
    got = gpu_rate(solver, fx["boards"])
    assert_same(fx["names"], got, (fx["rating"], fx["open"], fx["marks"]))
    d = torch.from_numpy(fx["boards"].copy()).to(solver.device)
    only = solver.rate(d)
    r, o = solver.rate(d, return_open=True)
    r2, m = solver.rate(d, return_marks=True)
    for t in (only, r, r2):
        assert np.array_equal(t.cpu().numpy(), fx["rating"])
    assert np.array_equal(o.cpu().numpy(), fx["open"])
    assert np.array_equal(m.cpu().numpy().view(np.uint16), fx["marks"])
    assert only.dtype == torch.int32 and o.dtype == torch.int32 and m.dtype == torch.int16 and m.shape == (len(d), 81)


@pytest.mark.parametrize("max_level", [1, 2, 3])
def test_fixture_at_lower_levels(solver, fx, max_level):
    """rating, open and SDK_RATE_NOT_RUN as the definition derives them from
    the level-4 answers; marks where those hold them, and against the host
    build of rate.h (test_rate_host.py checks it against the definition) on
    every board."""
    import test_rate_host as H
    from native_build import host_lib
    r, o, m = gpu_rate(solver, fx["boards"], max_level)
    for i in range(len(r)):
        want_r, want_o, known = R.at_level(fx["rating"][i], fx["open"][i], max_level)
        assert (int(r[i]), o[i].tolist()) == (want_r, want_o), fx["names"][i]
        if known:
            assert np.array_equal(m[i], fx["marks"][i]), fx["names"][i]
    assert_same(fx["names"], (r, o, m), H.rate(host_lib("rate_host"), fx["boards"], max_level))
    only = solver.rate(torch.from_numpy(fx["boards"].copy()), max_level=max_level)
    assert np.array_equal(only.cpu().numpy(), r)


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(solver, fx, n):
    idx = mix(fx, n, seed=n)
    assert n < 6 or {int(v) for v in fx["rating"][idx]} == {0, 1, 2, 3, 4, 5}
    for max_level in (4, 3):
        got = gpu_rate(solver, fx["boards"][idx], max_level)
        if max_level == 4:
            assert_same([fx["names"][i] for i in idx], got, (fx["rating"][idx], fx["open"][idx], fx["marks"][idx]))
        else:
            want = [R.at_level(fx["rating"][i], fx["open"][i], 3)[:2] for i in idx]
            assert [(int(a), b.tolist()) for a, b in zip(got[0], got[1])] == want


def test_every_board_through_the_trial_kernel(solver, fx):
    idx = np.nonzero(fx["rating"] == 4)[0][:130]
    assert len(idx) == 130
    assert_same([fx["names"][i] for i in idx], gpu_rate(solver, fx["boards"][idx]),
                (fx["rating"][idx], fx["open"][idx], fx["marks"][idx]))


def test_no_board_through_the_trial_kernel(solver, fx):
    idx = np.resize(np.nonzero(fx["rating"] == 1)[0], 130)
    assert_same([fx["names"][i] for i in idx], gpu_rate(solver, fx["boards"][idx]),
                (fx["rating"][idx], fx["open"][idx], fx["marks"][idx]))


def test_empty_board_takes_twelve_chunks(solver):
    """729 candidates: 12 chunks of 64 in one round, none of them dead."""
    r, o, m = gpu_rate(solver, np.zeros((3, 81), dtype=np.uint8))
    assert r.tolist() == [5] * 3 and (o == 81).all() and (m == 0x1FF).all()
    assert solver.rate(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0,)
    for bad in (0, 5):
        with pytest.raises(ValueError):
            solver.rate(torch.zeros((1, 81), dtype=torch.uint8), max_level=bad)


def _abi_call(solver, d_boards, n, max_level, arena, scratch_arena, opens=True, marks=True):
    """sdk_rate_batch on buffers carved from guarded arenas; returns the
    outputs' views and the return code."""
    L = solver.lib
    need = int(L.sdk_rate_scratch_bytes(n, max_level))
    rating = arena.carve(4 * n, itemsize=4, name="rating")
    o = arena.carve(16 * n, itemsize=4, name="open") if opens else None
    m = arena.carve(162 * n, offset_mod4=2, name="marks") if marks else None  # 2-byte aligned, not 4
    sc = scratch_arena.carve(need, name="scratch", align=8)
    with torch.cuda.device(solver.device):
        rc = L.sdk_rate_batch(d_boards.data_ptr(), rating.data_ptr(), o.data_ptr() if opens else None,
                              m.data_ptr() if marks else None, n, max_level, sc.data_ptr(), need,
                              int(torch.cuda.current_stream(solver.device).cuda_stream))
    torch.cuda.synchronize(solver.device)
    return rc, rating, o, m


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_byte_offset_inputs_and_guard_bytes(solver, fx, offset):
    """d_boards at every address mod 4 inside an arena of bytes > 9; the three
    outputs and the scratch inside arenas whose other bytes must not change;
    the inputs unchanged."""
    n = 131
    idx = mix(fx, n, seed=40 + offset)
    dev = solver.device
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 16), Arena(dev, OUT_FILL, 1 << 17), Arena(dev, OUT_FILL, 1 << 14)
    d = inputs.boards(n, offset_mod4=offset, name="boards")
    d.copy_(torch.from_numpy(fx["boards"][idx]))
    assert d.data_ptr() % 4 == offset
    rc, rating, o, m = _abi_call(solver, d, n, 4, outs, scratch)
    assert rc == 0 and m.data_ptr() % 4 == 2
    got = (rating.cpu().numpy(), o.cpu().numpy().reshape(n, 4), m.cpu().numpy().view(np.uint16).reshape(n, 81))
    assert_same([fx["names"][i] for i in idx], got, (fx["rating"][idx], fx["open"][idx], fx["marks"][idx]))
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), fx["boards"][idx])
    # the optional outputs left out, at max_level 3: nothing but the ratings is written
    outs2 = Arena(dev, OUT_FILL, 1 << 14)
    rc, rating, _, _ = _abi_call(solver, d, n, 3, outs2, scratch, opens=False, marks=False)
    assert rc == 0
    assert rating.cpu().numpy().tolist() == [R.at_level(fx["rating"][i], fx["open"][i], 3)[0] for i in idx]
    for a in (inputs, outs2, scratch):
        a.assert_guards()


def test_bad_arguments_launch_nothing(solver, fx):
    """Every refused call returns -2 and leaves the outputs and the scratch as
    they were."""
    n = 64
    dev = solver.device
    L = solver.lib
    outs = Arena(dev, OUT_FILL, 1 << 16)
    d = torch.from_numpy(fx["boards"][:n].copy()).to(dev)
    rating = outs.carve(4 * n, itemsize=4, name="rating")
    o = outs.carve(16 * n, itemsize=4, name="open")
    m = outs.carve(162 * n, name="marks")
    need = int(L.sdk_rate_scratch_bytes(n, 4))
    sc = outs.carve(need, name="scratch", align=8)
    args = lambda **kw: [kw.get(k, v) for k, v in (("b", d.data_ptr()), ("r", rating.data_ptr()), ("o", o.data_ptr()),
                                                   ("m", m.data_ptr()), ("n", n), ("lvl", 4), ("sc", sc.data_ptr()),
                                                   ("bytes", need), ("st", None))]
    with torch.cuda.device(dev):
        for kw in ({"lvl": 0}, {"lvl": 5}, {"n": -1}, {"b": None}, {"r": None}, {"sc": None}, {"bytes": need - 1},
                   {"m": m.data_ptr() + 1}, {"o": o.data_ptr() + 2}):
            assert L.sdk_rate_batch(*args(**kw)) == -2, kw
    torch.cuda.synchronize(dev)
    assert bool((outs.buf == OUT_FILL).all())


def test_back_to_back_calls_share_one_scratch(solver, fx):
    """Two calls on one stream with the one cached scratch, nothing between
    them: the second call's counters are re-armed in stream order."""
    idx = mix(fx, 257, seed=9)
    d = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    solver.rate(d)  # the scratch is sized now
    a = solver.rate(d, return_open=True)
    b = solver.rate(d, return_open=True)
    c = solver.rate(d[:65], max_level=3)
    e = solver.rate(d)
    for r, o in (a, b):
        assert np.array_equal(r.cpu().numpy(), fx["rating"][idx]) and np.array_equal(o.cpu().numpy(), fx["open"][idx])
    assert c.cpu().numpy().tolist() == [R.at_level(fx["rating"][i], fx["open"][i], 3)[0] for i in idx[:65]]
    assert np.array_equal(e.cpu().numpy(), fx["rating"][idx])


def test_ratings_agree_with_count_and_solve(solver, fx):
    """rating 1..4 => exactly one completion, and the marks' single bits are
    solve's grid; rating 0 => no completion."""
    b = torch.from_numpy(fx["boards"].copy()).to(solver.device)
    r, m = solver.rate(b, return_marks=True)
    cnt = solver.count_solutions(b, limit=2)
    solved = (r >= 1) & (r <= 4)
    assert int(solved.sum()) > 300 and int((r == 0).sum()) >= 8
    assert bool((cnt[solved] == 1).all()) and bool((cnt[r == 0] == 0).all())
    grid, st = solver.solve(b[solved])
    assert bool((st == 1).all())
    assert torch.equal(m[solved].to(torch.int64), torch.ones_like(grid, dtype=torch.int64) << (grid.to(torch.int64) - 1))


def test_symmetry_images_keep_rating_and_open(solver, fx):
    from sudoku_solver_distributed_amd.gen import _symmetry_images
    idx = mix(fx, 64, seed=77)
    rng = np.random.default_rng(5)
    images = np.stack([_symmetry_images(fx["boards"][i:i + 1], 1, seed=int(rng.integers(1 << 30)))[0] for i in idx])
    r, o, m = gpu_rate(solver, images)
    assert np.array_equal(r, fx["rating"][idx]) and np.array_equal(o, fx["open"][idx])
    count = lambda a: np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=1).sum(1)
    assert np.array_equal(count(m), count(fx["marks"][idx]))
    # and the marks bit for bit, under symmetries whose maps are known (symmetry_cases.py)
    import symmetry_cases as S
    syms = [S.random_symmetry(rng) for _ in idx]
    r, o, m = gpu_rate(solver, np.stack([S.image_board(fx["boards"][i], s) for i, s in zip(idx, syms)]))
    assert np.array_equal(r, fx["rating"][idx]) and np.array_equal(o, fx["open"][idx])
    assert np.array_equal(m, np.stack([S.image_marks(fx["marks"][i], s) for i, s in zip(idx, syms)]))


def test_rated_batch(solver):
    from sudoku_solver_distributed_amd.gen import rated_batch, unique_batch
    puzzles, rating, full = rated_batch(64, seed=1, return_solutions=True)
    want, want_full = unique_batch(64, seed=1, return_solutions=True)
    assert torch.equal(puzzles, want) and torch.equal(full, want_full)
    assert rating.shape == (64,) and rating.dtype == torch.int32
    assert bool(((rating >= 1) & (rating <= 5)).all())
    assert torch.equal(rating, solver.rate(want))
    kinds = sorted({int(v) for v in rating})
    keep = kinds[:1] + kinds[-1:]
    sub, sub_rating = rated_batch(64, seed=1, ratings=keep)
    mask = torch.isin(rating, torch.tensor(keep, dtype=torch.int32, device=rating.device))
    assert torch.equal(sub, want[mask]) and torch.equal(sub_rating, rating[mask]) and 0 < len(sub) <= 64
    none, none_rating = rated_batch(64, seed=1, ratings=[0])
    assert none.shape == (0, 81) and none_rating.shape == (0,)
