"""GPU checks of the exact candidates (cand_kernel through
BatchSolver.candidates and the C ABI) against the fixture
tests/golden/cand_cases.json, which the oracle's counter made once per cell
and digit; against the rating's marks; and of gen.make_unique built on them.
Every check is an equality."""
import numpy as np
import pytest
import torch

import cand_cases as K
import count_cases as C
from abi_arena import IN_FILL, OUT_FILL, Arena
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    names, boards, marks, count = K.load_fixture()
    return {"names": names, "boards": boards, "marks": marks, "count": count,
            "is_b": np.array([n.startswith("b_") for n in names])}


def shuffled(fx, n, seed):
    """Fixture indices of n boards in a seeded order, the whole fixture in
    turn before any board repeats, so that a wave's lanes are in different
    phases; past one turn the set-b boards are not repeated a third time (at
    most 40 of them in a batch)."""
    rng = np.random.default_rng(seed)
    k = len(fx["boards"])
    turns = [rng.permutation(k) for _ in range(min(2, -(-n // k)))]
    rest = rng.permutation(np.nonzero(~fx["is_b"])[0])
    idx = np.concatenate(turns + [np.resize(rest, max(0, n - 2 * k))])[:n]
    return rng.permutation(idx) if n > k else idx


def gpu_cand(solver, boards, count=True, **kw):
    d = torch.from_numpy(np.array(boards, dtype=np.uint8)).to(solver.device)
    out = solver.candidates(d, return_count=count, **kw)
    m, c = out if count else (out, None)
    assert m.dtype == torch.int16 and m.shape == (len(d), 81)
    assert c is None or (c.dtype == torch.int32 and c.shape == (len(d),))
    return m.cpu().numpy().view(np.uint16), None if c is None else c.cpu().numpy()


def assert_same(fx, idx, m, c):
    bad = np.nonzero((m != fx["marks"][idx]).any(1) | ((c != fx["count"][idx]) if c is not None else False))[0]
    assert len(bad) == 0, [(fx["names"][idx[i]], None if c is None else int(c[i]), int(fx["count"][idx[i]]),
                            int((m[i] != fx["marks"][idx[i]]).sum())) for i in bad[:8]]


@pytest.mark.parametrize("n,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (513, 2)])
def test_fixture_equality(solver, fx, n, max_waves):
    """A partial wave, a wave less a lane, a wave, a wave and a lane; and 513
    boards on two waves, about four boards a lane: claim, refill and drain."""
    idx = shuffled(fx, n, seed=100 + n)
    if n == 513:
        assert fx["is_b"][idx].sum() <= 40 and f"b_{K.HEAVY_B}" in {fx["names"][i] for i in idx}  # the 22 000-pass board
        assert len(set(idx.tolist())) == len(fx["boards"])  # every fixture board
    m, c = gpu_cand(solver, fx["boards"][idx], max_waves=max_waves)
    assert_same(fx, idx, m, c)
    only, _ = gpu_cand(solver, fx["boards"][idx], count=False, max_waves=max_waves)  # d_count = NULL
    assert_same(fx, idx, only, None)


def test_empty_batch_and_arguments(solver):
    m, c = solver.candidates(torch.zeros((0, 81), dtype=torch.uint8), return_count=True)
    assert m.shape == (0, 81) and c.shape == (0,)
    with pytest.raises(ValueError):
        solver.candidates(torch.zeros((1, 81), dtype=torch.uint8), max_waves=-1)


def test_back_to_back_calls_share_one_scratch(solver, fx):
    """Two calls on one stream with the one cached scratch, nothing between
    them, then a 65-board call: the queue head is re-armed in stream order.
    The solve workspace is not involved (verify() is clean)."""
    idx = shuffled(fx, 130, seed=7)
    d = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    solver.candidates(d)  # the scratch is sized now
    a = solver.candidates(d, return_count=True)
    b = solver.candidates(d, return_count=True)
    e = solver.candidates(d[:65], return_count=True)
    for (m, c), sel in ((a, idx), (b, idx), (e, idx[:65])):
        assert_same(fx, sel, m.cpu().numpy().view(np.uint16), c.cpu().numpy())
    solver.verify()


def test_byte_offset_input_and_guard_bytes(solver, fx):
    """d_boards at an odd address inside an arena of bytes > 9; d_marks (2-byte
    aligned, not 4), d_count and the scratch inside arenas whose other bytes
    must not change; the inputs unchanged."""
    n = 67
    idx = shuffled(fx, n, seed=41)
    dev, L = solver.device, solver.lib
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 15), Arena(dev, OUT_FILL, 1 << 16), Arena(dev, OUT_FILL, 1 << 21)
    d = inputs.boards(n, offset_mod4=1, name="boards")
    d.copy_(torch.from_numpy(fx["boards"][idx]))
    need = int(L.sdk_candidates_scratch_bytes(n, 0))
    assert need == 256 + 2 * 64 * 83 * 128
    marks = outs.carve(162 * n, offset_mod4=2, name="marks")
    count = outs.carve(4 * n, itemsize=4, name="count")
    sc = scratch.carve(need, name="scratch", align=8)
    assert d.data_ptr() % 2 == 1 and marks.data_ptr() % 4 == 2
    with torch.cuda.device(dev):
        st = int(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.sdk_candidates_batch(d.data_ptr(), marks.data_ptr(), count.data_ptr(), n, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_same(fx, idx, marks.cpu().numpy().view(np.uint16).reshape(n, 81), count.cpu().numpy())
        marks2 = outs.carve(162 * n, offset_mod4=2, name="marks2")
        rc = L.sdk_candidates_batch(d.data_ptr(), marks2.data_ptr(), None, n, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_same(fx, idx, marks2.cpu().numpy().view(np.uint16).reshape(n, 81), None)
        for kw in ((d.data_ptr(), marks.data_ptr() + 1, count.data_ptr(), n, sc.data_ptr(), need, 0, st),
                   (d.data_ptr(), marks.data_ptr(), count.data_ptr(), n, sc.data_ptr(), need - 1, 0, st)):
            assert L.sdk_candidates_batch(*kw) == -2
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), fx["boards"][idx])


def test_candidates_within_the_rating_marks(solver, fx):
    """The rating's marks are a superset of the truth on every board with a
    completion, and the truth itself where the rating is 1..4."""
    sel = np.nonzero(fx["count"] >= 1)[0]
    d = torch.from_numpy(fx["boards"][sel]).to(solver.device)
    rating, rate_marks = solver.rate(d, return_marks=True)
    cand = solver.candidates(d)
    assert cand.cpu().numpy().view(np.uint16).tolist() == fx["marks"][sel].tolist()
    assert not bool((cand & ~rate_marks).any())
    solved = (rating >= 1) & (rating <= 4)
    assert int(solved.sum()) >= 32 and int((~solved).sum()) >= 32
    assert torch.equal(cand[solved], rate_marks[solved])
    assert bool((rating[~solved] == 5).all())  # a board with a completion is never dead


def _restated(board):
    """make_unique's loop on one board with the oracle's per-candidate marks."""
    b, added = np.array(board, dtype=np.uint8), 0
    while True:
        marks, _ = K.oracle_marks(b)
        width = [bin(m).count("1") for m in marks]
        if max(width) < 2:
            return b, added
        cell = width.index(max(width))
        b[cell] = (marks[cell] & -marks[cell]).bit_length()
        added += 1


def test_make_unique(solver):
    from sudoku_solver_distributed_amd.gen import make_unique
    s = C.sets()
    boards = np.concatenate([s["d"][:16], np.zeros((1, 81), np.uint8), s["a"][:8], s["e"][:8], s["f"][4:5]])
    puzzles, added = make_unique(torch.from_numpy(boards))
    assert puzzles.dtype == torch.uint8 and puzzles.shape == boards.shape
    assert added.dtype == torch.int32 and added.shape == (len(boards),)
    p, a = puzzles.cpu().numpy(), added.cpu().numpy()
    given = boards != 0
    assert np.array_equal(p[given], boards[given])  # the givens are kept
    assert np.array_equal(a, (p != 0).sum(1) - given.sum(1))
    for i in range(17):
        assert O.count_solutions(p[i], 2) == 1, i
    assert (a[:16] > 0).sum() >= 8 and a[16] >= 17
    assert np.array_equal(p[17:], boards[17:]) and not a[17:].any()  # one completion, none, a byte of 10
    for i in range(4):
        want, want_added = _restated(boards[i])
        assert np.array_equal(p[i], want) and a[i] == want_added, i
