"""GPU checks of the unique candidates (uniq_kernel through
BatchSolver.unique_candidates and the C ABI) against the fixture
tests/golden/uniq_cases.json, which the oracle's counter made once per cell
and digit; against the composition from candidates and count_solutions that
the call replaces; and of gen.exchange / gen.exchange_search built on it.
Every check is an equality."""
import numpy as np
import pytest
import torch

import count_cases as C
import uniq_cases as U
from abi_arena import IN_FILL, OUT_FILL, Arena
from oracle import oracle as O
from test_gpu_cand import shuffled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    names, boards, once, marks, count = U.load_fixture()
    return {"names": names, "boards": boards, "once": once, "marks": marks, "count": count,
            "is_b": np.array([n.startswith("b_") for n in names])}


def gpu_uniq(solver, boards, marks=True, count=True, **kw):
    d = torch.from_numpy(np.array(boards, dtype=np.uint8)).to(solver.device)
    out = solver.unique_candidates(d, return_marks=marks, return_count=count, **kw)
    out = list(out) if marks or count else [out]
    o, m, c = out[0], out[1] if marks else None, out[-1] if count else None
    assert o.dtype == torch.int16 and o.shape == (len(d), 81)
    assert m is None or (m.dtype == torch.int16 and m.shape == (len(d), 81))
    assert c is None or (c.dtype == torch.int32 and c.shape == (len(d),))
    return (o.cpu().numpy().view(np.uint16), None if m is None else m.cpu().numpy().view(np.uint16),
            None if c is None else c.cpu().numpy())


def assert_same(fx, idx, o, m, c):
    bad = np.nonzero((o != fx["once"][idx]).any(1) | ((m != fx["marks"][idx]).any(1) if m is not None else False) |
                     ((c != fx["count"][idx]) if c is not None else False))[0]
    assert len(bad) == 0, [(fx["names"][idx[i]], None if c is None else int(c[i]), int(fx["count"][idx[i]]),
                            int((o[i] != fx["once"][idx[i]]).sum())) for i in bad[:8]]


@pytest.mark.parametrize("n,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (513, 2)])
def test_fixture_equality(solver, fx, n, max_waves):
    """A partial wave, a wave less a lane, a wave, a wave and a lane; and 513
    boards on two waves, about four boards a lane: claim, refill and drain.
    With and without d_marks / d_count; marks as candidates() gives them."""
    idx = shuffled(fx, n, seed=100 + n)
    if n == 513:
        assert fx["is_b"][idx].sum() <= 40 and len(set(idx.tolist())) == len(fx["boards"])  # every fixture board
    o, m, c = gpu_uniq(solver, fx["boards"][idx], max_waves=max_waves)
    assert_same(fx, idx, o, m, c)
    only, _, _ = gpu_uniq(solver, fx["boards"][idx], marks=False, count=False, max_waves=max_waves)  # both NULL
    assert_same(fx, idx, only, None, None)
    cand = solver.candidates(torch.from_numpy(fx["boards"][idx]).to(solver.device), max_waves=max_waves)
    assert np.array_equal(cand.cpu().numpy().view(np.uint16), m)


def test_empty_batch_and_arguments(solver):
    o, m, c = solver.unique_candidates(torch.zeros((0, 81), dtype=torch.uint8), return_marks=True, return_count=True)
    assert o.shape == (0, 81) and m.shape == (0, 81) and c.shape == (0,)
    assert solver.unique_candidates(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0, 81)
    with pytest.raises(ValueError):
        solver.unique_candidates(torch.zeros((1, 81), dtype=torch.uint8), max_waves=-1)


def test_back_to_back_calls_share_one_scratch(solver, fx):
    """Two calls on one stream with the one cached scratch, nothing between
    them, then a 65-board call: the queue head is re-armed in stream order.
    The solve workspace is not involved (verify() is clean)."""
    idx = shuffled(fx, 130, seed=7)
    d = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    solver.unique_candidates(d)  # the scratch is sized now
    a = solver.unique_candidates(d, return_marks=True, return_count=True)
    b = solver.unique_candidates(d, return_marks=True, return_count=True)
    e = solver.unique_candidates(d[:65], return_marks=True, return_count=True)
    for (o, m, c), sel in ((a, idx), (b, idx), (e, idx[:65])):
        assert_same(fx, sel, o.cpu().numpy().view(np.uint16), m.cpu().numpy().view(np.uint16), c.cpu().numpy())
    solver.verify()


def test_byte_offset_input_and_guard_bytes(solver, fx):
    """d_boards at an odd address inside an arena of bytes > 9; d_once and
    d_marks (2-byte aligned, not 4), d_count and the scratch (its exact size)
    inside arenas whose other bytes must not change; the inputs unchanged."""
    n = 67
    idx = shuffled(fx, n, seed=41)
    dev, L = solver.device, solver.lib
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 15), Arena(dev, OUT_FILL, 1 << 17), Arena(dev, OUT_FILL, 1 << 21)
    d = inputs.boards(n, offset_mod4=1, name="boards")
    d.copy_(torch.from_numpy(fx["boards"][idx]))
    need = int(L.sdk_unique_candidates_scratch_bytes(n, 0))
    assert need == 256 + 2 * 64 * 85 * 128
    once = outs.carve(162 * n, offset_mod4=2, name="once")
    marks = outs.carve(162 * n, offset_mod4=2, name="marks")
    count = outs.carve(4 * n, itemsize=4, name="count")
    sc = scratch.carve(need, name="scratch", align=8)
    assert d.data_ptr() % 2 == 1 and once.data_ptr() % 4 == 2 and marks.data_ptr() % 4 == 2
    f = L.sdk_unique_candidates_batch
    u16 = lambda t: t.cpu().numpy().view(np.uint16).reshape(n, 81)
    with torch.cuda.device(dev):
        st = int(torch.cuda.current_stream(dev).cuda_stream)
        rc = f(d.data_ptr(), once.data_ptr(), marks.data_ptr(), count.data_ptr(), n, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_same(fx, idx, u16(once), u16(marks), count.cpu().numpy())
        once2 = outs.carve(162 * n, offset_mod4=2, name="once2")
        rc = f(d.data_ptr(), once2.data_ptr(), None, None, n, sc.data_ptr(), need, 0, st)
        torch.cuda.synchronize(dev)
        assert rc == 0
        assert_same(fx, idx, u16(once2), None, None)
        ok = (d.data_ptr(), once.data_ptr(), marks.data_ptr(), count.data_ptr(), n, sc.data_ptr(), need, 0, st)
        for at, value in ((1, once.data_ptr() + 1), (2, marks.data_ptr() + 1), (3, count.data_ptr() + 2),
                          (5, sc.data_ptr() + 4), (6, need - 1)):
            assert f(*ok[:at], value, *ok[at + 1:]) == -2  # a misaligned pointer; a scratch one byte short
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), fx["boards"][idx])


def test_equals_the_composition_it_replaces(solver):
    """Independent of the fixture, 64 boards of set d: every marks bit of an
    empty cell expanded into a board; count_solutions(limit=2) gives 1 exactly
    where the once bit is set and 2 elsewhere."""
    boards = torch.from_numpy(C.sets()["d"][64:128].copy()).to(solver.device)
    once, marks, count = solver.unique_candidates(boards, return_marks=True, return_count=True)
    want_once, want_marks, want_count, counts = U.composed(solver, boards)
    assert bool(((counts == 1) | (counts == 2)).all()) and int((counts == 1).sum()) > 64 and int((counts == 2).sum()) > 64
    assert torch.equal(marks, want_marks) and torch.equal(count, want_count)
    assert torch.equal(once, want_once)


def _popcount(t):
    t = t.to(torch.int32)
    return int(sum(((t >> d) & 1).sum() for d in range(9)))


def test_symmetry_images_have_as_many_bits(solver, fx):
    """16 boards with several completions and their gen.apply_symmetry images:
    the total popcounts of once and of marks are equal, and once and marks are
    the images of the fixture's, bit for bit (symmetry_cases.from_number)."""
    import symmetry_cases as S
    from sudoku_solver_distributed_amd.gen import apply_symmetry
    sel = np.nonzero((fx["count"] == 2) & (fx["once"] != 0).any(1))[0][:16]
    assert len(sel) == 16
    sym = np.random.default_rng(5).integers(0, 2 * 1296 * 1296, size=16)
    images, maps = apply_symmetry(fx["boards"][sel], sym)
    assert (images != fx["boards"][sel]).any(1).all()
    o, m, c = gpu_uniq(solver, images)
    for k, i in enumerate(sel):
        assert _popcount(torch.from_numpy(o[k].astype(np.int32))) == _popcount(torch.from_numpy(fx["once"][i].astype(np.int32)))
        assert _popcount(torch.from_numpy(m[k].astype(np.int32))) == _popcount(torch.from_numpy(fx["marks"][i].astype(np.int32)))
        s = S.from_number(sym[k], maps[k])
        assert np.array_equal(o[k], S.image_marks(fx["once"][i], s)) and np.array_equal(m[k], S.image_marks(fx["marks"][i], s))
    assert (c == 2).all()


def _restated_exchange(puzzle):
    """exchange() of one proper puzzle from oracle_once on its Q boards."""
    rows = []
    for a in np.nonzero(puzzle)[0]:
        q = puzzle.copy()
        q[a] = 0
        once, _, _ = U.oracle_once(q)
        for b in np.nonzero(q == 0)[0]:
            for v in range(1, 10):
                if once[b] >> (v - 1) & 1 and not (b == a and v == puzzle[a]):
                    nb = q.copy()
                    nb[b] = v
                    rows.append((nb, int(a), int(b), v))
    return rows


def test_exchange(solver):
    from sudoku_solver_distributed_amd.gen import exchange
    s = C.sets()
    puzzles = s["a"][:4]
    nb, parent, removed, cell, digit = (t.cpu().numpy() for t in exchange(torch.from_numpy(puzzles.copy())))
    assert nb.dtype == np.uint8 and nb.shape == (len(parent), 81) and parent.dtype == np.int64
    assert removed.dtype == cell.dtype == digit.dtype == np.int32 and len(nb) > 0
    assert set(parent.tolist()) <= set(range(4))
    for k in range(len(nb)):
        par = puzzles[parent[k]]
        assert (nb[k] != 0).sum() == 17 and O.count_solutions(nb[k], 2) == 1, k
        diff = np.nonzero(nb[k] != par)[0]
        assert par[removed[k]] != 0 and nb[k][cell[k]] == digit[k] and 1 <= digit[k] <= 9
        if cell[k] == removed[k]:  # the clue's digit changed in place
            assert diff.tolist() == [cell[k]]
        else:  # one removal and one addition
            assert sorted(diff.tolist()) == sorted([removed[k], cell[k]]) and nb[k][removed[k]] == 0 and par[cell[k]] == 0
    keys = list(zip(parent.tolist(), removed.tolist(), cell.tolist(), digit.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # puzzle 2: the one of the four whose 17 Q boards the oracle restates quickest (2 s; puzzle 1 takes 48 s)
    want = _restated_exchange(puzzles[2])
    got = [(nb[k], int(removed[k]), int(cell[k]), int(digit[k])) for k in np.nonzero(parent == 2)[0]]
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and g[1:] == w[1:]
    # an ambiguous board, an unsolvable one and a byte of 10 between proper puzzles
    mixed = np.stack([puzzles[0], s["b"][0], s["e"][0], s["f"][4], puzzles[2]])
    nb2, parent2, removed2, cell2, digit2 = (t.cpu().numpy() for t in exchange(torch.from_numpy(mixed)))
    assert set(parent2.tolist()) == {0, 4}
    for src, dst in ((0, 0), (2, 4)):
        assert np.array_equal(nb2[parent2 == dst], nb[parent == src])
        assert np.array_equal(removed2[parent2 == dst], removed[parent == src])
        assert np.array_equal(cell2[parent2 == dst], cell[parent == src])
        assert np.array_equal(digit2[parent2 == dst], digit[parent == src])
    empty = exchange(torch.zeros((0, 81), dtype=torch.uint8))
    assert empty[0].shape == (0, 81) and all(t.shape == (0,) for t in empty[1:])


def test_exchange_search(solver):
    from sudoku_solver_distributed_amd.gen import exchange, exchange_search
    seeds = torch.from_numpy(C.sets()["a"][:2].copy())
    classes = solver.canonical(seeds.to(solver.device))
    assert not torch.equal(classes[0], classes[1])
    canon = solver.canonical(exchange(classes)[0]).cpu().numpy()
    want, seen = [c for c in classes.cpu().numpy()], {c.tobytes() for c in classes.cpu().numpy()}
    for c in canon:  # first appearance
        if c.tobytes() not in seen:
            seen.add(c.tobytes())
            want.append(c)
    want = np.stack(want)
    assert len(want) > 3  # at least two new classes, so that a target of 3 cuts between them
    got = exchange_search(seeds, target=10 ** 6, max_rounds=1)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(exchange_search(seeds, target=10 ** 6, max_rounds=1), got)  # deterministic
    small = exchange_search(seeds, target=3)  # cut inside round 1
    assert np.array_equal(small.cpu().numpy(), want[:3])
    assert torch.equal(exchange_search(seeds, target=10 ** 6, max_rounds=0), classes)
