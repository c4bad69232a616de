"""GPU checks that need no recorded answer: symmetry covariance of the
analysis kernels (rate, candidates, unique_candidates, minimize,
count_solutions, solve) on the pool of symmetry_cases.py and three seeded
images of every board, the same launches against the host builds of the
headers, the entries' agreement with one another on the pool, and three
kernels (count, sample, unique_candidates) on one set of completions.  Every
launch holds the boards in a seeded shuffled order, so that a wave's lanes
are in different phases.  Every check is an equality."""
import numpy as np
import pytest
import torch

import min_cases as M
import native_build
import symmetry_cases as S
import test_cand_host as KH
import test_count_host as CH
import test_min_host as MH
import test_uniq_host as UH

pytestmark = pytest.mark.gpu

SLICE = 513  # boards of the one-wave launches: about eight a lane through claim, refill and drain


@pytest.fixture(scope="module")
def rows():
    boards, source, which, syms = S.images()
    return {"boards": boards, "source": source, "which": which, "syms": syms, "names": S.pool()[1],
            "own": which == 0, "orders": S.orders(31)}


def launch(rows, seed, call, size=None, with_order=False):
    """call(boards tensor[, orders tensor]) on the rows of images() in the
    shuffled order of `seed` (the first `size` of them); returns (the row
    numbers, every output as a numpy array in that order)."""
    perm = S.shuffled(seed, size)
    args = [torch.from_numpy(rows["boards"][perm])]
    if with_order:
        args.append(torch.from_numpy(rows["orders"][perm]))
    out = call(*args)
    out = out if isinstance(out, tuple) else (out,)
    return perm, [t.cpu().numpy() for t in out]


def whole(rows, seed, call, **kw):
    """launch() of every row; the outputs back in the order of images()."""
    perm, outs = launch(rows, seed, call, **kw)
    back = []
    for o in outs:
        a = np.empty_like(o)
        a[perm] = o
        back.append(a.view(np.uint16) if a.dtype == np.int16 else a)
    return back


def u16(a):
    return a.view(np.uint16) if a.dtype == np.int16 else a


@pytest.fixture(scope="module")
def cand_all(solver, rows):
    return whole(rows, 1, lambda b: solver.candidates(b, return_count=True))


@pytest.fixture(scope="module")
def uniq_all(solver, rows):
    return whole(rows, 2, lambda b: solver.unique_candidates(b, return_marks=True, return_count=True))


@pytest.fixture(scope="module")
def rate_all(solver, rows):
    return whole(rows, 3, lambda b: solver.rate(b, max_level=4, return_open=True, return_marks=True))


@pytest.fixture(scope="module")
def count_all(solver, rows):
    return {limit: whole(rows, 4 + limit, lambda b: solver.count_solutions(b, limit=limit, return_first=True))
            for limit in (2, 64)}


@pytest.fixture(scope="module")
def min_all(solver, rows):
    return {"probe": whole(rows, 5, lambda b: solver.minimize(b, probe=True, return_removed=True)),
            "greedy": whole(rows, 6, lambda b, o: solver.minimize(b, o, return_removed=True), with_order=True)}


# ---- covariance, and the host model on every row

def test_rate_is_covariant(solver, rows, rate_all):
    for max_level in (4, 2):
        r, o, m = rate_all if max_level == 4 else whole(
            rows, 30, lambda b: solver.rate(b, max_level=2, return_open=True, return_marks=True))
        S.assert_covariant(r, "same", "rating")
        S.assert_covariant(o, "same", "open")
        assert S.assert_covariant(m, "marks", "marks") >= 100
        assert len(set(r.tolist())) >= 3


def test_candidates_are_covariant(solver, rows, cand_all):
    m, c = cand_all
    S.assert_covariant(c, "same", "count")
    assert S.assert_covariant(m, "marks", "marks") >= 100
    hm, hc = KH.cand(native_build.host_lib("cand_host"), rows["boards"])
    assert np.array_equal(m, hm) and np.array_equal(c, hc)
    perm, (sm, sc) = launch(rows, 11, lambda b: solver.candidates(b, return_count=True, max_waves=1), size=SLICE)
    assert np.array_equal(u16(sm), m[perm]) and np.array_equal(sc, c[perm])


def test_unique_candidates_are_covariant(solver, rows, uniq_all):
    o, m, c = uniq_all
    S.assert_covariant(c, "same", "count")
    assert S.assert_covariant(m, "marks", "marks") >= 100
    assert S.assert_covariant(o, "marks", "once") >= 100
    ho, hm, hc = UH.uniq(native_build.host_lib("uniq_host"), rows["boards"])
    assert np.array_equal(o, ho) and np.array_equal(m, hm) and np.array_equal(c, hc)
    perm, (so, sm, sc) = launch(rows, 12, lambda b: solver.unique_candidates(b, return_marks=True, return_count=True,
                                                                              max_waves=1), size=SLICE)
    assert np.array_equal(u16(so), o[perm]) and np.array_equal(u16(sm), m[perm]) and np.array_equal(sc, c[perm])


def test_minimize_is_covariant(solver, rows, min_all):
    host = native_build.host_lib("min_host")
    for mode, (out, status, removed) in min_all.items():
        S.assert_covariant(status, "same", mode + " status")
        S.assert_covariant(removed, "same", mode + " removed")
        assert S.assert_covariant(out, "board", mode + " out") >= 100
        assert (removed > 0).sum() >= 400
        want = MH.minimize(host, rows["boards"], rows["orders"], M.PROBE if mode == "probe" else M.GREEDY)
        assert all(np.array_equal(x, y) for x, y in zip((out, status, removed), want)), mode
    perm, got = launch(rows, 13, lambda b: solver.minimize(b, probe=True, return_removed=True, max_waves=1), size=SLICE)
    assert all(np.array_equal(x, y[perm]) for x, y in zip(got, min_all["probe"]))
    perm, got = launch(rows, 14, lambda b, o: solver.minimize(b, o, return_removed=True, max_waves=1), size=SLICE,
                       with_order=True)
    assert all(np.array_equal(x, y[perm]) for x, y in zip(got, min_all["greedy"]))


def test_count_is_invariant(solver, rows, count_all):
    for limit, (cnt, _) in count_all.items():
        S.assert_covariant(cnt, "same", "count")
        want, _ = CH._count(native_build.host_lib("count_host"), rows["boards"], limit, first=False)
        assert np.array_equal(cnt, want), limit
    assert ((count_all[64][0] > 2) & (count_all[64][0] < 64)).sum() >= 400  # exact mid-range counts


def test_solve_is_covariant(solver, rows, count_all):
    """The boards with one completion: the grid of the image is the image of
    the grid."""
    one = count_all[2][0] == 1
    assert one[rows["own"]].sum() >= 300
    grids = np.zeros_like(rows["boards"])
    sel = np.nonzero(one)[0]
    perm = np.random.default_rng(15).permutation(sel)
    g, st = solver.solve(torch.from_numpy(rows["boards"][perm]))
    assert bool((st == 1).all())
    grids[perm] = g.cpu().numpy()
    want, moved = S.carried(grids, "board")
    assert np.array_equal(grids[sel], want[sel]) and moved >= 100


# ---- the entries on the pool agree with one another

def test_entries_agree(solver, rows, cand_all, uniq_all, rate_all, count_all, min_all):
    own = rows["own"]
    boards = rows["boards"]
    (km, kc), (o, m, c), (r, _, rm) = cand_all, uniq_all, rate_all
    assert np.array_equal(km, m)
    assert not (o & ~m).any() and not (m & ~rm)[c >= 1].any()
    for other in (kc, np.minimum(2, count_all[64][0]), count_all[2][0], min_all["probe"][1], min_all["greedy"][1]):
        assert np.array_equal(c, other)
    solved = (r >= 1) & (r <= 4)
    assert (c[solved] == 1).all() and (c[r == 0] == 0).all() and solved.sum() >= 400 and (r == 0).sum() >= 100
    # one completion: marks == once == the bits of solve's grid
    one = np.nonzero(c == 1)[0]
    grid, st = solver.solve(torch.from_numpy(boards[one]))
    bits = (1 << (grid.cpu().numpy().astype(np.int64) - 1)).astype(np.uint16)
    assert bool((st == 1).all()) and np.array_equal(m[one], bits) and np.array_equal(o[one], bits)
    # sample and d_first on the pool's own boards: valid grids that keep the givens, inside the marks
    base = torch.from_numpy(boards[own]).to(solver.device)
    grids, status = solver.sample(base, seed=3, per_board=4)
    assert np.array_equal(np.minimum(1, status.cpu().numpy()), np.repeat(np.minimum(1, c[own]), 4))
    sets = [(grids.cpu().numpy(), np.repeat(np.nonzero(own)[0], 4))]
    sets += [(first, np.arange(len(boards))) for _, first in count_all.values()]
    for g, row in sets:
        has = c[row] >= 1
        assert has.sum() >= 700
        assert np.array_equal(g[~has], boards[row][~has])  # no completion: the input board
        g, row = g[has], row[has]
        assert bool((solver.check(torch.from_numpy(g).to(solver.device)) == 1).all())
        given = boards[row] != 0
        assert np.array_equal(g[given], boards[row][given])
        assert ((m[row].astype(np.int64) >> (g.astype(np.int64) - 1)) & 1).all()


def test_probe_erases_exactly_the_redundant_givens(solver, rows, uniq_all, min_all):
    """The pool's boards with one completion: probe erases a given exactly
    where count_solutions of the board without it is 1."""
    own = np.nonzero(rows["own"] & (uniq_all[2] == 1))[0]
    assert len(own) >= 300
    i, cell = np.nonzero(rows["boards"][own])
    trial = rows["boards"][own][i].copy()
    trial[np.arange(len(i)), cell] = 0
    cnt = solver.count_solutions(torch.from_numpy(trial), limit=2).cpu().numpy()
    assert set(cnt.tolist()) == {1, 2}
    erased = min_all["probe"][0][own][i, cell] == 0
    assert np.array_equal(erased, cnt == 1) and erased.sum() >= 1000 and (~erased).sum() >= 1000


# ---- three kernels, one set of completions

def test_count_sample_and_unique_candidates_on_one_set_of_completions(solver):
    """Boards of c and d with k = 2..16 completions (count_solutions at limit
    64) whose sampled grids number k distinct ones: marks and once recomputed
    from those k grids are unique_candidates'.  The sampler is specified bit
    for bit, so the boards covered are those test_symmetry_host.py finds on
    the host model: at least 64."""
    boards = S.few_boards()
    d = torch.from_numpy(boards).to(solver.device)
    k = solver.count_solutions(d, limit=64).cpu().numpy()
    grids, status = solver.sample(d, seed=S.SAMPLE_SEED, per_board=S.SAMPLE_PER_BOARD)
    sel, marks, once = S.covered(boards, k, grids.cpu().numpy(), status.cpu().numpy())
    assert len(sel) >= 64
    o, m, c = solver.unique_candidates(d[torch.from_numpy(sel).to(solver.device)], return_marks=True, return_count=True)
    assert np.array_equal(u16(m.cpu().numpy()), marks) and np.array_equal(u16(o.cpu().numpy()), once)
    assert bool((c == 2).all()) and (once != 0).any(1).sum() >= 32


def test_empty_batch(solver):
    none = torch.zeros((0, 81), dtype=torch.uint8)
    assert [t.shape[0] for t in solver.rate(none, return_open=True, return_marks=True)] == [0, 0, 0]
    assert [t.shape[0] for t in solver.candidates(none, return_count=True)] == [0, 0]
    assert [t.shape[0] for t in solver.unique_candidates(none, return_marks=True, return_count=True)] == [0, 0, 0]
    assert [t.shape[0] for t in solver.minimize(none, probe=True, return_removed=True)] == [0, 0, 0]
    assert [t.shape[0] for t in solver.count_solutions(none, limit=64, return_first=True)] == [0, 0]
    assert [t.shape[0] for t in solver.sample(none, per_board=4)] == [0, 0]
    assert [t.shape[0] for t in solver.solve(none)] == [0, 0]
