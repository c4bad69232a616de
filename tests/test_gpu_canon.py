"""GPU checks of the canonical form (canon_kernel + canon_reduce_kernel
through BatchSolver.canonical) against the corpus of minlex classes, the CPU
tool's fixture tests/golden/canon_cases.json and gen.apply_symmetry, and of
gen.class_ids / gen.unique_batch(distinct=True) built on it.  Every check is
an equality."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from sudoku_solver_distributed_amd import gen

pytestmark = pytest.mark.gpu

SYMMETRIES = 3359232


def _arr(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


def _run(solver, boards, **kw):
    """(canon, sym, autos) as arrays."""
    out = solver.canonical(torch.from_numpy(np.ascontiguousarray(boards)), return_sym=True, return_autos=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def classes(solver):
    """The 80 corpus lines and the GPU's (canon, sym, autos) of them."""
    base = np.stack([_arr(s) for s in gen.hard17_classes()])
    return base, _run(solver, base)


@pytest.fixture(scope="module")
def fixture_cases():
    doc = load_golden("canon_cases.json")["cases"]
    return ([c["name"] for c in doc], np.stack([_arr(c["board"]) for c in doc]),
            np.stack([_arr(c["canon"]) for c in doc]))


@pytest.fixture(scope="module")
def fixture_run(solver, fixture_cases):
    return _run(solver, fixture_cases[1], slices=1)


def test_corpus_lines_are_fixed_points(classes):
    base, (canon, sym, autos) = classes
    assert np.array_equal(canon, base)
    assert (autos >= 1).all() and (sym >= 0).all()
    assert np.array_equal(gen.apply_symmetry(base, sym)[0], base)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_images_of_a_class_come_back_to_it(solver, classes, n):
    base, (_, _, class_autos) = classes
    which = (7 * np.arange(n) + n) % 80
    images = np.empty((n, 81), dtype=np.uint8)
    for k in np.unique(which):
        at = np.nonzero(which == k)[0]
        images[at] = gen._symmetry_images(base[k:k + 1], len(at), seed=1000 * n + int(k))
    canon, sym, autos = _run(solver, images)
    assert np.array_equal(canon, base[which])
    assert np.array_equal(autos, class_autos[which])
    assert np.array_equal(gen.apply_symmetry(images, sym)[0], canon)
    only = solver.canonical(torch.from_numpy(images))  # d_autos = NULL, one tensor back
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), canon)


def test_fixture_and_invalid_boards(solver, fixture_cases):
    """The CPU tool's canon for every fixture board; a byte-10 board and a
    byte-255 board in between come back as they are with -1, -1."""
    _, boards, want = fixture_cases
    bad10, bad255 = boards[20].copy(), boards[9].copy()
    bad10[80] = 10
    bad255[0] = 255
    mixed = np.concatenate([boards[:13], bad10[None], boards[13:30], bad255[None], boards[30:]])
    canon, sym, autos = _run(solver, mixed)
    good = np.ones(len(mixed), dtype=bool)
    good[[13, 31]] = False
    assert np.array_equal(canon[good], want)
    assert np.array_equal(canon[~good], mixed[~good])
    assert list(sym[~good]) == [-1, -1] and list(autos[~good]) == [-1, -1]
    assert (sym[good] >= 0).all() and (autos[good] >= 1).all()
    assert np.array_equal(gen.apply_symmetry(mixed[good], sym[good])[0], want)


@pytest.mark.parametrize("slices", [0, 2, 7, 18, 2592])
def test_slices_never_change_results(solver, fixture_cases, fixture_run, slices):
    got = _run(solver, fixture_cases[1], slices=slices)
    for g, w in zip(got, fixture_run):
        assert np.array_equal(g, w)


def test_one_board_many_slices(solver, fixture_cases, fixture_run):
    """n = 1: slices=0 cuts the board into many slices; the same answer."""
    names, boards, _ = fixture_cases
    for name in ("puzzle_30", "cyclic_grid", "hard_search_3"):
        i = names.index(name)
        auto, one = _run(solver, boards[i:i + 1]), _run(solver, boards[i:i + 1], slices=1)
        for a, b, w in zip(auto, one, fixture_run):
            assert np.array_equal(a, b) and np.array_equal(a, w[i:i + 1])
    for bad in (-1, 2593):
        with pytest.raises(ValueError):
            solver.canonical(torch.from_numpy(boards[:1].copy()), slices=bad)
    assert solver.canonical(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0, 81)


def test_anchors(fixture_cases, fixture_run):
    names, _, _ = fixture_cases
    canon, sym, autos = fixture_run
    e, o = names.index("empty"), names.index("one_clue")
    assert (int(autos[e]), int(sym[e])) == (SYMMETRIES, 0)
    assert int(autos[o]) == SYMMETRIES // 81 == 41472  # the group is transitive on the cells
    assert canon[o].tolist() == [0] * 80 + [1]
    a, b = names.index("pair_a"), names.index("pair_b")
    assert np.array_equal(canon[a], canon[b]) and autos[a] == autos[b]


def test_back_to_back_calls_share_one_scratch(solver, classes):
    """Two calls on one stream and one cached scratch, 257 boards and then 3:
    the second call's records overwrite the first's while both are queued."""
    base, _ = classes
    big = gen._symmetry_images(base, 257, seed=9)
    which = np.random.default_rng(9).integers(len(base), size=257)
    small = gen._symmetry_images(base[5:6], 3, seed=10)
    a = solver.canonical(torch.from_numpy(big).to(solver.device), return_autos=True)
    b = solver.canonical(torch.from_numpy(small).to(solver.device), return_autos=True)
    assert np.array_equal(a[0].cpu().numpy(), base[which])
    assert np.array_equal(b[0].cpu().numpy(), base[[5, 5, 5]])
    assert (b[1] == b[1][0]).all().item()


def test_class_ids_of_a_hard17_batch(classes):
    base, _ = classes
    n = 4096
    boards = gen.hard17_batch(n, seed=2)
    which = np.random.default_rng(2).integers(len(base), size=n)  # _symmetry_images' first draw
    canon, ids, first = (t.cpu().numpy() for t in gen.class_ids(boards))
    assert np.array_equal(canon, base[which])  # every canon is the line of the image's class
    assert len(first) == len(np.unique(which)) == ids.max() + 1
    assert len(set(zip(ids.tolist(), which.tolist()))) == len(first)  # one id per class, one class per id
    for c in range(len(first)):
        assert first[c] == np.nonzero(ids == c)[0][0]
    # classes are numbered in the order of their canonical forms
    lines = [bytes(canon[i]) for i in first]
    assert lines == sorted(lines)


def test_unique_batch_distinct(solver):
    plain, full = gen.unique_batch(32, 81, seed=5, return_solutions=True)
    again = gen.unique_batch(32, 81, seed=5, distinct=False)
    assert torch.equal(again, plain)
    keep = torch.sort(gen.class_ids(plain)[2]).values
    dp, df = gen.unique_batch(32, 81, seed=5, return_solutions=True, distinct=True)
    assert torch.equal(dp, plain[keep]) and torch.equal(df, full[keep])
    assert torch.equal(gen.unique_batch(32, 81, seed=5, distinct=True), dp)
    # a batch with a repeated class: two images of one puzzle count once
    twice = torch.cat([plain[:4], gen.apply_symmetry(plain[:2], 1234567)[0]])
    _, ids, first = gen.class_ids(twice)
    assert len(first) == 4 and ids[4] == ids[0] and ids[5] == ids[1] and sorted(first.tolist()) == [0, 1, 2, 3]
