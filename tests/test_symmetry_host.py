"""CPU checks of symmetry covariance (symmetry_cases.py): the helper against
gen.apply_symmetry and against the oracle, the host builds of the analysis
headers (rate.h, plane_cand.h, plane_uniq.h, plane_min.h, plane_count.h)
against the oracle on boards outside every fixture, f(image of B) = image of
f(B) for every one of them on the pool, the pool's cost condition, and the
sampler's coverage that test_gpu_symmetry.py relies on.  Every check is an
equality."""
import numpy as np
import pytest

import count_cases as C
import min_cases as M
import native_build
import sample_cases as SC
import symmetry_cases as S
import test_cand_host as KH
import test_count_host as CH
import test_min_host as MH
import test_rate_host as RH
import test_uniq_host as UH
import uniq_cases as U
from oracle import oracle as O


@pytest.fixture(scope="module")
def rows():
    boards, source, which, syms = S.images()
    return {"boards": boards, "source": source, "which": which, "syms": syms}


# ---- the helper itself

def test_images_equal_apply_symmetry():
    """64 random symmetry numbers on pool boards: image_board under
    from_number is gen.apply_symmetry's image byte for byte; a symmetry and
    its inverse give the board, the marks and a turn order back."""
    from sudoku_solver_distributed_amd.gen import CANON_SYMMETRIES, apply_symmetry
    boards, names = S.pool()
    rng = np.random.default_rng(11)
    sel = rng.choice(np.nonzero((boards <= 9).all(1))[0], 64, replace=False)
    sel[:3] = [int(np.nonzero(names == "f")[0][k]) for k in (0, 1, 3)]  # the empty board, a full grid, a clash
    sym = rng.integers(0, CANON_SYMMETRIES, size=64)
    images, maps = apply_symmetry(boards[sel], sym)
    transposed = 0
    for k, i in enumerate(sel):
        s = S.from_number(sym[k], maps[k])
        assert np.array_equal(S.image_board(boards[i], s), images[k]), (int(i), int(sym[k]))
        transposed += sym[k] >= 1296 * 1296
        back = S.inverse(s)
        marks = rng.integers(0, 512, size=81).astype(np.uint16)
        order = rng.permutation(81).astype(np.uint8)
        order[:5] = [81, 255, 100, 0, 80]
        assert np.array_equal(S.image_board(images[k], back), boards[i])
        assert np.array_equal(S.image_marks(S.image_marks(marks, s), back), marks)
        assert np.array_equal(S.image_order(S.image_order(order, s), back), order)
        assert (S.image_order(order, s)[:3] == order[:3]).all()
        # a turn order names the image's cell: the same digit sits there
        cells = order[order <= 80]
        assert np.array_equal(s[1][boards[i][cells].astype(np.int64)], images[k][S.image_order(cells, s)])
    assert 8 <= transposed <= 56
    for seed in range(16):  # random_symmetry: a bijection of the cells that keeps the units, pi a bijection
        src, pi = S.random_symmetry(np.random.default_rng(seed))
        assert sorted(src.tolist()) == list(range(81)) and pi[0] == 0 and sorted(pi.tolist()) == list(range(10))
        full = C._b81(C.FULL)
        assert (S.image_board(full, (src, pi)) != full).any() and O.check(S.image_board(full, (src, pi)))


def _cd_with_count_2(k):
    """The first k boards of c and of d (alternating) that have several completions."""
    s = C.sets()
    out = []
    for key in ("c", "d"):
        out.append([g for g in s[key] if O.count_solutions(g, 2) == 2][:k])
    return np.array([g for pair in zip(*out) for g in pair], dtype=np.uint8)


def test_images_against_the_oracle():
    """The image convention pinned to the definition, not to the code under
    test: on 64 boards of c and d with several completions, oracle_once of the
    image is the image of oracle_once of the board."""
    boards = _cd_with_count_2(32)
    assert len(boards) == 64
    rng = np.random.default_rng(12)
    moved = 0
    for b in boards:
        s = S.random_symmetry(rng)
        once, marks, count = U.oracle_once(b)
        once2, marks2, count2 = U.oracle_once(S.image_board(b, s))
        assert count == count2 == 2
        assert np.array_equal(S.image_marks(once, s), np.array(once2, dtype=np.uint16))
        assert np.array_equal(S.image_marks(marks, s), np.array(marks2, dtype=np.uint16))
        moved += (np.array(once2) != np.array(once)).any()
    assert moved >= 32


def test_host_builds_equal_the_oracle_on_all_of_c_and_d():
    """512 boards, most of them in no fixture: uniq_host's once, marks and
    count, and cand_host's marks and count, equal oracle_once's."""
    s = C.sets()
    boards = np.concatenate([s["c"], s["d"]])
    want = [U.oracle_once(b) for b in boards]
    once, marks = (np.array([w[k] for w in want], dtype=np.uint16) for k in (0, 1))
    count = np.array([w[2] for w in want], dtype=np.int32)
    o, m, c = UH.uniq(native_build.host_lib("uniq_host"), boards)
    assert np.array_equal(o, once) and np.array_equal(m, marks) and np.array_equal(c, count)
    km, kc = KH.cand(native_build.host_lib("cand_host"), boards)
    assert np.array_equal(km, marks) and np.array_equal(kc, count)
    assert (count == 2).sum() >= 256 and (once[count == 2] != 0).any(1).sum() >= 128


# ---- covariance of every host build, on the pool

def test_pool_is_what_the_module_says():
    boards, names = S.pool()
    assert {k: int((names == k).sum()) for k in "abcdefhsr"} == \
        {"a": 128, "b": 32, "c": 256, "d": 256, "e": 64, "f": 5, "h": 32, "s": 128, "r": 10}
    assert ((boards[names == "h"] != 0).sum(1) == 15).all()
    all_rows, source, which, syms = S.images()
    assert len(all_rows) == len(boards) + S.IMAGES * (len(boards) - 1) and (boards > 9).any(1).sum() == 1
    assert np.array_equal(all_rows[:len(boards)], boards) and not which[:len(boards)].any()
    assert (all_rows[len(boards):] != boards[source[len(boards):]]).any(1).sum() >= 3 * 900
    assert not boards.flags.writeable and not all_rows.flags.writeable


def test_cost_condition_of_the_pool(rows):
    """plane_uniq.h's host build, the dearest of the entries: no board or image
    over the budget, few enough heavy ones for a single launch."""
    stats = {}
    _, _, _, per = UH.uniq(native_build.host_lib("uniq_host"), rows["boards"], stats=stats, passes=True)
    print("most passes", int(per.max()), "row", int(per.argmax()), "over", S.HEAVY_PASSES, int((per > S.HEAVY_PASSES).sum()),
          "mean", float(per.mean()))
    assert int(per.max()) <= U.PASS_BUDGET
    assert int((per > S.HEAVY_PASSES).sum()) <= S.HEAVY_PER_LAUNCH


@pytest.mark.parametrize("max_level", [1, 2, 3, 4])
def test_rate_is_covariant(rows, max_level):
    r, o, m = RH.rate(native_build.host_lib("rate_host"), rows["boards"], max_level)
    S.assert_covariant(r, "same", "rating")
    S.assert_covariant(o, "same", "open")
    assert S.assert_covariant(m, "marks", "marks") >= 100
    assert len(set(r.tolist())) >= 3


def test_candidates_are_covariant(rows):
    m, c = KH.cand(native_build.host_lib("cand_host"), rows["boards"])
    S.assert_covariant(c, "same", "count")
    assert S.assert_covariant(m, "marks", "marks") >= 100


def test_unique_candidates_are_covariant(rows):
    o, m, c = UH.uniq(native_build.host_lib("uniq_host"), rows["boards"])
    S.assert_covariant(c, "same", "count")
    assert S.assert_covariant(m, "marks", "marks") >= 100
    assert S.assert_covariant(o, "marks", "once") >= 100
    several = c == 2
    assert (o[several] != 0).any(1).sum() >= 400  # once bits of ambiguous boards are really compared


def test_minimize_is_covariant(rows):
    """Probe; greedy under the explicit order 0..80 carried to the images
    (what the default order means for the board itself); greedy under a random
    order carried over."""
    host = native_build.host_lib("min_host")
    lib_out, status, removed = MH.minimize(host, rows["boards"], None, M.PROBE)
    S.assert_covariant(status, "same", "probe status")
    S.assert_covariant(removed, "same", "probe removed")
    assert S.assert_covariant(lib_out, "board", "probe out") >= 100
    assert (removed > 0).sum() >= 400
    plain = np.broadcast_to(np.arange(81, dtype=np.uint8), rows["boards"].shape)
    ident = np.array([S.image_order(plain[r], rows["syms"][int(rows["source"][r]), int(rows["which"][r])])
                      if rows["which"][r] else plain[r] for r in range(len(plain))])
    own = rows["which"] == 0
    default = MH.minimize(host, rows["boards"][own], None, M.GREEDY)
    for order in (ident, S.orders(31)):
        out, status, removed = MH.minimize(host, rows["boards"], order, M.GREEDY)
        S.assert_covariant(status, "same", "greedy status")
        S.assert_covariant(removed, "same", "greedy removed")
        assert S.assert_covariant(out, "board", "greedy out") >= 100
        assert (removed > 0).sum() >= 400
        if order is ident:  # the default order is the explicit 0..80
            assert all(np.array_equal(x, y[own]) for x, y in zip(default, (out, status, removed)))


@pytest.mark.parametrize("limit", [2, 64, 1024])
def test_count_is_invariant(rows, limit):
    cnt, _ = CH._count(native_build.host_lib("count_host"), rows["boards"], limit, first=False)
    S.assert_covariant(cnt, "same", "count")
    if limit > 2:
        assert ((cnt > 2) & (cnt < limit)).sum() >= 400  # exact mid-range counts


# ---- the sampler covers small sets of completions (what test_gpu_symmetry.py selects on the GPU)

def test_sampler_covers_the_boards_with_few_completions():
    """S.few_boards(): at SAMPLE_PER_BOARD draws under SAMPLE_SEED the host
    model of the sampler returns every completion of at least 64 boards of c
    and d that have 2..16 of them; marks and once recomputed from those grids
    are uniq_host's."""
    boards = S.few_boards()
    k, _ = CH._count(native_build.host_lib("count_host"), boards, 64, first=False)
    grids, status = SC.host_sample(native_build.host_lib("sample_host"), boards, seed=S.SAMPLE_SEED,
                                   per_board=S.SAMPLE_PER_BOARD)
    sel, marks, once = S.covered(boards, k, grids, status)
    print("boards with 2..16 completions", int(((k >= 2) & (k <= 16)).sum()), "covered", len(sel))
    assert len(sel) >= 64
    o, m, c = UH.uniq(native_build.host_lib("uniq_host"), boards[sel])
    assert np.array_equal(m, marks) and np.array_equal(o, once) and (c == 2).all()
    assert (once != 0).any(1).sum() >= 32
