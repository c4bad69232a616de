"""Sudoku's symmetries in plain numpy, and the board pool the covariance tests
share (test_symmetry_host.py on the CPU, test_gpu_symmetry.py on the GPU).

A symmetry s = (src, pi): src[81] says which source cell every image cell
takes, pi[10] relabels the digits (pi[0] = 0).

    image_board(b, s)[k] = pi[b[src[k]]]
    image_marks(m, s)[k] = m[src[k]] with bit d-1 moved to bit pi[d]-1
    image_order(o, s)[t] = inv_src[o[t]]  (a turn byte > 80 names no cell and stays)

Covariant under a symmetry (f(image of B) = image of f(B)): candidates' marks,
unique_candidates' once and marks, rate's marks, minimize's out (greedy with
the turn order carried by image_order), solve's grid on a board with one
completion.  Invariant: the rating, the four open counts, count, status,
removed, count_solutions at any limit, the canonical form and autos.  NOT
covariant, and never compared through an image: count_solutions' d_first and
sample's grids on a board with several completions -- which completion comes
out follows the search's cell and digit order, which the image changes.

pool(): the boards, built once per process from seeds alone and read-only.
Cost condition (test_symmetry_host.py asserts it on the host build of
plane_uniq.h, over the pool and every image the tests launch): no board over
uniq_cases.PASS_BUDGET host passes, and at most HEAVY_PER_LAUNCH of them over
HEAVY_PASSES, so that one launch may hold them all.  A board of a set over the
budget would be replaced by the next of its set (SKIP lists them); none is.
Measured: the most expensive of the 3 641 boards and images takes 30 046
passes (an image of a 15-clue board of set h), and 13 take more than 4 096.
"""
import functools

import numpy as np

HEAVY_PASSES = 4096     # a board a wave waits for (test_gpu_cand.shuffled keeps at most 40 of set b in a batch)
HEAVY_PER_LAUNCH = 40
IMAGES = 3              # seeded symmetries per board
SEED = 20262
# (set, position) of boards over the budget, each replaced by the next of its set: none
SKIP = frozenset()
# the slices of count_cases.sets() the pool takes
TAKE = (("a", 128), ("b", 32), ("c", 256), ("d", 256), ("e", 64), ("f", 5))


# ---------------------------------------------------------------- symmetries
def _lines(rng):
    """A permutation of range(9) that keeps bands together: a band permutation
    composed with a permutation inside each band."""
    bands = rng.permutation(3)
    return np.concatenate([3 * bands[k] + rng.permutation(3) for k in range(3)]).astype(np.int64)


def make(R, C, transposed, pi):
    """(src, pi) from line maps R, C: src[9i+j] = 9R[i]+C[j], or 9C[j]+R[i]
    when transposed."""
    R, C = np.asarray(R, dtype=np.int64), np.asarray(C, dtype=np.int64)
    src = (9 * C[None, :] + R[:, None] if transposed else 9 * R[:, None] + C[None, :]).reshape(81)
    pi = np.asarray(pi, dtype=np.int64)
    assert sorted(src.tolist()) == list(range(81)) and pi[0] == 0 and sorted(pi[1:].tolist()) == list(range(1, 10))
    return src, pi


def random_symmetry(rng):
    """A uniform draw of (src, pi) from a numpy Generator."""
    R, C = _lines(rng), _lines(rng)
    transposed = bool(rng.integers(2))
    pi = np.concatenate([[0], 1 + rng.permutation(9)])
    return make(R, C, transposed, pi)


def from_number(sym, digit_map):
    """(src, pi) of symmetry number `sym` of gen.apply_symmetry and the row of
    its digit_maps for one board.  The row labels only the digits the board
    holds; the digits absent from it get the unused labels in ascending order.
    Any such completion is valid: a board is symmetric under swapping two
    digits it does not hold, so every completion of the row gives the same
    image of the board, and images of its marks that are equally right."""
    from sudoku_solver_distributed_amd.gen import line_perms
    perms = line_perms()
    sym = int(sym)
    t, R, C = sym // (1296 * 1296), perms[(sym // 1296) % 1296], perms[sym % 1296]
    pi = np.asarray(digit_map, dtype=np.int64).copy()
    unused = [v for v in range(1, 10) if v not in set(pi[1:].tolist())]
    pi[1:][pi[1:] == 0] = unused
    return make(R, C, t == 1, pi)


def inverse(s):
    """The symmetry that takes every image back."""
    src, pi = s
    inv_src, inv_pi = np.empty(81, dtype=np.int64), np.empty(10, dtype=np.int64)
    inv_src[src] = np.arange(81)
    inv_pi[pi] = np.arange(10)
    return inv_src, inv_pi


def image_board(board, s):
    src, pi = s
    return pi[np.asarray(board, dtype=np.int64)[..., src]].astype(np.uint8)


def image_marks(marks, s):
    """The image of 81 candidate masks (marks, once, the rating's marks)."""
    src, pi = s
    m = np.asarray(marks).astype(np.int64)[..., src]
    out = np.zeros_like(m)
    for d in range(1, 10):
        out |= ((m >> (d - 1)) & 1) << (pi[d] - 1)
    return out.astype(np.uint16)


def image_order(order, s):
    """The turn order that names, turn by turn, the image's cell of the cell
    `order` names; bytes above 80 name no cell and stay."""
    inv_src, _ = inverse(s)
    o = np.asarray(order, dtype=np.int64)
    return np.where(o <= 80, inv_src[np.minimum(o, 80)], o).astype(np.uint8)


# ---------------------------------------------------------------------- pool
@functools.lru_cache(maxsize=None)
def pool():
    """(boards (k, 81) uint8, names (k,) of str: the set of every board),
    read-only.  Sets a-f: count_cases.sets() by TAKE; h: 32 boards of
    hard17_batch(128, seed=99) with two clues removed by a seeded draw; s:
    hard_search_batch(128, seed=5); r: the ten boards of the rate fixture with
    the highest rating (the first ten in the fixture's order)."""
    import count_cases as C
    import rate_cases as R
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    sets = C.sets()
    boards, names = [], []
    for key, k in TAKE:
        keep = [i for i in range(len(sets[key])) if (key, i) not in SKIP][:k]
        boards.append(sets[key][keep])
        names += [key] * len(keep)
    rng = np.random.default_rng(SEED)
    h17 = hard17_batch(128, seed=99).numpy()
    h = h17[rng.choice(128, 32, replace=False)].copy()
    for g in h:
        g[rng.choice(np.nonzero(g)[0], 2, replace=False)] = 0
    _, rate_boards, rating, _, _ = R.load_fixture()
    top = np.argsort(-np.asarray(rating), kind="stable")[:10]
    boards += [h, hard_search_batch(128, seed=5).numpy(), np.asarray(rate_boards)[top]]
    names += ["h"] * 32 + ["s"] * 128 + ["r"] * 10
    boards, names = np.ascontiguousarray(np.concatenate(boards), dtype=np.uint8), np.array(names)
    boards.setflags(write=False)
    names.setflags(write=False)
    return boards, names


@functools.lru_cache(maxsize=None)
def images():
    """The pool and its IMAGES seeded symmetries per board, end to end:
    (boards (m, 81) uint8, source (m,): the pool index of every row, which
    (m,): 0 for the board itself and j for its j-th image, syms: (pool index,
    j) -> (src, pi)), read-only.  Boards with a byte > 9 have no image."""
    base, _ = pool()
    rng = np.random.default_rng(SEED + 1)
    rows, source, which, syms = [base], [np.arange(len(base))], [np.zeros(len(base), dtype=np.int64)], {}
    has = np.nonzero((base <= 9).all(1))[0]
    for j in range(1, IMAGES + 1):
        out = np.empty((len(has), 81), dtype=np.uint8)
        for k, i in enumerate(has):
            syms[int(i), j] = random_symmetry(rng)
            out[k] = image_board(base[i], syms[int(i), j])
        rows.append(out)
        source.append(has)
        which.append(np.full(len(has), j, dtype=np.int64))
    boards, source, which = np.ascontiguousarray(np.concatenate(rows)), np.concatenate(source), np.concatenate(which)
    for v in (boards, source, which):
        v.setflags(write=False)
    return boards, source, which, syms


# ---- three kernels, one set of completions: count_solutions, sample, unique_candidates
SAMPLE_PER_BOARD, SAMPLE_SEED = 96, 7  # fixed on the host model: test_symmetry_host.py prints what they cover


def few_boards():
    """All of sets c and d: where the boards with 2..16 completions are."""
    import count_cases as C
    s = C.sets()
    return np.concatenate([s["c"], s["d"]])


def covered(boards, k, grids, status):
    """The boards whose count k (count_solutions at limit 64) is 2..16 and
    whose SAMPLE_PER_BOARD sampled grids hold exactly k distinct ones -- every
    completion, then.  Returns (their indices, marks, once): marks the OR of
    the grids' digit bits, once the bits exactly one grid sets."""
    grids = np.asarray(grids).reshape(len(boards), -1, 81)
    status = np.asarray(status).reshape(len(boards), -1)
    sel, marks, once = [], [], []
    for i in np.nonzero((np.asarray(k) >= 2) & (np.asarray(k) <= 16))[0]:
        assert (status[i] == 1).all(), int(i)
        distinct = np.unique(grids[i], axis=0)
        if len(distinct) != k[i]:
            continue
        bits = 1 << (distinct.astype(np.int64) - 1)
        one = np.zeros(81, dtype=np.int64)
        for d in range(9):
            one |= (((bits >> d) & 1).sum(0) == 1).astype(np.int64) << d
        sel.append(int(i))
        marks.append(np.bitwise_or.reduce(bits, axis=0))
        once.append(one)
    return np.array(sel, dtype=np.int64), np.array(marks, dtype=np.uint16), np.array(once, dtype=np.uint16)


def shuffled(seed, size=None):
    """The rows of images() in a seeded shuffled order (the first `size` of
    it), so that a wave's lanes hold boards of different sets, and a board and
    its images lie apart."""
    order = np.random.default_rng(seed).permutation(len(images()[0]))
    return order if size is None else order[:size]


def orders(seed):
    """A turn order for every row of images(): a seeded permutation of the 81
    cells with eight turns blanked (255: the turn is skipped) for the pool's
    own rows, carried by image_order to their images."""
    boards, source, which, syms = images()
    rng = np.random.default_rng(seed)
    k = int((which == 0).sum())
    own = np.stack([rng.permutation(81) for _ in range(k)]).astype(np.uint8)
    for row in own:
        row[rng.choice(81, 8, replace=False)] = 255
    out = np.empty((len(boards), 81), dtype=np.uint8)
    for r in range(len(boards)):
        out[r] = own[source[r]] if which[r] == 0 else image_order(own[source[r]], syms[int(source[r]), int(which[r])])
    return out


def carried(answers, kind):
    """What covariance asks of every row of images(), from the answers of the
    pool's own rows (`answers` holds one answer per row of images()): kind
    "same" the source's answer, "marks" its image_marks, "board" its
    image_board.  Returns (want, moved): moved counts the image rows whose
    expected answer differs from the source's own array."""
    boards, source, which, syms = images()
    answers = np.asarray(answers)
    want = answers[source].copy()
    if kind != "same":
        f = image_marks if kind == "marks" else image_board
        for r in np.nonzero(which)[0]:
            want[r] = f(answers[source[r]], syms[int(source[r]), int(which[r])])
    moved = int((want != answers[source]).reshape(len(want), -1).any(1).sum())
    return want, moved


def assert_covariant(answers, kind, what):
    """answers of all rows of images(), in its order: every image row holds
    what carried() asks.  Returns moved."""
    _, source, which, _ = images()
    answers = np.asarray(answers)
    want, moved = carried(answers, kind)
    bad = np.nonzero((answers != want).reshape(len(want), -1).any(1))[0]
    names = pool()[1]
    assert len(bad) == 0, (what, len(bad), [(str(names[source[r]]), int(source[r]), int(which[r])) for r in bad[:8]])
    return moved
