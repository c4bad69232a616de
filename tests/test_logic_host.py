"""CPU checks of the named techniques (csrc/logic.h, what logic_kernel's lanes
and logic_wave_kernel's waves run): the header compiled for the host
(tests/native/logic_host.cpp) against the fixture tests/golden/logic_cases.json
and, live, against the plain-Python definition of logic_cases.py; against the
rating's host build on the steps the two share; that nothing depends on the
schedule of the rules or on a symmetry of the state; and the C ABI's argument
checks through ctypes (no GPU).  Every check is an equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import logic_cases as G
import native_build

_vp = ctypes.c_void_p
# in (NULL ok), start (NULL ok), ladder, steps, step, open (NULL ok), left (NULL ok), marks (NULL ok), n -> 0 / -2
native_build.PROTOS.setdefault("logic_host", {"logic_host_batch": (
    [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int64], ctypes.c_int)})
native_build.PROTOS.setdefault("rate_host", {"rate_host_batch": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int], None)})


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("logic_host")


@pytest.fixture(scope="module")
def fx():
    return G.load_fixture()


def run(lib, boards, start, ladder=G.DEFAULT_LADDER, opens=True, left=True, marks=True):
    """logic_host_batch: (step, open, left, marks), None for an output left out."""
    b = None if boards is None else np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    s = None if start is None else np.ascontiguousarray(start, dtype=np.uint16).reshape(-1, 81)
    n = len(b) if b is not None else len(s)
    lad = np.array(ladder, dtype=np.uint32)
    st = np.full(n, 12345, dtype=np.int32)
    o = np.full((n, 8), 12345, dtype=np.int32) if opens else None
    le = np.full((n, 8), 12345, dtype=np.int32) if left else None
    m = np.full((n, 81), 0xFFFF, dtype=np.uint16) if marks else None
    ptr = lambda a: None if a is None else a.ctypes.data
    assert lib.logic_host_batch(ptr(b), ptr(s), lad.ctypes.data, len(lad), st.ctypes.data, ptr(o), ptr(le), ptr(m), n) == 0
    return st, o, le, m


def inputs(fx, idx=None):
    """(boards, start) of the fixture's states: the planted ones are pencil
    marks on empty boards, passed with both inputs."""
    idx = np.arange(len(fx["boards"])) if idx is None else np.asarray(idx)
    return fx["boards"][idx], fx["start"][idx]


def assert_same(names, got, want):
    bad = [i for i in range(len(names)) if any(not np.array_equal(g[i], w[i]) for g, w in zip(got, want))]
    assert not bad, [(names[i], int(got[0][i]), int(want[0][i]), got[1][i].tolist(), want[1][i].tolist(),
                      got[2][i].tolist(), want[2][i].tolist()) for i in bad[:6]]


def spread(fx, per=6, planted=24):
    """Indices of up to `per` boards of every step 0..8 and of `planted`
    planted states, two of every (kind, k)."""
    board = fx["kind"] == ""
    sel = [np.nonzero(board & (fx["step"] == k))[0][:per] for k in range(9)]
    for kind in G.KINDS:
        for k in (2, 3, 4):
            sel.append(np.nonzero((fx["kind"] == kind) & (fx["k"] == k))[0][:planted // 12])
    return np.concatenate(sel)


def test_fixture_is_what_the_design_lists(fx):
    """The recorded answers themselves: the tally of first solving steps, the
    boards the design names, 16 planted states of every kind and size."""
    board = fx["kind"] == ""
    assert int(board.sum()) == 408
    tally = {int(k): int(v) for k, v in zip(*np.unique(fx["step"][board], return_counts=True))}
    assert tally == {0: 8, 1: 48, 2: 34, 3: 54, 4: 27, 5: 1, 6: 1, 8: 235}
    at = {n: k for k, n in enumerate(fx["names"])}
    assert fx["step"][at["seed_160"]] == 5 and fx["step"][at["seed_74"]] == 6
    for name in ("seed_52", "seed_100", "seed_122", "seed_136"):   # X-wing removes candidates and does not solve
        i = at[name]
        assert fx["step"][i] == 8 and fx["left"][i][5] < fx["left"][i][4]
    assert int((board & (fx["step"] == 8) & (fx["left"][:, 5] < fx["left"][:, 4])).sum()) == 14
    # step 7 removes candidates on 13 boards (12 of the 17-clue classes and seed_92) and solves none
    swordfish = board & (fx["left"][:, 6] != fx["left"][:, 5])
    assert int(swordfish.sum()) == 13 and (fx["step"][swordfish] == 8).all() and "seed_92" in {fx["names"][i] for i in np.nonzero(swordfish)[0]}
    for kind in G.KINDS:
        for k in (2, 3, 4):
            assert int(((fx["kind"] == kind) & (fx["k"] == k)).sum()) == 16
    solved = (fx["step"] >= 1) & (fx["step"] <= 7)
    assert (fx["marks"][fx["step"] == 0] == 0).all()
    assert (np.bitwise_and(fx["marks"][solved], fx["marks"][solved] - 1) == 0).all() and (fx["marks"][solved] != 0).all()
    assert (fx["open"][:, 7] == G.NOT_RUN).all() and (fx["left"][:, 7] == G.NOT_RUN).all()


def test_host_matches_fixture(host, fx):
    """All 600 states bit for bit, with all outputs and with each optional
    output NULL."""
    b, s = inputs(fx)
    want = (fx["step"], fx["open"], fx["left"], fx["marks"])
    assert_same(fx["names"], run(host, b, s), want)
    for drop in ("opens", "left", "marks"):
        got = run(host, b, s, **{drop: False})
        for g, w, name in zip(got, want, ("step", "opens", "left", "marks")):
            assert (g is None) if name == drop else np.array_equal(g, w), (drop, name)
    only = run(host, b, s, opens=False, left=False, marks=False)
    assert np.array_equal(only[0], fx["step"]) and only[1:] == (None, None, None)
    # the boards alone and the planted states' marks alone: the NULL inputs
    board = np.nonzero(fx["kind"] == "")[0]
    assert_same([fx["names"][i] for i in board], run(host, fx["boards"][board], None), [w[board] for w in want])
    marks = np.nonzero(fx["kind"] != "")[0]
    assert_same([fx["names"][i] for i in marks], run(host, None, fx["start"][marks]), [w[marks] for w in want])


@pytest.mark.parametrize("ladder", [G.DEFAULT_LADDER, *G.LADDERS], ids=lambda l: "-".join(map(str, l)))
def test_host_matches_the_python_definition_live(host, fx, ladder):
    """About 40 boards over all steps and 24 planted states, marks included,
    against logic_cases.logic run now."""
    sel = spread(fx)
    assert len(sel) >= 60
    b, s = inputs(fx, sel)
    st, o, le, m = run(host, b, s, ladder)
    for k, i in enumerate(sel):
        want = G.logic(b[k] if fx["has_board"][i] else None, s[k] if fx["has_start"][i] else None, ladder)
        assert (int(st[k]), o[k].tolist(), le[k].tolist(), m[k].tolist()) == want, (fx["names"][i], ladder)


def test_first_steps_are_the_rating(host, fx):
    """Steps 1..3 of the default ladder are the rating's levels 1..3: step,
    open and marks of the ladder cut after three steps equal rate_host's at
    max_level 3 on all 408 boards, and the default ladder's first three open
    counts are those."""
    board = np.nonzero(fx["kind"] == "")[0]
    boards = fx["boards"][board]
    rate = native_build.host_lib("rate_host")
    n = len(boards)
    r, ro, rm = np.zeros(n, np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 81), np.uint16)
    rate.rate_host_batch(np.ascontiguousarray(boards).ctypes.data, r.ctypes.data, ro.ctypes.data, rm.ctypes.data, n, 3)
    st, o, le, m = run(host, boards, None, G.DEFAULT_LADDER[:3])
    assert np.array_equal(st, r) and np.array_equal(o[:, :3], ro[:, :3]) and np.array_equal(m, rm)
    assert (o[:, 3:] == G.NOT_RUN).all() and (le[:, 3:] == G.NOT_RUN).all()
    low = fx["step"][board] <= 3
    assert np.array_equal(fx["open"][board][:, :3], ro[:, :3])
    assert np.array_equal(fx["step"][board][low], r[low]) and (r[~low] == 4).all()


@pytest.mark.parametrize("ladder", [G.DEFAULT_LADDER, *G.LADDERS], ids=lambda l: "-".join(map(str, l)))
def test_schedule_of_the_rules_does_not_matter(fx, ladder):
    """Matrices, rows and subsets in descending order, a sweep's removals all
    taken from the sweep's first state: identical outputs on the whole
    fixture."""
    a = native_build.host_lib("logic_host")
    d = native_build.host_lib("logic_host", defines=("SDK_LOGIC_DESCEND=1", "SDK_RATE_DESCEND=1"))
    b, s = inputs(fx)
    for x, y in zip(run(a, b, s, ladder), run(d, b, s, ladder)):
        assert np.array_equal(x, y)


def test_symmetry_images_keep_step_open_and_left(host, fx):
    """Relabelled, permuted and transposed images of 40 states over all steps
    and kinds (the pencil marks carried by image_marks): the same step, open
    and left, and the image of the marks."""
    import symmetry_cases as S
    sel = spread(fx, per=2, planted=24)
    rng = np.random.default_rng(26)
    b, s = inputs(fx, sel)
    syms = [S.random_symmetry(rng) for _ in sel]
    ib = np.stack([S.image_board(x, t) for x, t in zip(b, syms)])
    is_ = np.stack([S.image_marks(x, t) for x, t in zip(s, syms)])
    st, o, le, m = run(host, ib, is_)
    assert np.array_equal(st, fx["step"][sel]) and np.array_equal(o, fx["open"][sel]) and np.array_equal(le, fx["left"][sel])
    assert np.array_equal(m, np.stack([S.image_marks(fx["marks"][i], t) for i, t in zip(sel, syms)]))


def test_planted_states_change_first_at_their_own_step(host, fx):
    planted = np.nonzero(fx["kind"] != "")[0]
    assert len(planted) == 192
    st, o, le, m = run(host, None, fx["start"][planted])
    count = np.unpackbits(np.ascontiguousarray(fx["start"][planted]).view(np.uint8), axis=1).sum(1)
    for k, i in enumerate(planted):
        assert G.first_change(int(count[k]), le[k].tolist()) == G.pattern_step(str(fx["kind"][i]), int(fx["k"][i])), fx["names"][i]


def test_hall_violations_behave_as_recorded(host, fx):
    """Pigeonhole violations N, H and L do not see: dead under the ladder that
    holds the rule, and whatever the definition recorded under the others."""
    assert len(fx["violations"]) >= 12
    for name, start, ladder, step, opens, left, marks in fx["violations"]:
        st, o, le, m = run(host, None, start, ladder)
        assert (int(st[0]), o[0].tolist(), le[0].tolist()) == (step, opens, left), (name, ladder)
        assert np.array_equal(m[0], marks), (name, ladder)
    by = {(name, tuple(ladder)): step for name, _, ladder, step, _, _, _ in fx["violations"]}
    row = "four_cells_three_digits_row"
    assert by[row, (G.N, G.N | G.S4)] == 0 and by[row, (G.NHL,)] == 2 and by[row, (G.N, G.N | G.S2)] == 3


def test_bytes_above_9_and_marks_above_0x1ff_are_invalid(host, fx):
    b, s = inputs(fx, np.arange(12))
    b, s = b.copy(), s.copy()
    b[1, 0], b[3, 80], s[5, 40], s[7, 17] = 10, 255, 0x200, 0x8001
    hit = [1, 3, 5, 7]
    for ladder in (G.DEFAULT_LADDER, [G.N]):
        st, o, le, m = run(host, b, s, ladder)
        assert (st[hit] == G.INVALID).all() and (o[hit] == G.INVALID).all() and (le[hit] == G.INVALID).all()
        assert (m[hit] == 0).all()
    st, o, le, m = run(host, b, s)
    rest = [k for k in range(12) if k not in hit]
    assert_same([fx["names"][k] for k in rest], (st[rest], o[rest], le[rest], m[rest]),
                (fx["step"][rest], fx["open"][rest], fx["left"][rest], fx["marks"][rest]))
    st, _, _, _ = run(host, None, s)
    assert (st[[5, 7]] == G.INVALID).all() and (st[[1, 3]] != G.INVALID).all()


def test_host_refuses_bad_ladders(host):
    z = np.zeros(81, dtype=np.uint8)
    out = np.zeros(1, dtype=np.int32)

    def call(lad, b=z, steps=None):
        words = np.array(lad or [0], dtype=np.uint32)
        return host.logic_host_batch(None if b is None else b.ctypes.data, None, words.ctypes.data,
                                     len(lad) if steps is None else steps, out.ctypes.data, None, None, None, 1)

    assert call([G.N]) == 0 and call([G.N | G.L, G.ALL]) == 0
    for lad in ([], [G.N] * 9, [G.H], [G.N, G.N], [G.N | G.H, G.N | G.L], [G.N, 0x201], [G.N | G.H, G.N]):
        assert call(lad) == -2, lad
        assert not G.ladder_ok(lad)
    assert call([G.N], None) == -2   # both inputs NULL


def test_rule_l_without_h(host, fx):
    """A rule set with L and without H (no level of the rating): against the
    definition, live, on boards that locked candidates act on."""
    sel = np.nonzero((fx["kind"] == "") & (fx["step"] == 3))[0][:6]
    ladder = [G.N | G.L, G.N | G.L | G.S2 | G.F2]
    st, o, le, m = run(host, fx["boards"][sel], None, ladder)
    for k, i in enumerate(sel):
        assert (int(st[k]), o[k].tolist(), le[k].tolist(), m[k].tolist()) == G.logic(fx["boards"][i], None, ladder)
    assert (le[:, 0] < 81 * 9).all()


def test_standalone_program_under_sanitizers(tmp_path, fx):
    """tests/native/logic_host.cpp as a program of its own (-DLOGIC_HOST_MAIN)
    built with -fsanitize=address,undefined: a board of every step and a
    planted state of every kind and size, no report."""
    exe = str(tmp_path / "logic_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DLOGIC_HOST_MAIN", "-o", exe,
                           os.path.join(native_build.NATIVE, "logic_host.cpp")])
    sel = spread(fx, per=1, planted=12)
    assert {int(v) for v in fx["step"][sel]} >= {0, 1, 2, 3, 4, 5, 6, 8} and len(sel) >= 20
    text = "".join(("s" + G.marks_text(fx["start"][i]) if fx["kind"][i] else "".join(str(int(v)) for v in fx["boards"][i]))
                   + "\n" for i in sel)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(sel)
    for line, i in zip(lines, sel):
        want = [str(int(fx["step"][i]))] + [f"{a}/{b}" for a, b in zip(fx["open"][i], fx["left"][i])]
        assert line.split() == want, (fx["names"][i], line)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f = L.sdk_logic_batch
    assert _lib.SDK_LOGIC_MAX_STEPS == 8 and _lib.SDK_LOGIC_NOT_RUN == -2
    assert (_lib.SDK_LOGIC_N, _lib.SDK_LOGIC_H, _lib.SDK_LOGIC_L, _lib.SDK_LOGIC_S2, _lib.SDK_LOGIC_S3, _lib.SDK_LOGIC_S4,
            _lib.SDK_LOGIC_F2, _lib.SDK_LOGIC_F3, _lib.SDK_LOGIC_F4) == (G.N, G.H, G.L, G.S2, G.S3, G.S4, G.F2, G.F3, G.F4)
    need = int(L.sdk_logic_scratch_bytes(100, 7))

    def call(ladder=G.DEFAULT_LADDER, steps=None, b=16, s=16, st=16, o=None, le=None, m=None, n=100, sc=16, size=need,
             null_ladder=False):
        lad = (ctypes.c_uint32 * max(len(ladder), 1))(*ladder)
        return f(b, s, None if null_ladder else ctypes.addressof(lad), len(ladder) if steps is None else steps, st, o, le, m,
                 n, sc, size, None)

    assert call(steps=0) == -2 and call(ladder=[G.N] * 9) == -2           # steps outside 1..8
    assert call(null_ladder=True) == -2
    assert call(ladder=[G.N, 0x201]) == -2 and call(ladder=[0x400 | G.N]) == -2   # a mask outside 0x1FF
    assert call(ladder=[G.H]) == -2 and call(ladder=[G.N, G.H | G.L]) == -2       # ... or without N
    assert call(ladder=[G.N, G.N]) == -2 and call(ladder=[G.N | G.H, G.N | G.L]) == -2   # not a proper superset
    assert call(ladder=[G.N | G.H, G.N]) == -2
    assert call(b=None, s=None) == -2                                     # both inputs NULL
    assert call(n=-1) == -2 and call(n=1 << 31, size=1 << 40) == -2       # n negative, above 2^31 - 1
    assert call(size=need - 1) == -2                                      # scratch one byte short
    assert call(st=None) == -2 and call(sc=None) == -2                    # a required pointer is NULL
    assert call(s=17) == -2 and call(m=17) == -2                          # d_start / d_marks at an odd address
    assert call(st=18) == -2 and call(o=18) == -2 and call(le=18) == -2 and call(sc=20) == -2   # misaligned
    assert call(b=None, s=None, st=None, n=0, sc=None, size=0) == 0       # n == 0
    assert call(b=None, s=None, st=None, n=0, sc=None, size=0, ladder=[G.H]) == -2   # ... still checks the ladder
    assert call(b=None, s=None, st=None, n=0, sc=None, size=0, steps=9) == -2


def test_scratch_bytes(L):
    sb = L.sdk_logic_scratch_bytes
    assert sb(100, 7) == 256 + 8 * 100 and sb(100, 1) == sb(100, 8) == 256 + 800 and sb(0, 7) == 256
    assert sb(-1, 7) == 0 and sb(1, 0) == 0 and sb(1, 9) == 0 and sb(1 << 31, 7) == 0
    assert sb(2 ** 31 - 1, 8) == 256 + 8 * (2 ** 31 - 1)
