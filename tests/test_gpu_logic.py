"""GPU checks of the named techniques (logic_kernel and logic_wave_kernel
through BatchSolver.logic and the C ABI) against the fixture
tests/golden/logic_cases.json, which the plain-Python definition of
logic_cases.py made, against the host build of logic.h under other ladders, and
against the rest of the library.  Every check is an equality."""
import ctypes

import numpy as np
import pytest
import torch

import logic_cases as G
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # a partial wave, a wave less a lane, a wave, a wave and a lane, several claims
OTHER = [*G.LADDERS, [G.N | G.L, G.N | G.L | G.S2 | G.F2]]  # (the last: L without H, no level of the rating)


@pytest.fixture(scope="module")
def fx():
    return G.load_fixture()


@pytest.fixture(scope="module")
def host():
    import test_logic_host as H
    from native_build import host_lib
    lib = host_lib("logic_host")
    return lambda boards, start, ladder=G.DEFAULT_LADDER: H.run(lib, boards, start, ladder)


def gpu_logic(solver, boards, start, ladder=None):
    s, o, le, m = solver.logic(None if boards is None else torch.from_numpy(np.array(boards, dtype=np.uint8)), ladder,
                               None if start is None else torch.from_numpy(np.array(start, dtype=np.uint16).view(np.int16)),
                               return_open=True, return_left=True, return_marks=True)
    return s.cpu().numpy(), o.cpu().numpy(), le.cpu().numpy(), m.cpu().numpy().view(np.uint16)


def assert_same(names, got, want):
    bad = [i for i in range(len(names)) if any(not np.array_equal(g[i], w[i]) for g, w in zip(got, want))]
    assert not bad, [(names[i], int(got[0][i]), int(want[0][i]), got[1][i].tolist(), want[1][i].tolist(),
                      got[2][i].tolist(), want[2][i].tolist(), int((got[3][i] != want[3][i]).sum())) for i in bad[:6]]


def want_of(fx, idx):
    return fx["step"][idx], fx["open"][idx], fx["left"][idx], fx["marks"][idx]


def names_of(fx, idx):
    return [fx["names"][i] for i in idx]


def mix(fx, n, seed=0):
    """Fixture indices of n states, one per step value 0..6 and 8 in rotation
    with a planted state after them (position = k mod 9), so a wave's lanes
    end on different steps and in both kernels."""
    rng = np.random.default_rng(seed)
    by = [rng.permutation(np.nonzero((fx["kind"] == "") & (fx["step"] == k))[0]) for k in (0, 1, 2, 3, 4, 5, 6, 8)]
    by.append(rng.permutation(np.nonzero(fx["kind"] != "")[0]))
    return np.array([by[j % 9][(j // 9) % len(by[j % 9])] for j in range(n)])


def test_fixture_at_the_default_ladder(solver, fx):
    """Every fixture state, with all outputs and with each optional output
    left out."""
    b, s = fx["boards"], fx["start"]
    assert_same(fx["names"], gpu_logic(solver, b, s), want_of(fx, slice(None)))
    db = torch.from_numpy(b.copy()).to(solver.device)
    ds = torch.from_numpy(s.view(np.int16).copy()).to(solver.device)
    only = solver.logic(db, start=ds)
    st, o = solver.logic(db, start=ds, return_open=True)
    st2, le = solver.logic(db, start=ds, return_left=True)
    st3, m = solver.logic(db, start=ds, return_marks=True)
    for t in (only, st, st2, st3):
        assert np.array_equal(t.cpu().numpy(), fx["step"])
    assert np.array_equal(o.cpu().numpy(), fx["open"]) and np.array_equal(le.cpu().numpy(), fx["left"])
    assert np.array_equal(m.cpu().numpy().view(np.uint16), fx["marks"])
    assert only.dtype == torch.int32 and o.dtype == torch.int32 and le.dtype == torch.int32 and m.dtype == torch.int16
    assert o.shape == (len(db), 8) and le.shape == (len(db), 8) and m.shape == (len(db), 81)


@pytest.mark.parametrize("ladder", OTHER, ids=lambda l: "-".join(map(str, l)))
def test_other_ladders_against_the_host_build(solver, fx, host, ladder):
    b, s = fx["boards"], fx["start"]
    assert_same(fx["names"], gpu_logic(solver, b, s, ladder), host(b, s, ladder))


def test_hall_violations(solver, fx):
    for name, start, ladder, step, opens, left, marks in fx["violations"]:
        st, o, le, m = gpu_logic(solver, None, start[None], ladder)
        assert (int(st[0]), o[0].tolist(), le[0].tolist()) == (step, opens, left), (name, ladder)
        assert np.array_equal(m[0], marks), (name, ladder)


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(solver, fx, host, n):
    idx = mix(fx, n, seed=n)
    assert n < 9 or ({int(v) for v in fx["step"][idx]} >= {0, 1, 2, 3, 4, 5, 6, 8} and (fx["kind"][idx] != "").any())
    b, s = fx["boards"][idx], fx["start"][idx]
    assert_same(names_of(fx, idx), gpu_logic(solver, b, s), want_of(fx, idx))
    ladder = G.LADDERS[1]
    assert_same(names_of(fx, idx), gpu_logic(solver, b, s, ladder), host(b, s, ladder))


def test_every_board_through_the_wave_kernel(solver, fx):
    """130 states the first three steps leave open."""
    idx = np.nonzero(fx["open"][:, 2] > 0)[0][::3][:130]
    assert len(idx) == 130 and (fx["kind"][idx] != "").any() and (fx["kind"][idx] == "").any()
    assert_same(names_of(fx, idx), gpu_logic(solver, fx["boards"][idx], fx["start"][idx]), want_of(fx, idx))


def test_no_board_through_the_wave_kernel(solver, fx):
    """130 states the first three steps settle: solved or dead by then."""
    idx = np.resize(np.nonzero(fx["open"][:, 2] <= 0)[0], 130)
    assert {int(v) for v in fx["step"][idx]} == {0, 1, 2, 3}
    assert_same(names_of(fx, idx), gpu_logic(solver, fx["boards"][idx], fx["start"][idx]), want_of(fx, idx))


def test_empty_boards(solver):
    z = np.zeros((3, 81), dtype=np.uint8)
    for ladder, steps in ((None, 7), ([G.N], 1), ([G.ALL], 1), ([G.N | G.S2, G.ALL], 2)):
        st, o, le, m = gpu_logic(solver, z, None, ladder)
        assert st.tolist() == [steps + 1] * 3 and (m == 0x1FF).all()
        assert (o[:, :steps] == 81).all() and (le[:, :steps] == 729).all()
        assert (o[:, steps:] == G.NOT_RUN).all() and (le[:, steps:] == G.NOT_RUN).all()
    st, o, le, m = gpu_logic(solver, None, np.full((2, 81), 0x1FF, dtype=np.uint16))
    assert st.tolist() == [8, 8] and (le[:, :7] == 729).all() and (m == 0x1FF).all()
    assert solver.logic(torch.zeros((0, 81), dtype=torch.uint8)).shape == (0,)
    with pytest.raises(ValueError):
        solver.logic(None, start=None)
    for bad in ([], [G.N] * 9, [G.H], [G.N, G.N], [G.N | G.H, G.N | G.L], [G.N, 0x201]):
        with pytest.raises(ValueError):
            solver.logic(torch.zeros((1, 81), dtype=torch.uint8), bad)


def test_start_alone(solver, fx):
    """boards=None: the planted states are pencil marks on empty boards."""
    idx = np.nonzero(fx["kind"] != "")[0]
    assert_same(names_of(fx, idx), gpu_logic(solver, None, fx["start"][idx]), want_of(fx, idx))
    # ... and the boards alone, start=None
    idx = np.nonzero(fx["kind"] == "")[0]
    assert_same(names_of(fx, idx), gpu_logic(solver, fx["boards"][idx], None), want_of(fx, idx))


def test_invalid_bytes_and_marks(solver, fx):
    idx = mix(fx, 18, seed=3)
    b, s = fx["boards"][idx].copy(), fx["start"][idx].copy()
    b[1, 0], b[3, 80], s[5, 40], s[7, 17] = 10, 255, 0x200, 0x8001
    hit = [1, 3, 5, 7]
    st, o, le, m = gpu_logic(solver, b, s)
    assert (st[hit] == G.INVALID).all() and (o[hit] == G.INVALID).all() and (le[hit] == G.INVALID).all() and (m[hit] == 0).all()
    rest = np.array([k for k in range(18) if k not in hit])
    assert_same(names_of(fx, idx[rest]), (st[rest], o[rest], le[rest], m[rest]), want_of(fx, idx[rest]))


def _abi_call(solver, d_boards, d_start, n, ladder, arena, scratch_arena, opens=True, left=True, marks=True):
    """sdk_logic_batch on buffers carved from guarded arenas; returns the
    return code and the outputs' views."""
    L = solver.lib
    need = int(L.sdk_logic_scratch_bytes(n, len(ladder)))
    step = arena.carve(4 * n, itemsize=4, name="step")
    o = arena.carve(32 * n, itemsize=4, name="open") if opens else None
    le = arena.carve(32 * n, itemsize=4, name="left") if left else None
    m = arena.carve(162 * n, offset_mod4=2, name="marks") if marks else None  # 2-byte aligned, not 4
    sc = scratch_arena.carve(need, name="scratch", align=8)
    lad = (ctypes.c_uint32 * len(ladder))(*ladder)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(solver.device):
        rc = L.sdk_logic_batch(ptr(d_boards), ptr(d_start), ctypes.addressof(lad), len(ladder), step.data_ptr(), ptr(o),
                               ptr(le), ptr(m), n, sc.data_ptr(), need,
                               int(torch.cuda.current_stream(solver.device).cuda_stream))
    torch.cuda.synchronize(solver.device)
    return rc, step, o, le, m


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_byte_offset_inputs_and_guard_bytes(solver, fx, offset):
    """d_boards at every address mod 4 inside an arena of bytes > 9, d_start
    and d_marks at 2 mod 4; the outputs and the scratch inside arenas whose
    other bytes must not change; the inputs unchanged."""
    n = 131
    idx = mix(fx, n, seed=40 + offset)
    dev = solver.device
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 17), Arena(dev, OUT_FILL, 1 << 17), Arena(dev, OUT_FILL, 1 << 14)
    d = inputs.boards(n, offset_mod4=offset, name="boards")
    d.copy_(torch.from_numpy(fx["boards"][idx]))
    ds = inputs.carve(162 * n, offset_mod4=2, name="start")
    ds.copy_(torch.from_numpy(np.ascontiguousarray(fx["start"][idx]).view(np.uint8).reshape(-1)))
    assert d.data_ptr() % 4 == offset and ds.data_ptr() % 4 == 2
    rc, step, o, le, m = _abi_call(solver, d, ds, n, G.DEFAULT_LADDER, outs, scratch)
    assert rc == 0 and m.data_ptr() % 4 == 2
    got = (step.cpu().numpy(), o.cpu().numpy().reshape(n, 8), le.cpu().numpy().reshape(n, 8),
           m.cpu().numpy().view(np.uint16).reshape(n, 81))
    assert_same(names_of(fx, idx), got, want_of(fx, idx))
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), fx["boards"][idx])
    assert np.array_equal(ds.cpu().numpy().view(np.uint16).reshape(n, 81), fx["start"][idx])
    # the optional outputs left out: nothing but the steps is written
    outs2 = Arena(dev, OUT_FILL, 1 << 14)
    rc, step, _, _, _ = _abi_call(solver, d, ds, n, G.DEFAULT_LADDER, outs2, scratch, opens=False, left=False, marks=False)
    assert rc == 0 and np.array_equal(step.cpu().numpy(), fx["step"][idx])
    for a in (inputs, outs2, scratch):
        a.assert_guards()


def test_bad_arguments_launch_nothing(solver, fx):
    """Every refused call returns -2 and leaves the outputs and the scratch as
    they were."""
    n = 64
    dev = solver.device
    L = solver.lib
    outs = Arena(dev, OUT_FILL, 1 << 17)
    d = torch.from_numpy(fx["boards"][:n].copy()).to(dev)
    ds = torch.from_numpy(fx["start"][:n].view(np.int16).copy()).to(dev)
    step = outs.carve(4 * n, itemsize=4, name="step")
    o = outs.carve(32 * n, itemsize=4, name="open")
    le = outs.carve(32 * n, itemsize=4, name="left")
    m = outs.carve(162 * n, name="marks")
    need = int(L.sdk_logic_scratch_bytes(n, 7))
    sc = outs.carve(need, name="scratch", align=8)

    def call(**kw):
        ladder = kw.get("ladder", G.DEFAULT_LADDER)
        lad = (ctypes.c_uint32 * max(len(ladder), 1))(*ladder)
        a = {"b": d.data_ptr(), "s": ds.data_ptr(), "steps": len(ladder), "st": step.data_ptr(), "o": o.data_ptr(),
             "le": le.data_ptr(), "m": m.data_ptr(), "n": n, "sc": sc.data_ptr(), "bytes": need}
        a.update({k: v for k, v in kw.items() if k != "ladder"})
        return L.sdk_logic_batch(a["b"], a["s"], ctypes.addressof(lad), a["steps"], a["st"], a["o"], a["le"], a["m"], a["n"],
                                 a["sc"], a["bytes"], None)

    with torch.cuda.device(dev):
        for kw in ({"steps": 0}, {"ladder": [G.N] * 9}, {"ladder": [G.H]}, {"ladder": [G.N, 0x201]}, {"ladder": [G.N, G.N]},
                   {"ladder": [G.N | G.H, G.N | G.L]}, {"b": None, "s": None}, {"n": -1}, {"st": None}, {"sc": None},
                   {"bytes": need - 1}, {"s": ds.data_ptr() + 1}, {"m": m.data_ptr() + 1}, {"o": o.data_ptr() + 2},
                   {"le": le.data_ptr() + 2}, {"st": step.data_ptr() + 2}, {"sc": sc.data_ptr() + 4}):
            assert call(**kw) == -2, kw
    torch.cuda.synchronize(dev)
    assert bool((outs.buf == OUT_FILL).all())


def test_back_to_back_calls_share_one_scratch(solver, fx, host):
    """Calls on one stream with the one cached scratch, nothing between them,
    with different n and ladders: every call's counters are re-armed in stream
    order."""
    idx = mix(fx, 257, seed=9)
    db = torch.from_numpy(fx["boards"][idx]).to(solver.device)
    ds = torch.from_numpy(fx["start"][idx].view(np.int16).copy()).to(solver.device)
    solver.logic(db, start=ds)  # the scratch is sized now
    a = solver.logic(db, start=ds, return_left=True)
    b = solver.logic(db, start=ds, return_left=True)
    c = solver.logic(db[:65], G.LADDERS[1], ds[:65])
    e = solver.logic(db[:130], G.DEFAULT_LADDER[:3], ds[:130])
    f = solver.logic(db, start=ds)
    for st, le in (a, b):
        assert np.array_equal(st.cpu().numpy(), fx["step"][idx]) and np.array_equal(le.cpu().numpy(), fx["left"][idx])
    assert np.array_equal(c.cpu().numpy(), host(fx["boards"][idx[:65]], fx["start"][idx[:65]], G.LADDERS[1])[0])
    assert np.array_equal(e.cpu().numpy(), host(fx["boards"][idx[:130]], fx["start"][idx[:130]], G.DEFAULT_LADDER[:3])[0])
    assert np.array_equal(f.cpu().numpy(), fx["step"][idx])


def test_steps_agree_with_the_other_entries(solver, fx):
    """On the 408 boards: the exact candidates are a subset of logic's marks
    (the rules are sound); step 1..7 => exactly one completion, and the marks'
    single bits are solve's grid; step 0 => no completion; steps 1..3 are
    rate's at max_level 3."""
    board = np.nonzero(fx["kind"] == "")[0]
    b = torch.from_numpy(fx["boards"][board].copy()).to(solver.device)
    st, o, m = solver.logic(b, return_open=True, return_marks=True)
    exact = solver.candidates(b)
    live = st != 0
    assert int(live.sum()) == 400 and bool(((exact[live] & ~m[live]) == 0).all())
    cnt = solver.count_solutions(b, limit=2)
    solved = (st >= 1) & (st <= 7)
    assert int(solved.sum()) == 165 and int((st == 0).sum()) == 8
    assert bool((cnt[solved] == 1).all()) and bool((cnt[st == 0] == 0).all())
    grid, status = solver.solve(b[solved])
    assert bool((status == 1).all())
    assert torch.equal(m[solved].to(torch.int64), torch.ones_like(grid, dtype=torch.int64) << (grid.to(torch.int64) - 1))
    r, ro = solver.rate(b, max_level=3, return_open=True)
    low = st <= 3
    assert torch.equal(st[low], r[low]) and bool((r[~low] == 4).all()) and torch.equal(o[:, :3], ro[:, :3])
    st3, o3, m3 = solver.logic(b, G.DEFAULT_LADDER[:3], return_open=True, return_marks=True)
    r, ro, rm = solver.rate(b, max_level=3, return_open=True, return_marks=True)
    assert torch.equal(st3, r) and torch.equal(o3[:, :3], ro[:, :3]) and torch.equal(m3, rm)


def test_symmetry_images_keep_step_open_and_left(solver, fx):
    import symmetry_cases as S
    idx = mix(fx, 72, seed=77)
    rng = np.random.default_rng(5)
    syms = [S.random_symmetry(rng) for _ in idx]
    ib = np.stack([S.image_board(fx["boards"][i], t) for i, t in zip(idx, syms)])
    is_ = np.stack([S.image_marks(fx["start"][i], t) for i, t in zip(idx, syms)])
    st, o, le, m = gpu_logic(solver, ib, is_)
    assert np.array_equal(st, fx["step"][idx]) and np.array_equal(o, fx["open"][idx]) and np.array_equal(le, fx["left"][idx])
    assert np.array_equal(m, np.stack([S.image_marks(fx["marks"][i], t) for i, t in zip(idx, syms)]))


def test_grade(solver, fx):
    from sudoku_solver_distributed_amd import gen, solver as sol
    assert list(sol.DEFAULT_LADDER) == G.DEFAULT_LADDER and list(gen.GRADE_NAMES) == G.GRADE_NAMES
    assert (sol.N, sol.H, sol.L, sol.S2, sol.S3, sol.S4, sol.F2, sol.F3, sol.F4) == (G.N, G.H, G.L, G.S2, G.S3, G.S4, G.F2,
                                                                                   G.F3, G.F4)
    board = np.nonzero(fx["kind"] == "")[0][::5]
    g = gen.grade(fx["boards"][board])
    assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), fx["step"][board])
    assert gen.grade_names(g) == [G.GRADE_NAMES[s] for s in fx["step"][board]]
    assert gen.grade_names([0, 4, 6, 8, -1]) == ["dead", "pairs", "X-wing", "beyond", "invalid"]
