"""GPU checks of the completion list (enum_kernel through
BatchSolver.completions and the C ABI sdk_enumerate_batch).  A list is checked
as a set (enum_cases.py): rows valid, givens kept, rows distinct, their number
the exact count the fixture or the oracle knows; then the buffer contract, the
overflow rule, the per-board limit, a scratch reused after a PARTIAL call, the
argument checks, agreement with the other entries, symmetry, and gen.py's two
helpers."""
import ctypes

import numpy as np
import pytest
import torch

import enum_cases as N
import symmetry_cases as S
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu


def _t(solver, boards):
    return torch.from_numpy(np.array(boards, dtype=np.uint8)).to(solver.device)


def _full(solver, boards, **kw):
    """completions(return_status=True) as numpy: (grids, offsets, count, status, info)."""
    g, off, count, status, info = solver.completions(_t(solver, boards), return_status=True, **kw)
    if "slice" in kw:
        assert info["max_passes"] <= kw["slice"] + N.RUN_MAX, info
    return g.cpu().numpy(), off.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy(), info


def _raw(solver, d_boards, grids, owner, capacity, limit, count, status, scratch, size, slice, max_rounds, max_tasks,
         max_waves, info=None):
    """sdk_enumerate_batch as a C caller reaches it: (return code, info dict)."""
    own = (ctypes.c_int64 * 6)()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(solver.device):
        st = int(torch.cuda.current_stream(solver.device).cuda_stream)
        rc = solver.lib.sdk_enumerate_batch(d_boards.data_ptr(), d_boards.shape[0], ptr(grids), ptr(owner), capacity,
                                            limit, count.data_ptr(), status.data_ptr(), slice, max_rounds, max_tasks,
                                            scratch.data_ptr(), size, max_waves, st, info if info is not None else own)
    return rc, dict(zip(N.INFO, (int(v) for v in own)))


def _check_csr(boards, grids, off, want):
    """A CSR result holds the completion set of every board."""
    owner = np.repeat(np.arange(len(boards)), np.diff(off)).astype(np.int32)
    assert off[0] == 0 and off[-1] == len(grids)
    N.check_complete(boards, grids, owner, len(grids), want)


# ---- 1. the light pool as a set, on the full grid and on two waves

@pytest.fixture(scope="module")
def light_boards():
    boards, want, _ = N.pool()
    idx = N.light(256)
    return boards[idx], want[idx]


def test_light_pool_is_listed_whole_and_reproducibly(solver, light_boards):
    boards, want = light_boards
    full = _full(solver, boards)
    tiny = _full(solver, boards, **N.TINY)
    back = _full(solver, boards[::-1].copy())
    print(full[4], tiny[4])
    for g, off, count, status, info in (full, tiny):
        assert (status == N.DONE).all() and np.array_equal(count, want) and info["total"] == info["listed"]
        _check_csr(boards, g, off, want)
    assert tiny[4]["parks"] > 0 and tiny[4]["donated"] > 0
    assert np.array_equal(full[0], tiny[0]) and np.array_equal(full[1], tiny[1])
    # the reversed batch: the same rows per board
    assert np.array_equal(np.diff(back[1])[::-1], np.diff(full[1]))
    for i in (0, 1, len(boards) // 2, len(boards) - 1):
        j = len(boards) - 1 - i
        assert np.array_equal(back[0][back[1][j]:back[1][j + 1]], full[0][full[1][i]:full[1][i + 1]])
    rows = np.concatenate([back[0][back[1][j]:back[1][j + 1]] for j in range(len(boards) - 1, -1, -1)])
    assert np.array_equal(rows, full[0])
    # sorted: ascending by board, then lexicographically
    for i in range(len(boards)):
        k = N.row_keys(full[0][full[1][i]:full[1][i + 1]])
        assert (k[:-1] < k[1:]).all()
    # sort=False only groups
    g, off = solver.completions(_t(solver, boards), sort=False)
    assert np.array_equal(off.cpu().numpy(), full[1])
    _check_csr(boards, g.cpu().numpy(), full[1], want)


# ---- 2. H1

def _check_h1_rows(rows, h1):
    assert len(rows) == N.H1_COUNT
    assert N.valid_grids(rows).all()
    assert ((h1[None] == 0) | (rows == h1[None])).all()
    assert len(np.unique(N.row_keys(rows))) == N.H1_COUNT


def test_h1_alone_on_the_full_grid(solver):
    h1, want = N.load_fixture()["h1"]
    assert want == N.H1_COUNT
    g, off, count, status, info = solver.completions(_t(solver, h1[None]), sort=False, return_status=True)
    print(info)
    assert int(count[0]) == want and int(status[0]) == N.DONE and info["total"] == info["listed"] == want
    assert off.tolist() == [0, want]
    _check_h1_rows(g.cpu().numpy(), h1)


def test_h1_wherever_it_stands(solver):
    """H1 first, last of the first wave, first of the second and last of 130
    boards on three waves: 4 x 885 469 rows."""
    _, want, _ = N.pool()
    h1, total = N.load_fixture()["h1"]
    batch, src = N.placed(130, h1, (0, 63, 64, -1), N.light(126))
    expect = np.where(src < 0, total, want[np.maximum(src, 0)])
    g, off, count, status, info = solver.completions(_t(solver, batch), capacity=int(expect.sum()), sort=False,
                                                     return_status=True, max_waves=3, max_rounds=N.MANY)
    print(info)
    assert (status.cpu().numpy() == N.DONE).all() and np.array_equal(count.cpu().numpy(), expect)
    off = off.cpu().numpy()
    assert np.array_equal(np.diff(off), expect)
    g = g.cpu().numpy()
    ref = None
    for at in (0, 63, 64, 129):
        rows = N.sorted_rows(g[off[at]:off[at + 1]])
        if ref is None:
            _check_h1_rows(rows, h1)
            ref = rows
        else:
            assert np.array_equal(rows, ref)
    lightrows = np.concatenate([g[off[i]:off[i + 1]] for i in np.nonzero(src >= 0)[0]])
    lo = np.repeat(np.nonzero(src >= 0)[0], expect[src >= 0]).astype(np.int32)
    N.check_complete(batch, lightrows, lo, len(lightrows), np.where(src >= 0, expect, 0))


# ---- 3. the raw ABI: buffers, overflow, limit

@pytest.fixture(scope="module")
def few():
    boards, want, _ = N.pool()
    idx = N.light(68)
    return boards[idx], want[idx]


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
@pytest.mark.parametrize("case", ("fits", "one", "short", "limit2"))
def test_buffer_contract(solver, few, offset, case):
    """d_grids at every address mod 4, d_owner, d_count, d_status and a
    scratch of exactly the stated size among 0xA5 bytes, at the tiny knobs:
    no guard byte and no row at or beyond `listed` may change, the inputs stay
    as they are, info is written in its six slots only."""
    boards, want = few
    n, dev, total = len(boards), solver.device, int(want.sum())
    limit = 2 if case == "limit2" else 0
    capacity = {"fits": total + 5, "one": 1, "short": total - 1, "limit2": n * 2}[case]
    knobs = dict(N.TINY)
    need = int(solver.lib.sdk_enumerate_scratch_bytes(n, knobs["max_waves"], knobs["max_tasks"]))
    assert need == 256 + 2 * (64 * 81 * 128 + 64 * 8) + 2 * 64 * 128 + 4 * n
    inputs, scratch = Arena(dev, IN_FILL, 1 << 14), Arena(dev, OUT_FILL, 1 << 21)
    outs = Arena(dev, OUT_FILL, 85 * capacity + 12 * n + (1 << 12))
    d = inputs.boards(n, (offset + 1) % 4, name="boards")
    d.copy_(torch.from_numpy(boards))
    before = inputs.buf.clone()
    grids = outs.boards(capacity, offset, name="grids")
    owner = outs.carve(4 * capacity, itemsize=4, name="owner")
    count = outs.carve(8 * n, itemsize=8, name="count")
    status = outs.carve(4 * n, itemsize=4, name="status")
    sc = scratch.carve(need, name="scratch", align=16)
    assert grids.data_ptr() % 4 == offset
    host = np.full(14, -7, dtype=np.int64)
    rc, _ = _raw(solver, d, grids, owner, capacity, limit, count, status, sc, need,
                 info=host[4:].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), **knobs)
    torch.cuda.synchronize(dev)
    assert rc == 0
    rounds, donated, parks, most, tot, listed = (int(v) for v in host[4:10])
    print(case, offset, host[4:10])
    assert (host[:4] == -7).all() and (host[10:] == -7).all()
    exp = np.minimum(want, limit) if limit else want
    assert tot == int(exp.sum()) and listed == min(tot, capacity)
    assert np.array_equal(count.cpu().numpy(), exp)
    assert np.array_equal(status.cpu().numpy(), np.where((want >= limit) & (limit > 0), N.LIMITED, N.DONE))
    assert rounds > 1 and donated > 0 and 0 < most <= knobs["slice"] + N.RUN_MAX
    assert parks > 0 or limit  # (a limit of 2 ends most tasks before the ring is full)
    g, o = grids.cpu().numpy(), owner.cpu().numpy()
    assert (g[listed:] == OUT_FILL).all() and (o.view(np.uint8)[4 * listed:] == OUT_FILL).all()
    gg, oo = np.full_like(g, 0xA5), np.full_like(o, -7)
    gg[:listed], oo[:listed] = g[:listed], o[:listed]
    per = N.check_listed(boards, gg, oo, listed)
    assert (per <= exp).all() and (listed < tot or np.array_equal(per, exp))
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert torch.equal(inputs.buf, before)


def test_limits_on_fewer_exactly_and_more(solver, few):
    boards, want = few
    assert (want == 1).any() and (want == 2).any() and (want < 64).any() and (want > 64).any()
    for limit in (1, 2, 64):
        for kw in ({}, N.TINY):
            g, off, count, status, info = _full(solver, boards, limit=limit, **kw)
            assert np.array_equal(status, np.where(want >= limit, N.LIMITED, N.DONE))
            assert np.array_equal(count, np.minimum(want, limit))
            assert info["total"] == info["listed"] == int(count.sum())
            _check_csr(boards, g, off, count)


def test_an_empty_board_costs_its_limit(solver, few):
    boards, want = few
    batch = np.concatenate([boards[:30], np.zeros((1, 81), np.uint8), boards[30:]])
    g, off, count, status, info = _full(solver, batch, limit=64)
    print(info)
    exp = np.minimum(np.concatenate([want[:30], [2 ** 40], want[30:]]), 64)
    assert np.array_equal(count, exp) and status[30] == N.LIMITED and info["rounds"] < 64
    _check_csr(batch, g, off, exp)


def test_capacity_zero_is_count_exact(solver):
    boards, want, want_status = N.pool()
    idx = np.concatenate([N.light(120), np.nonzero(want_status == N.INVALID)[0]])
    for kw in ({}, N.TINY):
        g, off, count, status, info = _full(solver, boards[idx], capacity=0, **kw)
        c2, s2 = solver.count_exact(_t(solver, boards[idx]), return_status=True, **kw)
        assert len(g) == 0 and info["listed"] == 0 and info["total"] == int(want[idx].sum())
        assert np.array_equal(count, c2.cpu().numpy()) and np.array_equal(status, s2.cpu().numpy())
        assert np.array_equal(count, want[idx]) and np.array_equal(status, want_status[idx])


def test_overflow_raises_with_the_total(solver, few):
    from sudoku_solver_distributed_amd._lib import SudokuHipError
    boards, want = few
    with pytest.raises(SudokuHipError, match=str(int(want.sum()))):
        solver.completions(_t(solver, boards), capacity=int(want.sum()) - 1)
    with pytest.raises(SudokuHipError, match="without a complete list"):
        solver.completions(_t(solver, np.zeros((1, 81), np.uint8)), max_rounds=2, slice=8, max_waves=2)


# ---- 4. one scratch, reused after a PARTIAL call

def test_scratch_reused_after_a_partial_call(solver, few):
    boards, want = few
    h1 = N.load_fixture()["h1"][0]
    dev = solver.device
    size = int(solver.lib.sdk_enumerate_scratch_bytes(68, 2, 64))
    sc = torch.full((size,), 0x5A, dtype=torch.uint8, device=dev)
    a = np.concatenate([np.zeros((1, 81), np.uint8), h1[None], boards[:30]])
    cap = 1 << 16
    grids, owner = torch.empty((cap, 81), dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    count, status = torch.empty(68, dtype=torch.int64, device=dev), torch.empty(68, dtype=torch.int32, device=dev)
    rc, info = _raw(solver, _t(solver, a), grids, owner, cap, 0, count[:32], status[:32], sc, size, slice=32,
                    max_rounds=4, max_tasks=64, max_waves=2)
    assert rc == 0 and info["rounds"] == 4 and info["parks"] > 0 and info["listed"] == info["total"], info
    c, s = count[:32].cpu().numpy(), status[:32].cpu().numpy()
    assert s[0] == N.PARTIAL and s[1] == N.PARTIAL
    g, o = grids.cpu().numpy(), owner.cpu().numpy()
    gg, oo = np.full_like(g, 0xA5), np.full_like(o, -7)
    gg[:info["listed"]], oo[:info["listed"]] = g[:info["listed"]], o[:info["listed"]]
    per = N.check_listed(a, gg, oo, info["listed"])
    assert np.array_equal(per, c) and (c[2:][s[2:] == N.DONE] == want[:30][s[2:] == N.DONE]).all()
    rc, info = _raw(solver, _t(solver, boards), grids, owner, cap, 0, count, status, sc, size, slice=32,
                    max_rounds=N.MANY, max_tasks=64, max_waves=2)
    assert rc == 0 and (status.cpu().numpy() == N.DONE).all() and np.array_equal(count.cpu().numpy(), want)
    g, o = grids.cpu().numpy(), owner.cpu().numpy()
    gg, oo = np.full_like(g, 0xA5), np.full_like(o, -7)
    gg[:info["listed"]], oo[:info["listed"]] = g[:info["listed"]], o[:info["listed"]]
    N.check_complete(boards, gg, oo, info["listed"], want)


# ---- 5. argument checks

def test_argument_checks_launch_nothing(solver):
    dev = solver.device
    n = 4
    need = int(solver.lib.sdk_enumerate_scratch_bytes(n, 2, 64))
    d = _t(solver, N.pool()[0][N.light(n)])
    out = Arena(dev, OUT_FILL, 1 << 13)
    grids, owner = out.boards(8, name="grids"), out.carve(32, itemsize=4, name="owner")
    count, status = out.carve(8 * n, itemsize=8, name="count"), out.carve(4 * n, itemsize=4, name="status")
    sc = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    f = solver.lib.sdk_enumerate_batch

    def call(grids=grids.data_ptr(), owner=owner.data_ptr(), capacity=8, limit=0):
        return f(d.data_ptr(), n, grids, owner, capacity, limit, count.data_ptr(), status.data_ptr(), 8, 4, 64,
                 sc.data_ptr(), need, 2, None, None)

    assert call(capacity=-1) == -2 and call(limit=-1) == -2 and call(capacity=2 ** 31) == -2
    assert call(grids=None) == -2 and call(owner=None) == -2 and call(owner=owner.data_ptr() + 2) == -2
    assert f(None, 0, None, None, 0, 0, None, None, 0, 0, 0, None, 0, 0, None, None) == 0
    torch.cuda.synchronize(dev)
    assert bool((out.buf == OUT_FILL).all()) and bool((sc == 0xA5).all())
    assert call(grids=None, owner=None, capacity=0) == 0


# ---- 6. agreement with the other entries

def test_other_entries_agree_with_the_list(solver):
    sel = N.placements()[0]
    boards, want, _ = N.pool()
    b, d = boards[sel], _t(solver, boards[sel])
    g, off, count, status, _ = _full(solver, b)
    assert (status == N.DONE).all() and np.array_equal(count, want[sel]) and np.array_equal(np.diff(off), want[sel])
    exact = solver.count_exact(d).cpu().numpy()
    assert np.array_equal(exact, np.diff(off))
    marks = solver.candidates(d).cpu().numpy().view(np.uint16).astype(np.int64)
    once = solver.unique_candidates(d).cpu().numpy().view(np.uint16).astype(np.int64)
    _, first = solver.count_solutions(d, limit=2, return_first=True)
    first = first.cpu().numpy()
    sampled, st = solver.sample(d, seed=3, per_board=8)
    sampled = sampled.cpu().numpy().reshape(len(b), 8, 81)
    assert (st.cpu().numpy() == 1).all()
    for i in range(len(b)):
        rows = g[off[i]:off[i + 1]]
        bits = 1 << (rows.astype(np.int64) - 1)
        assert np.array_equal(np.bitwise_or.reduce(bits, axis=0), marks[i])
        times = np.stack([(rows == v).sum(axis=0) for v in range(1, 10)])  # (9, 81)
        assert np.array_equal(sum(((times[v] == 1).astype(np.int64) << v) for v in range(9)), once[i])
        keys = set(N.row_keys(rows).tolist())
        assert N.row_keys(first[i:i + 1])[0] in keys
        assert set(N.row_keys(sampled[i]).tolist()) <= keys


# ---- 7. symmetry

def test_completions_of_an_image_are_the_images_of_the_completions(solver):
    boards, want, _ = N.pool()
    idx = N.light(40)
    idx = idx[want[idx] > 0][:32]
    rng = np.random.default_rng(20271)
    syms = [[S.random_symmetry(rng) for _ in range(3)] for _ in idx]
    images = np.stack([S.image_board(boards[i], s) for i, ss in zip(idx, syms) for s in ss])
    g, off, _, status, _ = _full(solver, boards[idx])
    gi, offi, _, si, _ = _full(solver, images)
    assert (status == N.DONE).all() and (si == N.DONE).all()
    for k in range(len(idx)):
        rows = g[off[k]:off[k + 1]]
        for j in range(3):
            got = gi[offi[3 * k + j]:offi[3 * k + j + 1]]
            assert np.array_equal(got, N.sorted_rows(S.image_board(rows, syms[k][j])))


# ---- 8. gen.py's helpers

def test_uniform_completions_follow_their_rule_and_reach_every_row(solver):
    from sudoku_solver_distributed_amd import gen
    boards, want, want_status = N.pool()
    idx = N.light(256)
    idx = idx[(want[idx] >= 2) & (want[idx] <= 6)][:6]
    assert len(idx) == 6
    b = np.concatenate([boards[idx], boards[(want == 0) & (want_status == N.DONE)][:1]])
    g, off, _, _, _ = _full(solver, b)
    out, st = gen.uniform_completions(_t(solver, b), seed=11, per_board=256, first_key=5, device=solver.device)
    out, st = out.cpu().numpy().reshape(len(b), 256, 81), st.cpu().numpy().reshape(len(b), 256)
    m64 = (1 << 64) - 1

    def mix(x):
        x &= m64
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & m64
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & m64
        return x ^ (x >> 31)

    for i in range(len(b) - 1):
        rows, c = g[off[i]:off[i + 1]], int(off[i + 1] - off[i])
        pick = [(((mix(mix(11) + 5 + i * 256 + j)) >> 32) * c) >> 32 for j in range(256)]
        assert np.array_equal(out[i], rows[pick]) and (st[i] == 1).all()
        assert set(pick) == set(range(c))
    assert (st[-1] == 0).all() and (out[-1] == b[-1][None]).all()
    from sudoku_solver_distributed_amd._lib import SudokuHipError
    with pytest.raises(SudokuHipError):
        gen.uniform_completions(_t(solver, b), limit=2, device=solver.device)


def test_completion_classes_sum_to_the_count(solver):
    from sudoku_solver_distributed_amd import gen
    boards, want, _ = N.pool()
    idx = N.light(256)
    i = idx[np.argmax(want[idx])]
    reps, mult = gen.completion_classes(_t(solver, boards[i][None]), device=solver.device)
    assert int(mult.sum()) == want[i] and len(reps) == len(mult) >= 1
    assert N.valid_grids(reps.cpu().numpy()).all()
    assert len(np.unique(N.row_keys(reps.cpu().numpy()))) == len(reps)
