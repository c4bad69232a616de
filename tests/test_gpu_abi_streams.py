"""Sections c (exact-size scratch with arbitrary contents) and d (every launch
and memset on the caller's stream) of test_gpu_abi_buffers.py for the seven
analysis entries of include/sudoku_hip.h, through the raw C ABI (runs on an
MI355X): sdk_rate_batch, sdk_candidates_batch, sdk_unique_candidates_batch,
sdk_minimize_batch, sdk_sample_batch (asynchronous on `stream`) and
sdk_count_exact_batch, sdk_enumerate_batch (SYNCHRONOUS on `stream`); then the
same promise one level up, BatchSolver's one cached scratch per entry used
from two streams.

Every entry runs at one shape (the _Case builders): arguments carved from
guarded arenas (abi_arena.Arena) at the odd addresses the entry allows, the
scratch exactly sdk_*_scratch_bytes(...) bytes at the entry's smallest
alignment.  Expectations are those of the entry's own GPU test and nothing
else: tests/golden/rate_cases.json, cand_cases.json, uniq_cases.json,
min_cases.json, sample_cases.json, exact_cases.py's pool (the fixture's and
the oracle's counts) and enum_cases.check_complete.  Nothing is compared with
another run of the code under test.

Section d is abi_arena._on_side_stream: the call waits on a side stream
behind a device delay, its inputs hold 0xFF until a copy on that stream
runs, and the default stream is idle, so a launch or memset that named
another stream runs at once and reads 0xFF, or finds its re-arm undone.  For
the five asynchronous entries the `dirty` call is the same entry on the 0xFF
inputs into other outputs; the two synchronous ones run in the harness's
blocking mode.  test_harness_sees_a_call_on_the_default_stream shows from
outside what a library that ignored `stream` looks like to this harness."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cand_cases as K
import enum_cases as N
import exact_cases as E
import min_cases as M
import rate_cases as R
import sample_cases as S
import uniq_cases as U
from abi_arena import IN_FILL, OUT_FILL, Arena, _delay_rate, _on_side_stream, _poisons, _stream_handle

pytestmark = pytest.mark.gpu

SLACK = 1 << 16  # arena bytes beyond the carved ones (guards, alignment)


# ----------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def _rate_fx():
    names, boards, rating, opens, marks = R.load_fixture()
    for a in (boards, rating, opens, marks):
        a.setflags(write=False)
    return {"names": names, "boards": boards, "rating": rating, "open": opens, "marks": marks}


@functools.lru_cache(maxsize=None)
def _cand_fx():
    names, boards, marks, count = K.load_fixture()
    return {"names": names, "boards": boards, "marks": marks, "count": count,
            "is_b": np.array([n.startswith("b_") for n in names])}


@functools.lru_cache(maxsize=None)
def _uniq_fx():
    names, boards, once, marks, count = U.load_fixture()
    return {"names": names, "boards": boards, "once": once, "marks": marks, "count": count,
            "is_b": np.array([n.startswith("b_") for n in names])}


@functools.lru_cache(maxsize=None)
def _min_fx():
    f = dict(M.load_fixture())
    f["groups"] = {"greedy81": np.nonzero((f["mode"] == M.GREEDY) & (f["max_empty"] == 81))[0]}
    return f


# -------------------------------------------------------------------- cases
class _Case:
    """One entry at its shape: the arenas, the arguments carved from them,
    the call and the comparison with the entry's fixture.

    inputs: (view, device tensor with the real contents, the same as numpy);
    outs / dirty_outs: two sets of output views (the second for the harness's
    `dirty` call; none for a blocking entry); scratch: the exact-size view;
    call(stream, outs): the entry through the C ABI, return code asserted
    (stream None: the current stream); check(got): tensors shaped like outs
    against the fixture; host: what a blocking entry's last call wrote to
    host memory (rounds, donated, parks, ...)."""

    def __init__(self, solver, name, blocking=False):
        self.solver, self.name, self.blocking = solver, name, blocking
        self.arenas, self.inputs, self.host = [], [], {}
        self.outs = self.dirty_outs = self.scratch = self.call = self.check = None

    def arena(self, fill, nbytes):
        a = Arena(self.solver.device, fill, int(nbytes) + SLACK)
        self.arenas.append(a)
        return a

    def give(self, view, array):
        array = np.ascontiguousarray(array)
        self.inputs.append((view, torch.from_numpy(array.copy()).to(self.solver.device), array))
        return view

    def carve_scratch(self, need, align):
        """`need` bytes at an address that is `align` and not 2 * align."""
        a = self.arena(OUT_FILL, need)
        a.carve(align, name="pad")
        self.scratch = a.carve(need, align=align, name="scratch")
        assert self.scratch.data_ptr() % (2 * align) == align and self.scratch.numel() == need
        return self.scratch

    def pairs(self):
        return [(view, real) for view, real, _ in self.inputs]

    def put_inputs(self):
        for view, real, _ in self.inputs:
            view.copy_(real)

    def assert_guards(self):
        for a in self.arenas:
            a.assert_guards()

    def finish(self):
        """The guards of every arena, and the inputs as they were given."""
        self.assert_guards()
        for view, _, array in self.inputs:
            assert np.array_equal(view.cpu().numpy(), array), self.name


def _u16(t, n):
    return t.cpu().numpy().view(np.uint16).reshape(n, 81)


def _rate(solver):
    """max_level 4 with d_open and d_marks: 257 boards, every rating 0..5 in
    turn, so the first kernel lists a third of them for the trial kernel
    (ratings 4 and 5: level 3 leaves them open) and answers the rest itself."""
    import test_gpu_rate as G
    fx, L, n = _rate_fx(), solver.lib, 257
    idx = G.mix(fx, n, seed=70)
    listed = fx["rating"][idx] >= 4
    assert listed.sum() >= 64 and (~listed).sum() >= 128 and {int(v) for v in fx["rating"][idx]} == {0, 1, 2, 3, 4, 5}
    c = _Case(solver, "rate")
    need = int(L.sdk_rate_scratch_bytes(n, 4))
    assert need == 256 + 8 * n
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 2 * 182 * n)
    b = c.give(ain.boards(n, 1, name="boards"), fx["boards"][idx])

    def outs(tag):
        return [aout.carve(4 * n, itemsize=4, name="rating" + tag), aout.carve(16 * n, itemsize=4, name="open" + tag),
                aout.carve(162 * n, offset_mod4=2, name="marks" + tag)]  # 2-byte aligned, not 4
    c.outs, c.dirty_outs = outs(""), outs(" (dirty)")
    sc = c.carve_scratch(need, 8)

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_rate_batch(b.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, 4, sc.data_ptr(),
                                  need, _stream_handle(solver, stream))
        assert rc == 0

    def check(got):
        G.assert_same([fx["names"][i] for i in idx],
                      (got[0].cpu().numpy(), got[1].cpu().numpy().reshape(n, 4), _u16(got[2], n)),
                      (fx["rating"][idx], fx["open"][idx], fx["marks"][idx]))
    c.call, c.check = call, check
    return c


def _candidates(solver):
    """513 boards on two waves (test_gpu_cand.shuffled: every fixture board)."""
    import test_gpu_cand as G
    fx, L, n = _cand_fx(), solver.lib, 513
    idx = G.shuffled(fx, n, seed=613)
    assert len(set(idx.tolist())) == len(fx["boards"])
    c = _Case(solver, "candidates")
    need = int(L.sdk_candidates_scratch_bytes(n, 2))
    assert need == 256 + 2 * 64 * 83 * 128
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 2 * 166 * n)
    b = c.give(ain.boards(n, 1, name="boards"), fx["boards"][idx])

    def outs(tag):
        return [aout.carve(162 * n, offset_mod4=2, name="marks" + tag), aout.carve(4 * n, itemsize=4, name="count" + tag)]
    c.outs, c.dirty_outs = outs(""), outs(" (dirty)")
    sc = c.carve_scratch(need, 8)

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_candidates_batch(b.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), n, sc.data_ptr(), need, 2,
                                        _stream_handle(solver, stream))
        assert rc == 0

    c.call = call
    c.check = lambda got: G.assert_same(fx, idx, _u16(got[0], n), got[1].cpu().numpy())
    return c


def _unique_candidates(solver):
    """513 boards on two waves, d_marks and d_count asked for as well."""
    import test_gpu_cand
    import test_gpu_uniq as G
    fx, L, n = _uniq_fx(), solver.lib, 513
    idx = test_gpu_cand.shuffled(fx, n, seed=613)
    assert len(set(idx.tolist())) == len(fx["boards"])
    c = _Case(solver, "unique_candidates")
    need = int(L.sdk_unique_candidates_scratch_bytes(n, 2))
    assert need == 256 + 2 * 64 * 85 * 128
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 2 * 328 * n)
    b = c.give(ain.boards(n, 3, name="boards"), fx["boards"][idx])

    def outs(tag):
        return [aout.carve(162 * n, offset_mod4=2, name="once" + tag), aout.carve(162 * n, offset_mod4=2, name="marks" + tag),
                aout.carve(4 * n, itemsize=4, name="count" + tag)]
    c.outs, c.dirty_outs = outs(""), outs(" (dirty)")
    sc = c.carve_scratch(need, 8)

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_unique_candidates_batch(b.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n,
                                               sc.data_ptr(), need, 2, _stream_handle(solver, stream))
        assert rc == 0

    c.call = call
    c.check = lambda got: G.assert_same(fx, idx, _u16(got[0], n), _u16(got[1], n), got[2].cpu().numpy())
    return c


def _minimize(solver):
    """SDK_MIN_GREEDY to 81 empties with d_order given: boards and order are
    both inputs; 513 cases on two waves."""
    import test_gpu_min as G
    fx, L, n = _min_fx(), solver.lib, 513
    idx = G.shuffled(fx, "greedy81", n, seed=513)
    assert len(set(idx.tolist())) == len(fx["groups"]["greedy81"])
    c = _Case(solver, "minimize")
    need = int(L.sdk_minimize_scratch_bytes(n, 2))
    assert need == 256 + 2 * 64 * M.MIN_LEVELS * 128
    ain, aout = c.arena(IN_FILL, 162 * n), c.arena(OUT_FILL, 2 * 89 * n)
    b = c.give(ain.boards(n, 1, name="boards"), fx["boards"][idx])
    order = c.give(ain.boards(n, 3, name="order"), fx["order"][idx])

    def outs(tag):
        return [aout.boards(n, 3, name="out" + tag), aout.carve(4 * n, itemsize=4, name="status" + tag),
                aout.carve(4 * n, itemsize=4, name="removed" + tag)]
    c.outs, c.dirty_outs = outs(""), outs(" (dirty)")
    sc = c.carve_scratch(need, 8)

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_minimize_batch(b.data_ptr(), order.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                      n, M.GREEDY, 81, sc.data_ptr(), need, 2, _stream_handle(solver, stream))
        assert rc == 0

    c.call = call
    c.check = lambda got: G.assert_same(fx, idx, *(t.cpu().numpy() for t in got))
    return c


def _sample(solver):
    """d_boards given: sample_cases.mixed_call(513, turn 1) under the
    fixture's seed on two waves."""
    import test_gpu_sample as G
    rows, L, n = S.rows(), solver.lib, 513
    idx = S.mixed_call(n, 1, seed=613)
    c = _Case(solver, "sample")
    need = int(L.sdk_sample_scratch_bytes(n, 2))
    assert need == 256 + 2 * S.WAVE_BYTES
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 2 * 85 * n)
    b = c.give(ain.boards(n, 1, name="boards"), rows["board"][idx])

    def outs(tag):
        return [aout.boards(n, 3, name="out" + tag), aout.carve(4 * n, itemsize=4, name="status" + tag)]
    c.outs, c.dirty_outs = outs(""), outs(" (dirty)")
    sc = c.carve_scratch(need, 8)

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_sample_batch(b.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), n, 1, S.SEED, 0, sc.data_ptr(), need,
                                    2, _stream_handle(solver, stream))
        assert rc == 0

    c.call = call
    c.check = lambda got: G.assert_rows(rows, idx, got[0].cpu().numpy(), got[1].cpu().numpy())
    return c


def _count_exact(solver):
    """exact_cases.mixed(68) at the tiny knobs (two waves, a ring of 128
    lines, slices of 8 passes): several rounds, donations and parks."""
    _, want, want_status = E.pool()
    boards, idx = E.mixed(68)
    L, n, knobs = solver.lib, len(boards), dict(E.TINY)
    c = _Case(solver, "count_exact", blocking=True)
    need = int(L.sdk_count_exact_scratch_bytes(n, knobs["max_waves"], knobs["max_tasks"]))
    assert need == 256 + 2 * (64 * 81 * 128 + 64 * 8) + 2 * 64 * 128 + 4 * n
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 12 * n)
    b = c.give(ain.boards(n, 1, name="boards"), boards)
    c.outs = [aout.carve(8 * n, itemsize=8, name="count"), aout.carve(4 * n, itemsize=4, name="status")]
    sc = c.carve_scratch(need, 16)
    stats = (ctypes.c_int64 * 4)()

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_count_exact_batch(b.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), n, knobs["slice"],
                                         knobs["max_rounds"], knobs["max_tasks"], sc.data_ptr(), need, knobs["max_waves"],
                                         _stream_handle(solver, stream), stats)
        assert rc == 0
        c.host = dict(zip(("rounds", "donated", "parks", "max_passes"), (int(v) for v in stats)))

    def check(got):
        count, status = got[0].cpu().numpy(), got[1].cpu().numpy()
        print("count_exact:", c.host)
        bad = np.nonzero((count != want[idx]) | (status != want_status[idx]))[0]
        assert len(bad) == 0, [(int(i), int(idx[i]), int(count[i]), int(want[idx[i]]), int(status[i])) for i in bad[:10]]
        assert c.host["parks"] > 0 and c.host["rounds"] > 1 and c.host["donated"] > 0, c.host
        assert 0 < c.host["max_passes"] <= knobs["slice"] + E.RUN_MAX
    c.call, c.check = call, check
    return c


def _enumerate(solver):
    """test_gpu_enum's `few` boards (68 light boards of the pool) at the tiny
    knobs with a capacity that fits."""
    pool_boards, pool_want, _ = N.pool()
    sel = N.light(68)
    boards, want = pool_boards[sel], pool_want[sel]
    L, n, knobs, total = solver.lib, len(boards), dict(N.TINY), int(want.sum())
    capacity = total + 5
    c = _Case(solver, "enumerate", blocking=True)
    need = int(L.sdk_enumerate_scratch_bytes(n, knobs["max_waves"], knobs["max_tasks"]))
    assert need == 256 + 2 * (64 * 81 * 128 + 64 * 8) + 2 * 64 * 128 + 4 * n
    ain, aout = c.arena(IN_FILL, 81 * n), c.arena(OUT_FILL, 85 * capacity + 12 * n)
    b = c.give(ain.boards(n, 2, name="boards"), boards)
    c.outs = [aout.boards(capacity, 3, name="grids"), aout.carve(4 * capacity, itemsize=4, name="owner"),
              aout.carve(8 * n, itemsize=8, name="count"), aout.carve(4 * n, itemsize=4, name="status")]
    sc = c.carve_scratch(need, 16)
    info = (ctypes.c_int64 * 6)()

    def call(stream, o):
        with torch.cuda.device(solver.device):
            rc = L.sdk_enumerate_batch(b.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), capacity, 0, o[2].data_ptr(),
                                       o[3].data_ptr(), knobs["slice"], knobs["max_rounds"], knobs["max_tasks"],
                                       sc.data_ptr(), need, knobs["max_waves"], _stream_handle(solver, stream), info)
        assert rc == 0
        c.host = dict(zip(N.INFO, (int(v) for v in info)))

    def check(got):
        g, o, count, status = (t.cpu().numpy() for t in got)
        print("enumerate:", c.host)
        listed = c.host["listed"]
        assert c.host["total"] == listed == total
        assert np.array_equal(count, want) and (status == N.DONE).all()
        assert (g[listed:] == OUT_FILL).all() and (o.view(np.uint8)[4 * listed:] == OUT_FILL).all()
        gg, oo = np.full_like(g, 0xA5), np.full_like(o, -7)
        gg[:listed], oo[:listed] = g[:listed], o[:listed]
        N.check_complete(boards, gg, oo, listed, want)
        assert c.host["rounds"] > 1 and c.host["donated"] > 0 and c.host["parks"] > 0, c.host
        assert 0 < c.host["max_passes"] <= knobs["slice"] + N.RUN_MAX
    c.call, c.check = call, check
    return c


ENTRIES = {"rate": _rate, "candidates": _candidates, "unique_candidates": _unique_candidates, "minimize": _minimize,
           "sample": _sample, "count_exact": _count_exact, "enumerate": _enumerate}


# --------------------------------------------- c. exact-size, random scratch
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_poisoned_scratch(solver, entry):
    """Exactly sdk_*_scratch_bytes(...) bytes inside guards, 0xFF and then
    seeded random bytes, on the default stream: a stack line, list slot, park
    word or ring line read before the call wrote it shows in the answers or
    the guards (zeros and 0xA5, which the entries' own tests leave there, can
    hide it: a park word of 0 is "nothing parked")."""
    c = ENTRIES[entry](solver)
    c.put_inputs()
    for what, fill in _poisons(c.scratch):
        fill()
        for v in c.outs:
            v.view(torch.uint8).fill_(OUT_FILL)
        c.call(None, c.outs)
        torch.cuda.synchronize()
        c.check(c.outs)
        c.assert_guards()
    c.finish()


# ----------------------------------------------------------- d. stream order
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_stream(solver, entry):
    """The entry on a side stream behind a delay (abi_arena._on_side_stream).
    Asynchronous entries: a `dirty` call of the same entry on the 0xFF inputs
    leaves the queue head used, so a memset that ran early on another stream
    is undone and the call claims nothing.  Synchronous entries (count_exact:
    init, a kernel and a claim-word memset per round, a final kernel;
    enumerate likewise): the harness's blocking mode."""
    c = ENTRIES[entry](solver)
    got = _on_side_stream(solver, c.name, c.pairs(), lambda s: c.call(s, c.outs), c.outs, scratch=[c.scratch],
                          dirty=None if c.blocking else (lambda s: c.call(s, c.dirty_outs)), blocking=c.blocking)
    c.check(got)
    c.finish()


def test_harness_sees_a_call_on_the_default_stream(solver):
    """The negative control: candidates is handed the default stream while
    its input copy waits on the side stream -- from outside, a library that
    ignored `stream`.  Its kernel runs during the delay (`early`, which the
    harness asserts), reads 0xFF boards and answers SDK_INVALID with zero
    marks for every one of them, and the comparison of test_stream raises.
    Only valid memory is touched: the same call with the same arguments."""
    c = _candidates(solver)
    default = torch.cuda.default_stream(solver.device)
    got = _on_side_stream(solver, "candidates on the default stream", c.pairs(), lambda s: c.call(default, c.outs),
                          c.outs, scratch=[c.scratch])
    torch.cuda.synchronize()
    assert bool((got[1] == K.INVALID).all()) and not bool(got[0].any())
    with pytest.raises(AssertionError):
        c.check(got)
    c.finish()


# ----------------------------------------- the wrappers' one cached scratch
def _second_call_ms(second, s2):
    """The second call's own time on the device, by events, the device idle
    before it (the larger of two measurements)."""
    ms = 0.0
    for _ in range(2):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s2)
        second()
        e1.record(s2)
        s2.synchronize()
        ms = max(ms, e0.elapsed_time(e1))
    return ms


def _two_streams(solver, what, first, second, s1, s2):
    """first() on s1 behind a delay of ten times second()'s own duration,
    then second() on s2, both on the wrapper's one cached scratch: when s2
    has finished, s1's delay must be over, because BatchSolver._ws_stream
    made s2 wait for s1.  Without that wait s2 ends a delay's length early.
    Returns (first's result, second's result, was the delay still running
    when both calls had been issued)."""
    run, rate = _delay_rate(solver.device)
    first()  # every kernel loaded, the scratch sized
    ms = _second_call_ms(second, s2)
    torch.cuda.synchronize()
    after_delay = torch.cuda.Event()
    with torch.cuda.stream(s1):
        run(max(1, 10.0 * ms * rate))
        after_delay.record(s1)
    a = first()
    b = second()
    early = not after_delay.query()
    s2.synchronize()
    waited = after_delay.query()
    s1.synchronize()
    print(f"{what}: second call {ms:.3f} ms, delay {10.0 * ms:.3f} ms")
    assert waited, f"{what}: stream 2 finished while stream 1's delay of {10.0 * ms:.3f} ms was still running"
    return a, b, early


def test_wrapper_candidates_on_two_streams(solver):
    """BatchSolver.candidates on s1 and, with other boards, on s2.  The call
    is asynchronous, so the delay is still running when both are issued."""
    import test_gpu_cand as G
    fx = _cand_fx()
    ia, ib = G.shuffled(fx, 130, seed=7), G.shuffled(fx, 130, seed=8)
    assert not np.array_equal(ia, ib)
    da, db = (torch.from_numpy(fx["boards"][i]).to(solver.device) for i in (ia, ib))
    s1, s2 = torch.cuda.Stream(solver.device), torch.cuda.Stream(solver.device)
    a, b, early = _two_streams(solver, "candidates", lambda: solver.candidates(da, return_count=True, stream=s1),
                               lambda: solver.candidates(db, return_count=True, stream=s2), s1, s2)
    assert early
    for (m, cnt), idx in ((a, ia), (b, ib)):
        G.assert_same(fx, idx, m.cpu().numpy().view(np.uint16), cnt.cpu().numpy())


def test_wrapper_count_exact_on_two_streams(solver):
    """BatchSolver.count_exact, SYNCHRONOUS on its stream: the host is back
    from the call on s1 only after the delay, so here the order is the
    host's; the cached scratch, last written on s1, is armed again on s2.
    Light boards (at most 1022 completions each; the boards of the raw-ABI
    tests above take 2.5 s a call at the tiny knobs, and the delay is ten
    calls long)."""
    boards, want, want_status = E.pool()
    ia, ib = E.light(133)[:68], E.light(133)[68:]
    da, db = (torch.from_numpy(boards[i]).to(solver.device) for i in (ia, ib))
    s1, s2 = torch.cuda.Stream(solver.device), torch.cuda.Stream(solver.device)
    # more completions than one lane has passes in a round (a completion costs a pass): several rounds each
    assert min(want[ia].max(), want[ib].max()) > E.TINY["slice"] + E.RUN_MAX
    kw = dict(E.TINY, return_status=True, return_stats=True)
    a, b, _ = _two_streams(solver, "count_exact", lambda: solver.count_exact(da, stream=s1, **kw),
                           lambda: solver.count_exact(db, stream=s2, **kw), s1, s2)
    for (count, status, stats), idx in ((a, ia), (b, ib)):
        print("count_exact wrapper:", stats)
        assert np.array_equal(count.cpu().numpy(), want[idx]) and np.array_equal(status.cpu().numpy(), want_status[idx])
        assert stats["rounds"] > 1
