"""GPU tests of the unavoidable sets (BatchSolver.unavoidable,
sdk_unavoidable_batch, sdk_unavoidable_minimal_batch) against
the fixture tests/golden/ua_cases.json -- the enumeration at 9 cells and the
Python restatement at 12 -- the host build of csrc/ua.h beyond 12 cells, the
definitions recomputed through other entries (completions, count_solutions,
unique_batch, minimize) and the C ABI's contracts.  Rows are compared as
multisets, everything else by equality."""
import functools
from collections import Counter

import numpy as np
import pytest
import torch

import native_build
import symmetry_cases as Y
import ua_cases as U
from abi_arena import IN_FILL, OUT_FILL, Arena, _on_side_stream, _poisons, _stream_handle
from test_ua_host import host_minimal, run_host

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5


@functools.lru_cache(maxsize=None)
def grids_of(names=None):
    cases = U.load_fixture() if names is None else [c for c in U.load_fixture() if c.name in names]
    g = np.stack([c.grid for c in cases])
    g.setflags(write=False)
    return cases, g


def raw(solver, grids, max_size, capacity, max_waves=0):
    """sdk_unavoidable_batch as it is: (rows (listed, 4) uint32, count,
    status, (total, listed)), after a check that nothing at or beyond row
    `listed` was written."""
    g = torch.from_numpy(np.array(grids, dtype=np.uint8).reshape(-1, 81)).to(solver.device)
    n = g.shape[0]
    rows = torch.full((max(capacity, 1), 4), FILL32 - (1 << 32), dtype=torch.int32, device=solver.device)
    count = torch.full((n,), 12345, dtype=torch.int32, device=solver.device)
    status = torch.full((n,), 12345, dtype=torch.int32, device=solver.device)
    info = torch.full((2,), -7, dtype=torch.int64, device=solver.device)
    need = int(solver.lib.sdk_unavoidable_scratch_bytes(n, max_waves))
    sc = torch.empty(need, dtype=torch.uint8, device=solver.device)
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_unavoidable_batch(g.data_ptr(), n, max_size, rows.data_ptr() if capacity else None, capacity,
                                              count.data_ptr(), status.data_ptr(), info.data_ptr(), sc.data_ptr(), need,
                                              max_waves, _stream_handle(solver))
    assert rc == 0
    torch.cuda.synchronize()
    total, listed = (int(v) for v in info.tolist())
    assert listed == min(total, capacity)
    r = rows.cpu().numpy().view(np.uint32)
    assert (r[listed:] == FILL32).all()
    return r[:listed], count.cpu().numpy(), status.cpu().numpy(), (total, listed)


def assert_rows(cases, rows, count, status, max_size, want=None):
    got = U.by_owner(rows, len(cases))
    assert status.tolist() == [c.status for c in cases]
    for i, c in enumerate(cases):
        w = c.rows(max_size) if want is None else want[i]
        assert got[i] == w, (c.name, sum(got[i].values()), sum(w.values()))
        assert count[i] == sum(w.values()), c.name


def public(solver, grids, **kw):
    """BatchSolver.unavoidable's answer as (list of masks per grid, in the
    order given; offsets; the rest)."""
    out = solver.unavoidable(torch.from_numpy(np.array(grids, dtype=np.uint8).reshape(-1, 81)), **kw)
    sets, offsets = out[0].cpu().numpy(), out[1].cpu().numpy()
    if kw.get("packed"):
        assert sets.dtype == np.int32 and sets.shape[1:] == (3,)
        masks = U.words_to_masks(np.concatenate([sets.view(np.uint32), np.zeros((len(sets), 1), np.uint32)], axis=1))
    else:
        assert sets.dtype == np.uint8 and sets.shape[1:] == (81,) and sets.max(initial=0) <= 1
        masks = [U.mask_of(np.nonzero(r)[0]) for r in sets]
    assert offsets[0] == 0 and offsets[-1] == len(masks) and (np.diff(offsets) >= 0).all()
    return [masks[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)], offsets, out[2:]


@pytest.mark.parametrize("max_size", [9, 12])
def test_fixture(solver, max_size):
    """The whole fixture: the raw rows as multisets with counts and statuses;
    the public list without and with the minimal filter, unpacked and packed,
    in the public order."""
    cases, grids = grids_of()
    total = sum(sum(c.rows(max_size).values()) for c in cases)
    rows, count, status, info = raw(solver, grids, max_size, total)
    assert info == (total, total)
    assert_rows(cases, rows, count, status, max_size)
    with pytest.raises(Exception, match="3 of 24"):
        solver.unavoidable(torch.from_numpy(grids.copy()), max_size=max_size)
    every, _, (st,) = public(solver, grids, max_size=max_size, minimal=False, return_status=True)
    least, _, (st2,) = public(solver, grids, max_size=max_size, return_status=True)
    packed, _, _ = public(solver, grids, max_size=max_size, packed=True, return_status=True)
    assert st.cpu().tolist() == [c.status for c in cases] == st2.cpu().tolist()
    for i, c in enumerate(cases):
        assert every[i] == sorted(c.rows(max_size), key=U.sort_key), c.name
        assert least[i] == c.minimal(max_size) == packed[i], c.name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(solver, n):
    """max_size 8, the fixture's grids in turn from a place that moves with
    n, the three bad grids among them."""
    cases, grids = grids_of()
    idx = (np.arange(n) * 5 + n) % len(cases)
    picked = [cases[i] for i in idx]
    if n >= 63:
        assert {c.status for c in picked} == {U.DONE, U.INVALID, U.NOT_A_GRID}
    rows, count, status, (total, listed) = raw(solver, grids[idx], 8, 1 << 16)
    assert total == listed
    assert_rows(picked, rows, count, status, 8)


@pytest.mark.parametrize("max_size,names", [(14, ("cyclic", "hard17_0", "random_0", "random_5")), (16, ("cyclic", "random_0"))])
def test_against_the_host_build(solver, max_size, names):
    cases, grids = grids_of(names)
    host = native_build.host_lib("ua_host", openmp=True)
    hrows, hcount, hstatus, (htotal, hlisted), _ = run_host(host, grids, max_size, capacity=1 << 17)
    assert htotal == hlisted
    rows, count, status, info = raw(solver, grids, max_size, htotal)
    assert info == (htotal, htotal) and np.array_equal(count, hcount) and np.array_equal(status, hstatus)
    want = U.by_owner(hrows, len(cases))
    assert_rows(cases, rows, count, status, max_size, want=want)
    # the minimal sets: the filter entry on the device against its host model (test_ua_host.py pins that to the
    # subset definition) on the host's distinct rows
    least, _, _ = public(solver, grids, max_size=max_size)
    for i, c in enumerate(cases):
        masks = sorted(want[i], key=U.sort_key)
        keep = host_minimal(host, U.rows_to_words(masks), [0, len(masks)])
        assert least[i] == [m for m, k in zip(masks, keep) if k], c.name


def test_wave_counts(solver):
    """max_waves 1, 2, 7 and 0: the same multiset and counts (max_size 10,
    six grids and the bad ones)."""
    cases, grids = grids_of(("cyclic", "hard17_3", "hard17_7", "random_1", "random_2", "random_6", "byte_0", "row_repeat"))
    for w in (1, 2, 7, 0):
        rows, count, status, (total, listed) = raw(solver, grids, 10, 1 << 12, max_waves=w)
        assert total == listed
        assert_rows(cases, rows, count, status, 10)
    least, _, _ = public(solver, grids, max_size=10, max_waves=1, return_status=True)
    assert least == [c.minimal(10) for c in cases]


class _Raw:
    """sdk_unavoidable_batch at max_size 9 on every grid of the fixture:
    arguments carved from guarded arenas, the grids at an odd address, the
    list exactly `capacity` rows, the scratch exactly as large as asked and 8-
    but not 16-byte aligned."""

    def __init__(self, solver, capacity=None):
        self.solver, self.L = solver, solver.lib
        self.cases, self.grids = grids_of()
        self.n = n = len(self.cases)
        self.total = sum(sum(c.rows(9).values()) for c in self.cases)
        self.capacity = self.total if capacity is None else capacity
        self.need = int(self.L.sdk_unavoidable_scratch_bytes(n, 0))
        assert self.need == 64 + 128 * n
        self.ain = Arena(solver.device, IN_FILL, 81 * n + (1 << 16))
        self.aout = Arena(solver.device, OUT_FILL, 2 * (16 * self.capacity + 8 * n + 16) + (1 << 16))
        self.asc = Arena(solver.device, OUT_FILL, self.need + (1 << 16))
        self.g = self.ain.boards(n, 3, name="grids")
        self.real = torch.from_numpy(self.grids.copy()).to(solver.device)
        self.outs, self.other = self.carve_outs(""), self.carve_outs(" (second)")
        self.asc.carve(8, name="pad")
        self.sc = self.asc.carve(self.need, align=8, name="scratch")
        if self.sc.data_ptr() % 16 == 0:
            self.asc.carve(8, name="pad2")
            self.sc = self.asc.carve(self.need, align=8, name="scratch (odd)")
        assert self.sc.data_ptr() % 16 == 8

    def carve_outs(self, tag):
        n, a = self.n, self.aout
        return [a.carve(16 * max(self.capacity, 1), align=16, name="rows" + tag), a.carve(4 * n, itemsize=4, name="count" + tag),
                a.carve(4 * n, itemsize=4, name="status" + tag), a.carve(16, itemsize=8, name="info" + tag)]

    def call(self, outs, stream=None, **kw):
        a = dict(g=self.g.data_ptr(), n=self.n, m=9, r=outs[0].data_ptr(), cap=self.capacity, c=outs[1].data_ptr(),
                 s=outs[2].data_ptr(), i=outs[3].data_ptr(), sc=self.sc.data_ptr(), nb=self.need, w=0)
        a.update(kw)
        with torch.cuda.device(self.solver.device):
            return self.L.sdk_unavoidable_batch(a["g"], a["n"], a["m"], a["r"], a["cap"], a["c"], a["s"], a["i"], a["sc"],
                                                a["nb"], a["w"], _stream_handle(self.solver, stream))

    def check(self, got):
        rows, count, status, info = (t.cpu().numpy() for t in got)
        assert info.tolist() == [self.total, min(self.total, self.capacity)]
        rows = rows.view(np.uint32).reshape(-1, 4)[:int(info[1])]
        assert status.tolist() == [c.status for c in self.cases]
        assert count.tolist() == [sum(c.rows(9).values()) for c in self.cases]
        have = U.by_owner(rows, self.n) if len(rows) == 0 or rows[:, 3].max() < self.n else None
        assert have is not None
        for i, c in enumerate(self.cases):
            want = c.rows(9)
            if self.capacity >= self.total:
                assert have[i] == want, c.name
            else:  # what was dropped is unspecified: a sub-multiset
                assert not have[i] - want, c.name
        assert sum(sum(h.values()) for h in have) == int(info[1])

    def finish(self):
        torch.cuda.synchronize()
        for a in (self.ain, self.aout, self.asc):
            a.assert_guards()
        assert np.array_equal(self.g.cpu().numpy(), self.grids)


@pytest.mark.parametrize("short", [None, 1, 0])
def test_capacity_in_a_guarded_arena(solver, short):
    """capacity total, total - 1 and 0: counts and info whatever the
    capacity, rows [0, listed) all written, nothing beyond them (the list's
    region ends at row `capacity`: the guards behind it stay)."""
    total = _Raw(solver).total
    r = _Raw(solver, capacity=total if short is None else total - 1 if short else 0)
    r.g.copy_(r.real)
    assert r.call(r.outs, **(dict(r=None) if short == 0 else {})) == 0
    torch.cuda.synchronize()
    if short == 0:
        assert (r.outs[0] == OUT_FILL).all()
    else:
        rows = r.outs[0].cpu().numpy().view(np.uint32).reshape(-1, 4)
        assert not (rows == FILL32).all(axis=1).any()  # no hole
    r.check(r.outs)
    r.finish()


def test_retry_and_explicit_capacity(solver, monkeypatch):
    """A first guess that overflows is asked for again in full and equals
    the fixture; an explicit capacity that overflows raises with the number to
    ask for, and that number works."""
    from sudoku_solver_distributed_amd import solver as S
    cases, grids = grids_of(("cyclic", "hard17_1", "random_3", "random_4"))
    want = [c.minimal(12) for c in cases]
    monkeypatch.setitem(S.UA_CAPACITY, 12, 7)
    assert public(solver, grids, max_size=12)[0] == want
    monkeypatch.undo()
    assert S.UA_CAPACITY[12] == 2 * max(sum(c.rows12.values()) for c in U.valid_cases())
    assert S.UA_CAPACITY[9] == 2 * max(sum(c.rows(9).values()) for c in U.valid_cases())
    assert public(solver, grids, max_size=12)[0] == want
    total = sum(sum(c.rows12.values()) for c in cases)
    with pytest.raises(Exception, match=f"capacity={total}\\)"):
        public(solver, grids, max_size=12, capacity=total - 1)
    assert public(solver, grids, max_size=12, capacity=total)[0] == want
    for bad in (dict(max_size=3), dict(max_size=17), dict(max_waves=-1), dict(capacity=-1)):
        with pytest.raises(ValueError):
            solver.unavoidable(torch.from_numpy(grids.copy()), **bad)
    sets, offsets = solver.unavoidable(torch.zeros((0, 81), dtype=torch.uint8))
    assert sets.shape == (0, 81) and offsets.tolist() == [0]


def test_abi_two_calls_on_one_scratch(solver):
    r = _Raw(solver)
    r.g.copy_(r.real)
    assert r.call(r.outs) == 0 and r.call(r.other) == 0
    torch.cuda.synchronize()
    r.check(r.outs)
    r.check(r.other)
    r.finish()


def test_abi_bad_arguments_write_nothing(solver):
    r = _Raw(solver)
    r.g.copy_(r.real)
    before = r.aout.buf.clone()
    for kw in (dict(m=3), dict(m=17), dict(n=-1), dict(n=1 << 31), dict(cap=-1), dict(w=-1), dict(nb=r.need - 1),
               dict(g=None), dict(r=None), dict(c=None), dict(s=None), dict(i=None), dict(sc=None),
               dict(r=r.outs[0].data_ptr() + 8), dict(c=r.outs[1].data_ptr() + 2), dict(s=r.outs[2].data_ptr() + 1),
               dict(i=r.outs[3].data_ptr() + 4), dict(sc=r.sc.data_ptr() + 4)):
        assert r.call(r.outs, **kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.equal(r.aout.buf, before)
    assert (r.sc == OUT_FILL).all()
    r.finish()


def test_abi_poisoned_scratch(solver):
    """The scratch pre-filled with 0xFF and with random bytes: the heads and
    the masks are the call's own to arm."""
    r = _Raw(solver)
    r.g.copy_(r.real)
    for what, fill in _poisons(r.sc):
        fill()
        for v in r.outs:
            v.view(torch.uint8).fill_(OUT_FILL)
        assert r.call(r.outs) == 0, what
        torch.cuda.synchronize()
        r.check(r.outs)
    r.finish()


def test_abi_stream_order(solver):
    """The call on a side stream behind a delay and behind the copy that
    brings its inputs: every launch and the re-arming memset are on that
    stream."""
    r = _Raw(solver)

    def call(side):
        assert r.call(r.outs, stream=side) == 0

    def dirty(side):
        assert r.call(r.other, stream=side) == 0
    got = _on_side_stream(solver, "unavoidable", [(r.g, r.real)], call, r.outs, scratch=(r.sc,), dirty=dirty)
    r.check(got)
    r.finish()


def test_minimal_entry_on_shuffled_groups(solver):
    """sdk_unavoidable_minimal_batch as it is, on groups with duplicates, an
    empty group and groups around the tile of 64 rows, at max_waves 0, 1 and
    3: keep by the definition in Python ints; nothing beyond keep written."""
    rng = np.random.default_rng(42)
    cases = U.valid_cases()
    groups = []
    for c, size in ((cases[0], 12), (cases[5], 10), (cases[14], 12)):
        masks = list(c.rows(size).elements())
        masks += [masks[k] for k in rng.integers(0, len(masks), 30)]
        groups.append([masks[k] for k in rng.permutation(len(masks))])
    base = groups[1]
    groups += [[], base[:63], base[:64], base[:65], [0b1111, 0b0111, 0b0111, 1 << 80 | 0b0111, 1 << 80], [(1 << 81) - 1]]
    rows = np.concatenate([U.rows_to_words(g, owner=7) for g in groups if g])
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    want = np.concatenate([[int(not any((g[j] == g[k] and j < k) or (g[j] != g[k] and g[j] & ~g[k] == 0)
                                        for j in range(len(g)))) for k in range(len(g))] for g in groups if g])
    d_rows = torch.from_numpy(rows.view(np.int32)).to(solver.device)
    d_off = torch.from_numpy(offsets).to(solver.device)
    for w in (0, 1, 3):
        keep = torch.full((len(rows) + 64,), 77, dtype=torch.uint8, device=solver.device)
        with torch.cuda.device(solver.device):
            assert solver.lib.sdk_unavoidable_minimal_batch(d_rows.data_ptr(), d_off.data_ptr(), len(groups), keep.data_ptr(), w,
                                                            _stream_handle(solver)) == 0
        torch.cuda.synchronize()
        got = keep.cpu().numpy()
        assert (got[len(rows):] == 77).all() and np.array_equal(got[:len(rows)], want), w


def test_symmetry_images(solver):
    """The sets of a gen.apply_symmetry image are the cell images of the
    grid's sets (image cell k takes cell src[k]), rows and minimal sets alike;
    relabelling the digits changes nothing at all.  Six grids at max_size 10."""
    from sudoku_solver_distributed_amd import gen
    cases, grids = grids_of(("cyclic", "hard17_2", "hard17_9", "random_1", "random_4", "random_7"))
    rng = np.random.default_rng(2424)
    syms = rng.integers(0, 3359232, len(cases))
    images, maps = gen.apply_symmetry(grids, syms)
    moved = 0
    rows, count, status, _ = raw(solver, images, 10, 1 << 12)
    got = U.by_owner(rows, len(cases))
    least, _, _ = public(solver, images, max_size=10)
    for i, c in enumerate(cases):
        src, _ = Y.from_number(syms[i], maps[i])
        image = lambda m: U.mask_of(k for k in range(81) if (m >> int(src[k])) & 1)
        assert got[i] == Counter({image(m): v for m, v in c.rows(10).items()}), c.name
        assert least[i] == sorted((image(m) for m in c.minimal(10)), key=U.sort_key), c.name
        moved += least[i] != c.minimal(10)
    assert moved >= 4
    pi = np.concatenate([[0], 1 + rng.permutation(9)]).astype(np.uint8)
    a = solver.unavoidable(torch.from_numpy(grids.copy()), max_size=10)
    b = solver.unavoidable(torch.from_numpy(pi[grids]), max_size=10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cross_entries(solver):
    """Eight grids at max_size 10, the definitions through other entries:
    every listed set erased from its grid has at least two completions, each
    other than the grid differing from it on the whole set; every unique_batch
    puzzle hits every set of its solution, and with the clues of one set erased
    count_solutions answers 2 and hits_unavoidable False; the greedy bound is
    the Python greedy's, at most 17 on the hard17 grids and at most the clues
    of every minimize output."""
    from sudoku_solver_distributed_amd import gen
    cases, grids = grids_of(tuple(f"random_{k}" for k in range(8)))
    dg = torch.from_numpy(grids.copy()).to(solver.device)
    sets, offsets = solver.unavoidable(dg, max_size=10)
    owner = torch.repeat_interleave(torch.arange(len(cases), device=solver.device), offsets[1:] - offsets[:-1])
    erased = dg[owner].clone()
    erased[sets.bool()] = 0
    comp, coff = solver.completions(erased)
    per = (coff[1:] - coff[:-1]).cpu().numpy()
    assert len(per) == sets.shape[0] >= 8 * 60 and (per >= 2).all()
    which = torch.repeat_interleave(torch.arange(sets.shape[0], device=solver.device), coff[1:] - coff[:-1])
    differs = comp != dg[owner][which]
    same = ~differs.any(dim=1)
    assert int(same.sum()) == sets.shape[0]                      # the grid itself, once a set
    assert bool((differs[~same] == sets.bool()[which][~same]).all())  # every other one: on the whole set, nowhere else

    puzzles, full = gen.unique_batch(32, seed=5, return_solutions=True)
    psets, poff = solver.unavoidable(full, max_size=10)
    assert bool(gen.hits_unavoidable(puzzles, psets, poff).all())
    assert bool(gen.hits_unavoidable(puzzles, solver.unavoidable(full, max_size=10, packed=True)[0], poff).all())
    one = psets[poff[:-1] + (poff[1:] - poff[:-1]) // 2].bool()  # a set from the middle of every grid's list
    holed = puzzles.clone()
    holed[one] = 0
    assert solver.count_solutions(holed, limit=2).tolist() == [2] * 32
    assert not bool(gen.hits_unavoidable(holed, psets, poff).any())

    def greedy(masks):
        used, k = 0, 0
        for m in masks:
            if not m & used:
                used, k = used | m, k + 1
        return k
    hard, hgrids = grids_of(tuple(f"hard17_{k}" for k in range(12)))
    bound = gen.clue_lower_bound(torch.from_numpy(hgrids.copy())).tolist()
    assert bound == [greedy(c.minimal(12)) for c in hard] and max(bound) <= 17
    b10 = gen.clue_lower_bound(dg, max_size=10)
    assert b10.tolist() == [greedy(c.minimal(10)) for c in cases]
    rng = np.random.default_rng(10)
    for _ in range(3):
        order = torch.from_numpy(np.stack([rng.permutation(81) for _ in cases]).astype(np.uint8))
        out, st = solver.minimize(dg, order=order)
        assert bool((st == 1).all()) and bool(((out != 0).sum(dim=1) >= b10).all())
