"""GPU tests of the hitting sets (BatchSolver.hitting_sets,
BatchSolver.sub_puzzles, sdk_hitting_sets_batch, gen.min_hitting_clues,
gen.smallest_sub_puzzles, gen.neighbourhood) against the
fixture tests/golden/hit_cases.json -- brute force and the cell-by-cell
restatement -- the definitions recomputed through other entries
(count_solutions, unique_batch, exchange, minimize, hits_unavoidable) and the
C ABI's contracts.  Rows are compared as sets, everything else by equality."""
import functools
from math import comb

import numpy as np
import pytest
import torch

import hit_cases as H
import symmetry_cases as Y
import ua_cases as U
from abi_arena import IN_FILL, OUT_FILL, Arena, _on_side_stream, _poisons, _stream_handle

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
FINE_FAMILIES = 4096  # HIT_FINE_FAMILIES of hit_kernels.hip: larger batches run coarse tasks


def by_name(*names):
    by = {c.name: c for c in H.load_fixture()}
    return [by[n] for n in names]


def with_k(k):
    return [c for c in H.load_fixture() if k in c.answers]


def raw(solver, cases, k, capacity, limit=0, max_waves=0):
    """sdk_hitting_sets_batch as it is on these cases as one batch: (masks
    per family, count, status, (total, listed)), after a check that nothing at
    or beyond row `listed` was written and no input changed."""
    arrays = H.batch_arrays(cases)
    sets, offsets, A, R = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(solver.device) for a in arrays)
    n = len(cases)
    rows = torch.full((max(capacity, 1), 4), FILL32 - (1 << 32), dtype=torch.int32, device=solver.device)
    count = torch.full((n,), 12345, dtype=torch.int64, device=solver.device)
    status = torch.full((n,), 12345, dtype=torch.int32, device=solver.device)
    info = torch.full((2,), -7, dtype=torch.int64, device=solver.device)
    need = int(solver.lib.sdk_hitting_sets_scratch_bytes(n, max_waves))
    sc = torch.empty(need, dtype=torch.uint8, device=solver.device)
    with torch.cuda.device(solver.device):
        rc = solver.lib.sdk_hitting_sets_batch(sets.data_ptr() if sets.shape[0] else None, offsets.data_ptr(), A.data_ptr(),
                                               R.data_ptr(), n, k, limit, rows.data_ptr() if capacity else None, capacity,
                                               count.data_ptr(), status.data_ptr(), info.data_ptr(), sc.data_ptr(), need,
                                               max_waves, _stream_handle(solver))
    assert rc == 0
    torch.cuda.synchronize()
    total, listed = (int(v) for v in info.tolist())
    assert listed == min(total, capacity)
    for t, a in zip((sets, offsets, A, R), arrays):
        assert np.array_equal(t.cpu().numpy().view(a.dtype), a)
    r = rows.cpu().numpy().view(np.uint32)
    assert (r[listed:] == FILL32).all()
    assert listed == 0 or r[:listed, 3].max() < n
    got = [[] for _ in range(n)]
    for row, m in zip(r[:listed], U.words_to_masks(r[:listed])):
        got[int(row[3])].append(m)
    return got, count.cpu().numpy(), status.cpu().numpy(), (total, listed)


def public(solver, cases, k, **kw):
    """BatchSolver.hitting_sets' answer as (list of masks per family, in the
    order given; the rest)."""
    sets, offsets, A, R = H.batch_arrays(cases)
    out = solver.hitting_sets(torch.from_numpy(sets[:, :3].astype(np.int64)), torch.from_numpy(offsets), k,
                              allowed=torch.from_numpy(A[:, :3].astype(np.int64)),
                              required=torch.from_numpy(R[:, :3].astype(np.int64)), **kw)
    rows, off = out[0].cpu().numpy(), out[1].cpu().numpy()
    if kw.get("packed"):
        assert rows.dtype == np.int32 and rows.shape[1:] == (3,)
        masks = U.words_to_masks(np.concatenate([rows.view(np.uint32), np.zeros((len(rows), 1), np.uint32)], axis=1))
    else:
        assert rows.dtype == np.uint8 and rows.shape[1:] == (81,) and rows.max(initial=0) <= 1
        masks = [U.mask_of(np.nonzero(r)[0]) for r in rows]
    assert off[0] == 0 and off[-1] == len(masks) and (np.diff(off) >= 0).all() and len(off) == len(cases) + 1
    return [masks[off[i]:off[i + 1]] for i in range(len(cases))], out[2:]


def test_fixture(solver):
    """The whole fixture, one call a k: the raw rows as sets with counts and
    statuses where a case lists at most 2^16, the pure count everywhere (the
    tau cases' large ones included), and the public list in the public order,
    unpacked and packed."""
    cases = H.load_fixture()
    for k in sorted({k for c in cases for k in c.answers}):
        group = with_k(k)
        want = [c.answers[k][0] for c in group]
        got, count, status, (total, listed) = raw(solver, group, k, 0)
        assert (total, listed) == (sum(want), 0) and count.tolist() == want, k
        assert status.tolist() == [c.status for c in group], k
        listed_cases = [c for c in group if c.answers[k][0] <= 1 << 16]
        total = sum(c.answers[k][0] for c in listed_cases)
        got, count, status, info = raw(solver, listed_cases, k, total)
        assert info == (total, total)
        for i, c in enumerate(listed_cases):
            H.check_answer(c, k, got[i], int(count[i]), int(status[i]))
    group = [c for c in with_k(3) if c.answers[3][1] is not None]
    assert {c.status for c in group} == {H.DONE, H.INVALID}
    with pytest.raises(Exception, match="3 of %d" % len(group)):
        public(solver, group, 3)
    plain, (st,) = public(solver, group, 3, return_status=True)
    packed, (st2, cnt) = public(solver, group, 3, packed=True, return_status=True, return_count=True)
    assert st.cpu().tolist() == [c.status for c in group] == st2.cpu().tolist()
    assert cnt.cpu().tolist() == [c.answers[3][0] for c in group]
    for i, c in enumerate(group):
        assert plain[i] == c.answers[3][1] == packed[i], c.name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, FINE_FAMILIES + 1])
def test_batch_sizes(solver, n):
    """k = 3, the fixture's cases that record it in turn from a place that
    moves with n, invalid and empty families among them; the largest batch
    runs the coarse task cut."""
    pool = [c for c in with_k(3) if c.answers[3][1] is not None]
    idx = (np.arange(n) * 7 + n) % len(pool)  # (ten cases: every one in turn)
    picked = [pool[i] for i in idx]
    if n >= 63:
        assert {c.status for c in picked} == {H.DONE, H.INVALID} and any(not c.sets for c in picked)
    total = sum(c.answers[3][0] for c in picked)
    got, count, status, info = raw(solver, picked, 3, total)
    assert info == (total, total)
    for i in (range(n) if n <= 257 else range(0, n, 37)):
        H.check_answer(picked[i], 3, got[i], int(count[i]), int(status[i]))
    assert count.tolist() == [c.answers[3][0] for c in picked]


def test_wave_counts(solver):
    """max_waves 1, 2, 7 and 0: the same rows and counts (k = 17: the hard17
    families at 6 and 12 cells, with and without required cells)."""
    group = with_k(17)
    assert len(group) >= 12
    total = sum(c.answers[17][0] for c in group)
    for w in (1, 2, 7, 0):
        got, count, status, info = raw(solver, group, 17, total, max_waves=w)
        assert info == (total, total)
        for i, c in enumerate(group):
            H.check_answer(c, 17, got[i], int(count[i]), int(status[i]))
    rows, _ = public(solver, group, 17, max_waves=1)
    assert [len(r) for r in rows] == [c.answers[17][0] for c in group]


def test_limit(solver):
    """limit = 1, 2 and count - 1: count == limit, SDK_HIT_LIMITED, every
    listed row one of the full list; at the count itself LIMITED still, above
    it DONE."""
    for c in by_name("cyclic", "hard17_1_at12", "random_2_at6", "edge_cells", "empty_family"):
        k = max(c.answers, key=lambda kk: c.answers[kk][0] if c.answers[kk][1] is not None else -1)
        full, rows, _ = c.answers[k]
        for limit in (1, 2, full - 1, full, full + 1):
            for capacity in (full, 0):
                got, count, status, (total, listed) = raw(solver, [c], k, capacity, limit=limit)
                want = min(limit, full)
                assert count[0] == total == want and listed == min(want, capacity), (c.name, limit)
                assert status[0] == (H.LIMITED if limit <= full else H.DONE), (c.name, limit)
                assert len(set(got[0])) == listed and set(got[0]) <= set(rows), (c.name, limit)
    group = with_k(17)
    got, count, status, (total, listed) = raw(solver, group, 17, len(group), limit=1)
    want = [min(1, c.answers[17][0]) for c in group]
    assert count.tolist() == want and total == listed == sum(want)
    assert status.tolist() == [H.LIMITED if w else c.status for w, c in zip(want, group)]
    assert all(set(g) <= set(c.answers[17][1] or g) and len(g) == w for g, c, w in zip(got, group, want))


def test_k_at_the_largest_size(solver):
    """k = SDK_HIT_MAX_CLUES = 32 (and 31) on the family whose rows are few."""
    (c,) = by_name("k32")
    for k in (31, 32):
        got, count, status, _ = raw(solver, [c], k, 64)
        H.check_answer(c, k, got[0], int(count[0]), int(status[0]))
    rows, _ = public(solver, [c], 32)
    assert rows[0] == c.answers[32][1]


class _Raw:
    """sdk_hitting_sets_batch at k = 17 on every case that records it:
    arguments carved from guarded arenas, the list exactly `capacity` rows,
    the scratch exactly as large as asked and 8- but not 16-byte aligned."""

    def __init__(self, solver, capacity=None):
        self.solver, self.L = solver, solver.lib
        self.cases = with_k(17)
        self.n = n = len(self.cases)
        self.arrays = H.batch_arrays(self.cases)
        self.total = sum(c.answers[17][0] for c in self.cases)
        self.capacity = self.total if capacity is None else capacity
        self.need = int(self.L.sdk_hitting_sets_scratch_bytes(n, 0))
        assert self.need == 64
        nin = sum(a.nbytes for a in self.arrays)
        self.ain = Arena(solver.device, IN_FILL, nin + (1 << 16))
        self.aout = Arena(solver.device, OUT_FILL, 2 * (16 * self.capacity + 12 * n + 16) + (1 << 16))
        self.asc = Arena(solver.device, OUT_FILL, self.need + (1 << 16))
        self.ins = [self.ain.carve(a.nbytes, align=16 if j != 1 else 8, name=name)
                    for j, (a, name) in enumerate(zip(self.arrays, ("sets", "offsets", "allowed", "required")))]
        self.real = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(solver.device) for a in self.arrays]
        self.outs, self.other = self.carve_outs(""), self.carve_outs(" (second)")
        self.asc.carve(8, name="pad")
        self.sc = self.asc.carve(self.need, align=8, name="scratch")
        if self.sc.data_ptr() % 16 == 0:
            self.asc.carve(8, name="pad2")
            self.sc = self.asc.carve(self.need, align=8, name="scratch (odd)")
        assert self.sc.data_ptr() % 16 == 8

    def carve_outs(self, tag):
        n, a = self.n, self.aout
        return [a.carve(16 * max(self.capacity, 1), align=16, name="rows" + tag), a.carve(8 * n, itemsize=8, name="count" + tag),
                a.carve(4 * n, itemsize=4, name="status" + tag), a.carve(16, itemsize=8, name="info" + tag)]

    def load(self):
        for v, t in zip(self.ins, self.real):
            v.copy_(t)

    def call(self, outs, stream=None, **kw):
        a = dict(s=self.ins[0].data_ptr(), o=self.ins[1].data_ptr(), a=self.ins[2].data_ptr(), q=self.ins[3].data_ptr(),
                 n=self.n, k=17, lim=0, r=outs[0].data_ptr(), cap=self.capacity, c=outs[1].data_ptr(), st=outs[2].data_ptr(),
                 i=outs[3].data_ptr(), sc=self.sc.data_ptr(), nb=self.need, w=0)
        a.update(kw)
        with torch.cuda.device(self.solver.device):
            return self.L.sdk_hitting_sets_batch(a["s"], a["o"], a["a"], a["q"], a["n"], a["k"], a["lim"], a["r"], a["cap"],
                                                 a["c"], a["st"], a["i"], a["sc"], a["nb"], a["w"],
                                                 _stream_handle(self.solver, stream))

    def check(self, got):
        rows, count, status, info = (t.cpu().numpy() for t in got)
        assert info.tolist() == [self.total, min(self.total, self.capacity)]
        rows = rows.view(np.uint32).reshape(-1, 4)[:int(info[1])]
        assert status.tolist() == [c.status for c in self.cases]
        assert count.tolist() == [c.answers[17][0] for c in self.cases]
        assert len(rows) == 0 or rows[:, 3].max() < self.n
        have = [[] for _ in self.cases]
        for r, m in zip(rows, U.words_to_masks(rows)):
            have[int(r[3])].append(m)
        for h, c in zip(have, self.cases):
            want = c.answers[17][1]
            assert len(set(h)) == len(h), c.name
            if self.capacity >= self.total:
                assert len(h) == c.answers[17][0] and (want is None or sorted(h, key=U.sort_key) == want), c.name
            else:  # what was dropped is unspecified: a subset
                assert want is None or set(h) <= set(want), c.name

    def finish(self):
        torch.cuda.synchronize()
        for a in (self.ain, self.aout, self.asc):
            a.assert_guards()
        for v, t in zip(self.ins, self.real):
            assert torch.equal(v, t)


@pytest.mark.parametrize("short", [None, 1, 0])
def test_capacity_in_a_guarded_arena(solver, short):
    """capacity total, total - 1 and 0: counts and info whatever the
    capacity, rows [0, listed) all written, nothing beyond them."""
    total = _Raw(solver).total
    r = _Raw(solver, capacity=total if short is None else total - 1 if short else 0)
    r.load()
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
    ask for, and that number works; capacity 0 lists nothing and counts."""
    from sudoku_solver_distributed_amd import solver as S
    group = by_name("hard17_0_at12", "hard17_1_at6", "edge_cells", "hard17_2_required")
    k = 17
    group = [c for c in group if k in c.answers]
    want = [c.answers[k][0] for c in group]
    monkeypatch.setattr(S, "HIT_CAPACITY", 7)
    rows, _ = public(solver, group, k)
    assert [len(r) for r in rows] == want
    monkeypatch.undo()
    again, _ = public(solver, group, k)
    assert again == rows and all(r == c.answers[k][1] for r, c in zip(rows, group) if c.answers[k][1] is not None)
    total = sum(want)
    with pytest.raises(Exception, match=f"capacity={total}\\)"):
        public(solver, group, k, capacity=total - 1)
    assert public(solver, group, k, capacity=total)[0] == rows
    none, (cnt,) = public(solver, group, k, capacity=0, return_count=True)
    assert none == [[] for _ in group] and cnt.cpu().tolist() == want
    for bad in (dict(k=-1), dict(k=33), dict(max_waves=-1), dict(capacity=-1), dict(limit=-1)):
        with pytest.raises(ValueError):
            public(solver, group, **dict(dict(k=k), **bad))
    rows, offsets = solver.hitting_sets(torch.zeros((0, 81), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), 5)
    assert rows.shape == (0, 81) and offsets.tolist() == [0]
    # the (S, 81) form of the sets and the masks, None for both masks: the empty family's C(81, 2) rows among them
    (c,) = by_name("edge_cells")
    cells = np.array([[m >> x & 1 for x in range(81)] for m in c.sets], dtype=np.uint8)
    rows, off = solver.hitting_sets(torch.from_numpy(cells), torch.tensor([0, 0, len(c.sets)]), 2)
    assert off.tolist() == [0, comb(81, 2), comb(81, 2) + len(H.brute_rows(c.sets, H.ALL81, 0, 2) or H.restated_rows(c.sets, H.ALL81, 0, 2))]
    mask = torch.from_numpy(np.array([c.A >> x & 1 for x in range(81)], dtype=np.uint8))
    rows, off = solver.hitting_sets(torch.from_numpy(cells), torch.tensor([0, len(c.sets)]), 3, allowed=mask)
    assert [U.mask_of(np.nonzero(r)[0]) for r in rows.cpu().numpy()] == c.answers[3][1]


def test_abi_two_calls_on_one_scratch(solver):
    r = _Raw(solver)
    r.load()
    assert r.call(r.outs) == 0 and r.call(r.other) == 0
    torch.cuda.synchronize()
    r.check(r.outs)
    r.check(r.other)
    r.finish()


def test_abi_bad_arguments_write_nothing(solver):
    r = _Raw(solver)
    r.load()
    before = r.aout.buf.clone()
    for kw in (dict(k=-1), dict(k=33), dict(n=-1), dict(n=1 << 31), dict(cap=-1), dict(w=-1), dict(lim=-1), dict(nb=r.need - 1),
               dict(o=None), dict(a=None), dict(q=None), dict(r=None), dict(c=None), dict(st=None), dict(i=None), dict(sc=None),
               dict(s=r.ins[0].data_ptr() + 8), dict(a=r.ins[2].data_ptr() + 8), dict(q=r.ins[3].data_ptr() + 4),
               dict(o=r.ins[1].data_ptr() + 4), dict(r=r.outs[0].data_ptr() + 8), dict(c=r.outs[1].data_ptr() + 4),
               dict(st=r.outs[2].data_ptr() + 1), dict(i=r.outs[3].data_ptr() + 4), dict(sc=r.sc.data_ptr() + 4)):
        assert r.call(r.outs, **kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.equal(r.aout.buf, before)
    assert (r.sc == OUT_FILL).all()
    r.finish()


def test_abi_poisoned_scratch(solver):
    """The scratch pre-filled with 0xFF and with random bytes: the heads are
    the call's own to arm."""
    r = _Raw(solver)
    r.load()
    for what, fill in _poisons(r.sc):
        fill()
        for v in r.outs:
            v.view(torch.uint8).fill_(OUT_FILL)
        assert r.call(r.outs) == 0, what
        torch.cuda.synchronize()
        r.check(r.outs)
    r.finish()


def test_abi_stream_order(solver):
    """The call on a side stream behind a delay and behind the copies that
    bring its inputs: every launch and the re-arming memset are on that
    stream."""
    r = _Raw(solver)

    def call(side):
        assert r.call(r.outs, stream=side) == 0

    def dirty(side):
        assert r.call(r.other, stream=side) == 0
    # (0xFF inputs: offsets of -1 everywhere make every family empty, allowed with bit 81 makes it invalid)
    got = _on_side_stream(solver, "hitting_sets", list(zip(r.ins, r.real)), call, r.outs, scratch=(r.sc,), dirty=dirty)
    r.check(got)
    r.finish()


# ------------------------------------------------------------ across entries
@functools.lru_cache(maxsize=None)
def _proper(n=32, seed=5):
    from sudoku_solver_distributed_amd import gen
    puzzles, full = gen.unique_batch(n, seed=seed, return_solutions=True)
    return puzzles, full


def _board_set(t):
    return {bytes(r) for r in t.cpu().numpy()}


def test_sub_puzzles_inside_a_superset(solver):
    """32 unique_batch puzzles P, Q = P plus 5 more of the grid's digits:
    sub_puzzles(grid, |P|, allowed=Q) is the brute force over all C(|Q|, 5)
    erasures answered by count_solutions, holds P, and every row passes
    hits_unavoidable."""
    from sudoku_solver_distributed_amd import gen
    puzzles, full = _proper()
    rng = np.random.default_rng(55)
    q = puzzles.clone()
    for i in range(q.shape[0]):
        empty = np.nonzero(puzzles[i].cpu().numpy() == 0)[0]
        add = torch.from_numpy(rng.choice(empty, 5, replace=False)).to(q.device)
        q[i, add] = full[i, add]
    clues = (puzzles != 0).sum(dim=1)
    sets12 = solver.unavoidable(full, max_size=12, packed=True)
    for k in sorted(set(clues.tolist())):
        idx = torch.nonzero(clues == k)[:, 0]
        sub, off = solver.sub_puzzles(full[idx], k, allowed=(q[idx] != 0).to(torch.uint8), max_size=8)
        for j, i in enumerate(idx.tolist()):
            cells = torch.nonzero(q[i])[:, 0]
            drop = torch.combinations(torch.arange(k + 5, device=q.device), 5)
            boards = q[i].repeat(drop.shape[0], 1)
            boards[torch.arange(drop.shape[0], device=q.device).unsqueeze(1), cells[drop]] = 0
            want = boards[solver.count_solutions(boards, limit=2) == 1]
            mine = sub[off[j]:off[j + 1]]
            assert _board_set(mine) == _board_set(want) and mine.shape[0] == want.shape[0], i
            assert bytes(puzzles[i].cpu().numpy()) in _board_set(mine), i
            one = (sets12[0][sets12[1][i]:sets12[1][i + 1]], torch.tensor([0, int(sets12[1][i + 1] - sets12[1][i])]))
            for b in mine[:8]:
                assert bool(gen.hits_unavoidable(b[None], one[0], one[1].to(b.device)).all())


def test_sub_puzzles_with_required_cells(solver):
    """required = P minus 2 clues, A all cells, k = |P|: the brute force over
    the C(83 - |P|, 2) boards that add two of the grid's digits."""
    puzzles, full = _proper()
    clues = (puzzles != 0).sum(dim=1)
    for k in sorted(set(clues.tolist()))[:3]:
        idx = torch.nonzero(clues == k)[:, 0]
        req = puzzles[idx].clone()
        for j in range(idx.shape[0]):
            cells = torch.nonzero(req[j])[:, 0]
            req[j, cells[[1, k // 2]]] = 0
        sub, off = solver.sub_puzzles(full[idx], k, required=(req != 0).to(torch.uint8))
        for j, i in enumerate(idx.tolist()):
            empty = torch.nonzero(req[j] == 0)[:, 0]
            assert empty.shape[0] == 83 - k
            add = torch.combinations(torch.arange(83 - k, device=req.device), 2)
            boards = req[j].repeat(add.shape[0], 1)
            at = torch.arange(add.shape[0], device=req.device).unsqueeze(1)
            boards[at, empty[add]] = full[i][empty[add]]
            want = boards[solver.count_solutions(boards, limit=2) == 1]
            mine = sub[off[j]:off[j + 1]]
            assert _board_set(mine) == _board_set(want) and mine.shape[0] == want.shape[0], i
            assert bytes(puzzles[i].cpu().numpy()) in _board_set(mine)


def test_neighbourhood_at_one_is_exchange(solver):
    """neighbourhood(P, 1) against exchange(P)'s neighbours as sets of boards
    per parent, the parent itself in neither; a board with two completions
    contributes nothing.  exchange adds any digit that leaves one completion,
    so some of its neighbours complete to ANOTHER grid than their parent;
    neighbourhood, built on the parent's grid's unavoidable sets, lists the
    neighbours inside that grid.  So: exchange's neighbours are neighbourhood's
    and, besides them, only boards whose completion differs from the parent's
    -- exactly, both ways."""
    from sudoku_solver_distributed_amd import gen
    puzzles, full = _proper()
    p = puzzles[:6].clone()
    p[5, torch.nonzero(p[5])[0, 0]] = 0  # a minimal puzzle less a clue: several completions
    nb, parent = gen.neighbourhood(p, 1)
    ex, ex_parent = gen.exchange(p)[:2]
    cnt, grid = solver.count_solutions(ex, limit=2, return_first=True)
    assert cnt.tolist() == [1] * ex.shape[0]
    inside = (grid == full[ex_parent]).all(dim=1)
    assert 0 < int(inside.sum()) and 5 not in set(parent.tolist()) | set(ex_parent.tolist())
    print("exchange neighbours: %d, of them inside the parent's grid: %d" % (ex.shape[0], int(inside.sum())))
    for i in range(5):
        mine, want, other = nb[parent == i], ex[(ex_parent == i) & inside], ex[(ex_parent == i) & ~inside]
        assert _board_set(mine) == _board_set(want) and mine.shape[0] == len(_board_set(want)), i
        assert not _board_set(mine) & _board_set(other)
        assert bytes(p[i].cpu().numpy()) not in _board_set(mine)
        assert bool((mine == full[i] * (mine != 0)).all()) and bool(((mine != 0).sum(dim=1) == (p[i] != 0).sum()).all())
    assert nb.shape[0] == int(inside.sum())
    with pytest.raises(ValueError):
        gen.neighbourhood(p, 4)


def test_symmetry_images(solver):
    """The sub-puzzles of a gen.apply_symmetry image, with the masks' images,
    are the images of the sub-puzzles."""
    from sudoku_solver_distributed_amd import gen
    puzzles, full = _proper()
    rng = np.random.default_rng(2525)
    n = 6
    q = puzzles[:n].clone()
    for i in range(n):
        empty = np.nonzero(puzzles[i].cpu().numpy() == 0)[0]
        add = torch.from_numpy(rng.choice(empty, 3, replace=False)).to(q.device)
        q[i, add] = full[i, add]
    syms = rng.integers(0, 3359232, n)
    images, maps = gen.apply_symmetry(full[:n].cpu().numpy(), syms)
    qimg, _ = gen.apply_symmetry(q.cpu().numpy(), syms)
    images, qimg = torch.as_tensor(images), torch.as_tensor(qimg)
    moved = 0
    for i in range(n):
        k = int((puzzles[i] != 0).sum())
        a, _ = solver.sub_puzzles(full[i:i + 1], k, allowed=(q[i:i + 1] != 0).to(torch.uint8))
        b, _ = solver.sub_puzzles(images[i:i + 1], k, allowed=(qimg[i:i + 1] != 0).to(torch.uint8))
        src, _ = Y.from_number(syms[i], maps[i])
        cells_a = {tuple(np.nonzero(r)[0]) for r in a.cpu().numpy()}
        cells_b = {tuple(np.nonzero(r)[0]) for r in b.cpu().numpy()}
        assert cells_b == {tuple(sorted(kk for kk in range(81) if int(src[kk]) in set(t))) for t in cells_a}, i
        assert len(cells_a) == a.shape[0] == b.shape[0] > 0
        assert bool((b == images[i].to(b.device) * (b != 0)).all())
        moved += cells_a != cells_b
    assert moved >= 4


def test_min_hitting_clues(solver):
    """The hitting number against the fixture's tau at max_size 6; never
    below the greedy bound, at most the clues of every minimize output, at
    most 17 on the hard17 grids."""
    from sudoku_solver_distributed_amd import gen
    real = [f"hard17_{k}" for k in range(4)] + [f"random_{k}" for k in range(4)]
    by = {c.name: c for c in H.load_fixture()}
    grids = torch.from_numpy(np.stack([c.grid for c in U.load_fixture() if c.name in real]))
    assert [c.name for c in U.load_fixture() if c.name in real] == real
    tau6 = gen.min_hitting_clues(grids, max_size=6)
    assert tau6.tolist() == [by[f"{g}_tau6"].tau for g in real]
    assert bool((tau6 >= gen.clue_lower_bound(grids, max_size=6)).all())
    tau = gen.min_hitting_clues(grids, max_size=8)
    assert bool((tau >= gen.clue_lower_bound(grids, max_size=8)).all()) and bool((tau >= tau6).all())
    assert max(tau[:4].tolist()) <= 17
    rng = np.random.default_rng(10)
    dg = grids.to(solver.device)
    for _ in range(2):
        order = torch.from_numpy(np.stack([rng.permutation(81) for _ in real]).astype(np.uint8))
        out, st = solver.minimize(dg, order=order)
        assert bool((st == 1).all()) and bool(((out != 0).sum(dim=1) >= tau).all())


def test_hard17_puzzle_among_its_grid_sub_puzzles(solver):
    """sub_puzzles at k = 17 on a hard17 grid with required = its 17-clue
    puzzle minus 3 clues holds that puzzle; neighbourhood at d = 2 holds the
    d = 1 neighbours; smallest_sub_puzzles of the puzzle plus clues is 17 or
    less and every answer is proper."""
    from sudoku_solver_distributed_amd import gen
    p = torch.from_numpy(np.array([[int(ch) for ch in gen.hard17_classes()[0]]], dtype=np.uint8)).to(solver.device)
    cnt, grid = solver.count_solutions(p, limit=2, return_first=True)
    assert cnt.tolist() == [1]
    req = p.clone()
    req[0, torch.nonzero(p[0])[[0, 7, 16], 0]] = 0
    sub, off = solver.sub_puzzles(grid, 17, required=(req != 0).to(torch.uint8))
    assert off.tolist() == [0, sub.shape[0]] and bytes(p[0].cpu().numpy()) in _board_set(sub)
    assert solver.count_solutions(sub, limit=2).tolist() == [1] * sub.shape[0]
    one, _ = gen.neighbourhood(p, 1)
    two, parent = gen.neighbourhood(p, 2)
    assert _board_set(one) <= _board_set(two) and len(_board_set(two)) == two.shape[0] and set(parent.tolist()) <= {0}
    assert bool(((two != 0).sum(dim=1) == 17).all()) and bytes(p[0].cpu().numpy()) not in _board_set(two)
    q = p.clone()
    empty = torch.nonzero(p[0] == 0)[:4, 0]
    q[0, empty] = grid[0, empty]
    k, subs, soff = gen.smallest_sub_puzzles(q)
    assert soff.tolist() == [0, subs.shape[0]] and subs.shape[0] >= 1 and k.tolist()[0] <= 17
    assert bool(((subs != 0).sum(dim=1) == k[0]).all()) and bool((subs == q * (subs != 0)).all())
    assert solver.count_solutions(subs, limit=2).tolist() == [1] * subs.shape[0]
    if k.tolist()[0] == 17:
        assert bytes(p[0].cpu().numpy()) in _board_set(subs)
