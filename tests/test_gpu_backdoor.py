"""GPU checks of the backdoor search (sdk_backdoor_batch, BatchSolver.backdoors;
runs on an MI355X) against tests/golden/backdoor_cases.json -- rate_host_batch
on every subset of the empty cells, nothing of csrc/backdoor.h in it -- on
every case and output; batches whose lanes differ; grids of 1, 2 and 7 waves;
the answers recomputed from solver.rate on the filled boards; symmetry images;
the solutions=None path; and the C ABI's buffer, scratch and stream contracts
through the raw entry.  Every check is an equality."""
import functools
from itertools import combinations

import numpy as np
import pytest
import torch

import backdoor_cases as BC
import rate_cases as R
import symmetry_cases as Y
from abi_arena import IN_FILL, OUT_FILL, Arena, _on_side_stream, _stream_handle

pytestmark = pytest.mark.gpu

RUNS = [(1, 3), (2, 3), (3, 3), (2, 1), (1, 4)]


@functools.lru_cache(maxsize=None)
def fx():
    names, boards, grids, runs = BC.load_fixture()
    for a in (boards, grids):
        a.setflags(write=False)
    return {"names": names, "boards": boards, "grids": grids, "runs": runs}


def gpu(solver, boards, grids, level, max_size, count=True, first=True, cover=True, max_waves=0):
    """(size, count, first, cover) as numpy arrays; None for an output not asked for."""
    out = solver.backdoors(torch.from_numpy(np.array(boards, dtype=np.uint8)), level=level, max_size=max_size,
                           solutions=None if grids is None else torch.from_numpy(np.array(grids, dtype=np.uint8)),
                           return_count=count, return_first=first, return_cover=cover, max_waves=max_waves)
    out = list(out) if isinstance(out, tuple) else [out]
    torch.cuda.synchronize()
    size = out.pop(0).cpu().numpy()
    c = out.pop(0).cpu().numpy() if count else None
    f = out.pop(0).cpu().numpy() if first else None
    v = out.pop(0).cpu().numpy() if cover else None
    assert not out
    return size, c, f, v


def assert_same(names, got, want):
    s, c, f, v = got
    size, count, first, cover = want
    bad = np.nonzero((s != size) | (c != count) | (f != first).any(1) | (v != cover).any(1))[0]
    assert len(bad) == 0, [(names[k], int(s[k]), int(size[k]), int(c[k]), int(count[k]), f[k].tolist(), first[k].tolist(),
                            int((v[k] != cover[k]).sum())) for k in bad[:8]]


def mix(level, max_size, n, seed=0):
    """Positions in the run of n cases drawn cyclically from every answer the
    run has (sizes, max_size + 1 and the negative codes in turn), so that a
    wave's lanes hold boards that end at different sizes."""
    size = fx()["runs"][(level, max_size)][1]
    rng = np.random.default_rng(seed)
    by = [rng.permutation(np.nonzero(size == s)[0]) for s in sorted(set(int(v) for v in size))]
    return np.array([by[j % len(by)][(j // len(by)) % len(by[j % len(by)])] for j in range(n)])


def run_rows(level, max_size, pos):
    idx, size, count, first, cover = fx()["runs"][(level, max_size)]
    names = [fx()["names"][i] for i in idx[pos]]
    return names, fx()["boards"][idx[pos]], fx()["grids"][idx[pos]], (size[pos], count[pos], first[pos], cover[pos])


@pytest.mark.parametrize("level,max_size", RUNS)
def test_fixture(solver, level, max_size):
    """Every case of the run, with all outputs and with each optional output
    left out.  (1, 4): class_2 .. class_5, 635 376 subsets of four cells each,
    and the empty board, C(81, 4) ranks and no backdoor."""
    all_rows = np.arange(len(fx()["runs"][(level, max_size)][0]))
    names, boards, grids, want = run_rows(level, max_size, all_rows)
    assert_same(names, gpu(solver, boards, grids, level, max_size), want)
    for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = gpu(solver, boards, grids, level, max_size, *flags)
        for g, w, asked in zip(got, want, (True,) + flags):
            assert (g is None and not asked) or np.array_equal(g, w), flags


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(solver, n):
    """Level 1 at max_size 3: sizes 0..3, max_size + 1 and both negative codes
    in turn, in batches around the wave size and over several waves."""
    pos = mix(1, 3, n, seed=n)
    names, boards, grids, want = run_rows(1, 3, pos)
    if n >= 63:
        assert {int(s) for s in want[0]} == {BC.MISMATCH, BC.INVALID, 0, 1, 2, 3, 4}
    assert_same(names, gpu(solver, boards, grids, 1, 3), want)


def test_grid_size_does_not_matter(solver):
    """130 boards at level 1, max_size 3, on grids of one, two and seven waves
    and on the full grid: the fixture's answers, byte for byte the same."""
    pos = mix(1, 3, 130, seed=5)
    names, boards, grids, want = run_rows(1, 3, pos)
    for max_waves in (1, 2, 7, 0):
        assert_same(names, gpu(solver, boards, grids, 1, 3, max_waves=max_waves), want)


def _rated(solver, boards, level):
    r = solver.rate(torch.from_numpy(np.array(boards, dtype=np.uint8)), max_level=level).cpu().numpy()
    return (r >= 1) & (r <= level)


def test_recomputed_from_rate(solver):
    """Level 2 up to size 2 on 24 boards: size, count, first and cover from
    solver.rate on the board with every subset of at most two empty cells
    filled -- another kernel, no pruning."""
    idx, size, *_ = fx()["runs"][(2, 3)]
    pos = np.concatenate([np.nonzero(size == s)[0][:8] for s in (0, 1, 2, 3)])[:24]
    names, boards, grids, _ = run_rows(2, 3, pos)
    got = gpu(solver, boards, grids, 2, 2)
    want = ([], [], [], [])
    for b, g in zip(boards, grids):
        empty = [c for c in range(81) if b[c] == 0]
        ans = (3, 0, BC.NONE4, [0] * 81)
        for k in (0, 1, 2):
            sets = list(combinations(empty, k))
            trial = np.repeat(b[None, :], len(sets), axis=0)
            if k:
                cells = np.array(sets)
                trial[np.arange(len(sets))[:, None], cells] = g[cells]
            hit = np.nonzero(_rated(solver, trial, 2))[0]
            if len(hit):
                cover = np.zeros(81, dtype=np.uint8)
                if k:
                    cover[np.unique(np.array(sets)[hit])] = 1
                ans = (k, len(hit), list(sets[hit[0]]) + [255] * (4 - k), cover.tolist())
                break
        for w, a in zip(want, ans):
            w.append(a)
    want = (np.array(want[0]), np.array(want[1]), np.array(want[2], dtype=np.uint8), np.array(want[3], dtype=np.uint8))
    assert {int(s) for s in want[0]} == {0, 1, 2, 3}
    assert_same(names, got, want)


def test_first_is_a_minimal_backdoor_and_levels_nest(solver):
    """On every case of the runs at max_size 3: the reported first set, filled
    in, is rated 1..L, and with any one of its cells left out it is not; size
    0 exactly where rate says 1..L; and the size does not grow with the level."""
    sizes = {}
    for level in (1, 2, 3):
        all_rows = np.arange(len(fx()["runs"][(level, 3)][0]))
        names, boards, grids, _ = run_rows(level, 3, all_rows)
        s, c, f, v = gpu(solver, boards, grids, level, 3)
        sizes[level] = s
        ok = s >= 0
        assert np.array_equal(_rated(solver, np.where(boards > 9, 0, boards), level)[ok], (s == 0)[ok])
        full, less = [], []
        for k in np.nonzero((s >= 1) & (s <= 3))[0]:
            cells = f[k][:s[k]].astype(int)
            assert (f[k][s[k]:] == 255).all() and (np.diff(cells) > 0).all()
            b = boards[k].copy()
            b[cells] = grids[k][cells]
            full.append(b)
            for drop in cells:
                d = b.copy()
                d[drop] = boards[k][drop]
                less.append(d)
        assert len(full) >= 40 and _rated(solver, np.array(full), level).all()
        assert not _rated(solver, np.array(less), level).any()
    ok = sizes[1] >= 0
    assert (sizes[2][ok] <= sizes[1][ok]).all() and (sizes[3][ok] <= sizes[2][ok]).all()


def test_symmetry_images(solver):
    """Board and grid under one seeded symmetry (cells permuted, digits
    relabelled): the same size and count, and the cover is the image of the
    cover.  48 cases at level 2 and 16 at level 1, max_size 3."""
    rng = np.random.default_rng(2323)
    moved = 0
    for level, n in ((2, 48), (1, 16)):
        pos = mix(level, 3, n, seed=level)
        names, boards, grids, want = run_rows(level, 3, pos)
        valid = want[0] != BC.INVALID  # (a byte > 9 has no image)
        syms = [Y.random_symmetry(rng) for _ in range(n)]
        ib = np.array([Y.image_board(b, s) if ok else b for b, s, ok in zip(boards, syms, valid)], dtype=np.uint8)
        ig = np.array([Y.image_board(g, s) if ok else g for g, s, ok in zip(grids, syms, valid)], dtype=np.uint8)
        s, c, f, v = gpu(solver, ib, ig, level, 3)
        assert np.array_equal(s, want[0]) and np.array_equal(c, want[1])
        for k in np.nonzero(valid)[0]:
            assert np.array_equal(v[k], want[3][k][syms[k][0]]), names[k]
        moved += sum(not np.array_equal(f[k], want[2][k]) for k in range(n))
    assert moved >= 8  # first moves: it is not covariant


def test_solutions_none(solver):
    """Without solutions the completion comes from count_solutions: proper
    boards answer as with their grid given, a board with no completion is a
    MISMATCH, a board with two completions answers for one of them."""
    idx, size, count, first, cover = fx()["runs"][(2, 3)]
    names = [fx()["names"][i] for i in idx]
    proper = np.array([k for k, n in enumerate(names) if n.startswith(("class_", "seed_", "puzzles_30_", "proper_", "full_"))])
    assert len(proper) == 134
    _, boards, _, want = run_rows(2, 3, proper)
    dead = R.digits(R.NAMED["dead_at_level_2"][0])
    two = fx()["boards"][fx()["names"].index("undecided_trials_removed_a")]
    ten = fx()["boards"][fx()["names"].index("board_byte_10")]
    got = gpu(solver, np.concatenate([boards, dead[None], two[None], ten[None]]), None, 2, 3)
    assert_same([names[k] for k in proper], tuple(g[:len(proper)] for g in got), want)
    s, c, f, v = (g[len(proper):] for g in got)
    assert (int(s[0]), int(c[0]), f[0].tolist(), int(v[0].sum())) == (BC.MISMATCH, 0, BC.NONE4, 0)
    ab = [k for k, n in enumerate(names) if n.startswith("undecided_trials_removed_")]
    assert (int(s[1]), int(c[1]), f[1].tolist(), v[1].tolist()) in [
        (int(size[k]), int(count[k]), first[k].tolist(), cover[k].tolist()) for k in ab]
    assert (int(s[2]), int(c[2]), f[2].tolist(), int(v[2].sum())) == (BC.INVALID, 0, BC.NONE4, 0)
    with pytest.raises(ValueError):
        solver.backdoors(boards[:1], level=4)
    with pytest.raises(ValueError):
        solver.backdoors(boards[:1], level=0)
    with pytest.raises(ValueError):
        solver.backdoors(boards[:1], max_size=5)
    with pytest.raises(ValueError):
        solver.backdoors(boards[:1], max_size=0)


# ---------------------------------------------------------------- the raw ABI
class _Raw:
    """sdk_backdoor_batch at level 1, max_size 3 on the 130-board mix:
    arguments carved from guarded arenas, the byte arrays at addresses 1, 2 and
    3 mod 4, the scratch exactly as large as asked and 8- but not 16-byte
    aligned."""

    def __init__(self, solver, n=130):
        self.solver, self.L, self.n = solver, solver.lib, n
        pos = mix(1, 3, n, seed=9)
        self.names, self.boards, self.grids, self.want = run_rows(1, 3, pos)
        self.need = int(self.L.sdk_backdoor_scratch_bytes(n, 3, 0))
        assert self.need == 256 + 320 * n
        self.ain = Arena(solver.device, IN_FILL, 2 * 81 * n + (1 << 16))
        self.aout = Arena(solver.device, OUT_FILL, 2 * 94 * n + (1 << 16))
        self.asc = Arena(solver.device, OUT_FILL, self.need + (1 << 16))
        self.b, self.g = self.ain.boards(n, 1, name="boards"), self.ain.boards(n, 3, name="grids")
        self.real = [torch.from_numpy(a.copy()).to(solver.device) for a in (self.boards, self.grids)]
        self.outs, self.other = self.carve_outs(""), self.carve_outs(" (second)")
        self.asc.carve(8, name="pad")
        self.sc = self.asc.carve(self.need, align=8, name="scratch")
        assert self.sc.data_ptr() % 16 == 8

    def carve_outs(self, tag):
        n, a = self.n, self.aout
        return [a.carve(4 * n, itemsize=4, name="size" + tag), a.carve(4 * n, itemsize=4, name="count" + tag),
                a.carve(4 * n, offset_mod4=2, name="first" + tag), a.carve(81 * n, offset_mod4=3, name="cover" + tag)]

    def put_inputs(self):
        self.b.copy_(self.real[0])
        self.g.copy_(self.real[1])

    def call(self, outs, stream=None, **kw):
        a = dict(b=self.b.data_ptr(), g=self.g.data_ptr(), s=outs[0].data_ptr(), c=outs[1].data_ptr(),
                 f=outs[2].data_ptr(), v=outs[3].data_ptr(), n=self.n, level=1, size=3, sc=self.sc.data_ptr(),
                 nb=self.need, w=0)
        a.update(kw)
        with torch.cuda.device(self.solver.device):
            return self.L.sdk_backdoor_batch(a["b"], a["g"], a["s"], a["c"], a["f"], a["v"], a["n"], a["level"], a["size"],
                                             a["sc"], a["nb"], a["w"], _stream_handle(self.solver, stream))

    def check(self, got):
        n = self.n
        assert_same(self.names, (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy().reshape(n, 4),
                                 got[3].cpu().numpy().reshape(n, 81)), self.want)

    def finish(self):
        torch.cuda.synchronize()
        for a in (self.ain, self.aout, self.asc):
            a.assert_guards()
        assert np.array_equal(self.b.cpu().numpy(), self.boards) and np.array_equal(self.g.cpu().numpy(), self.grids)


def test_abi_odd_addresses_guards_and_reuse(solver):
    """Two calls back to back on one scratch into two sets of outputs: both
    right, no byte outside the extents written, the inputs as they were."""
    r = _Raw(solver)
    r.put_inputs()
    assert r.call(r.outs) == 0 and r.call(r.other) == 0
    torch.cuda.synchronize()
    r.check(r.outs)
    r.check(r.other)
    r.finish()


def test_abi_bad_arguments_write_nothing(solver):
    r = _Raw(solver)
    r.put_inputs()
    before = r.aout.buf.clone()
    for kw in (dict(level=0), dict(level=4), dict(size=0), dict(size=5), dict(n=-1), dict(w=-1), dict(nb=r.need - 1),
               dict(b=None), dict(g=None), dict(s=None), dict(sc=None), dict(s=r.outs[0].data_ptr() + 2),
               dict(c=r.outs[1].data_ptr() + 1), dict(sc=r.sc.data_ptr() + 4), dict(n=1 << 31)):
        assert r.call(r.outs, **kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.equal(r.aout.buf, before)
    assert (r.sc == OUT_FILL).all()
    r.finish()


def test_abi_poisoned_scratch(solver):
    """The scratch pre-filled with 0xFF: counters, list and records are the
    call's own to arm."""
    r = _Raw(solver)
    r.put_inputs()
    r.sc.fill_(0xFF)
    assert r.call(r.outs) == 0
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
    got = _on_side_stream(solver, "backdoor", [(r.b, r.real[0]), (r.g, r.real[1])], call, r.outs, scratch=(r.sc,),
                          dirty=dirty)
    r.check(got)
    r.finish()
