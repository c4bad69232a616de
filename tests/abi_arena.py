"""Caller memory for the C ABI's buffer contracts (test_abi_pool.py on the
CPU, test_gpu_abi_buffers.py and test_gpu_abi_streams.py on the GPU): guarded
arenas to carve the arguments from, one pool of boards whose answers come
from the oracle alone, built once per process and never modified, and the
harness of the poisoned-scratch and stream-order checks (_poisons,
_on_side_stream).

Arena: one uint8 buffer filled with one byte.  carve() hands out views at a
chosen address mod 4 (byte arrays) or at their natural alignment (int32 /
int64 arrays), each with at least GUARD untouched bytes before and after it;
assert_guards() names the first changed byte outside every carved region.
Output arenas are filled with 0xA5; input arenas with 0xFF, a byte > 9, so a
kernel that lets bytes outside [ptr, ptr + 81 n) into its answer reports
SDK_INVALID or a different grid.

Pool (kinds, in this order; want[order] = (rows, status) per board):
  hard17   256 hard17_batch boards: one completion (O.solve_unique_batch),
           the answer of both walks
  gen      256 boards made as generate_batch makes them (gen.py:31-52 with
           the oracle's walk as the fill), 30..55 empties: O.solve_batch(order)
  dead     clean givens, no completion, status 0, row = input: 16 full grids
           with one wrong clue and 12 blanks (O.solve_batch(order) itself),
           32 boards of test_gpu_frontier._slow_dead, which search, and
           frontier_cases.DEAD (the oracle's complete counter finds none, so
           the walk finds none either: the literal walk would not come back
           from them)
  clash    CLASH of test_gpu_batches.py and 63 full grids with one cell
           repeated in its row or column and 3..8 blanks: the literal walk
           (O.solve_batch, "node_literal" in node order: include/sudoku_hip.h
           promises node.py's short-circuit, which only such boards reach);
           some it "solves", some it does not
  invalid  a byte of 10 or 255: status -1, row = input
  single   the empty board and a full grid
"""
import functools
import time

import numpy as np
import torch

from oracle import oracle as O

GUARD = 256  # bytes before and after every carved region: a cache line and the widest store
OUT_FILL = 0xA5
IN_FILL = 0xFF
KINDS = ("hard17", "gen", "dead", "clash", "invalid", "single")
ORDERS = {"gen": 0, "node": 1}
FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"
CLASH = "88" + FULL[2:30] + "0" + FULL[31:50] + "0" + FULL[51:70] + "0" + FULL[71:]
SEED = 8128


class Arena:
    """`nbytes` of uint8 on `device`, every byte `fill`."""

    def __init__(self, device, fill, nbytes=1 << 22):
        self.fill = int(fill)
        self.buf = torch.full((int(nbytes),), self.fill, dtype=torch.uint8, device=device)
        self.regions = []  # (start, end, name), ascending
        self._cursor = 0

    def carve(self, nbytes, offset_mod4=0, itemsize=1, name=None, align=None):
        """A view of `nbytes` bytes: address = offset_mod4 (mod 4) for a byte
        array, a multiple of `itemsize` for an int32 / int64 array (returned
        as that dtype), a multiple of `align` where one is given (scratch)."""
        nbytes = int(nbytes)
        assert itemsize in (1, 4, 8) and nbytes % itemsize == 0 and 0 <= offset_mod4 < 4
        mod = align if align else (4 if itemsize == 1 else itemsize)
        rem = 0 if align or itemsize != 1 else offset_mod4
        start = self._cursor + GUARD
        start += (rem - (self.buf.data_ptr() + start)) % mod
        end = start + nbytes
        if end + GUARD > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is full ({end + GUARD} needed)")
        self._cursor = end
        self.regions.append((start, end, name or f"region{len(self.regions)}"))
        view = self.buf[start:end]
        assert (view.data_ptr() - rem) % mod == 0
        return view if itemsize == 1 else view.view(torch.int32 if itemsize == 4 else torch.int64)

    def boards(self, n, offset_mod4=0, name=None):
        """carve() for n boards, as an (n, 81) view."""
        return self.carve(81 * n, offset_mod4, name=name).view(n, 81)

    def first_damage(self):
        """None, or (offset, value, region name, side, distance) of the first
        changed byte outside all carved regions; distance 1 is the byte next
        to the region."""
        edges = [0] + [x for s, e, _ in self.regions for x in (s, e)] + [self.buf.numel()]
        for k in range(0, len(edges), 2):
            lo, hi = edges[k], edges[k + 1]
            bad = self.buf[lo:hi] != self.fill
            if not bool(bad.any()):
                continue
            at = lo + int(torch.nonzero(bad)[0, 0])
            before = [(at - e + 1, name, "after") for s, e, name in self.regions if e <= at]
            after = [(s - at, name, "before") for s, e, name in self.regions if s > at]
            dist, name, side = min(before[-1:] + after[:1])
            return at, int(self.buf[at]), name, side, dist
        return None

    def assert_guards(self):
        hit = self.first_damage()
        assert hit is None, ("byte %d of the arena is 0x%02x, not the fill: %d byte(s) %s region %s"
                             % (hit[0], hit[1], hit[4], hit[3], hit[2]))


# ------------------------------------------------------------------ the pool
def _b81(s):
    return np.array([int(c) for c in s], dtype=np.uint8)


def _generated(n, seed):
    """generate_batch(1, e, .) board by board for e = 30..55 in turn, with
    the oracle's gen.py walk as the fill (gen.generate_batch runs that fill
    on the GPU)."""
    import random
    from sudoku_solver_distributed_amd.gen import _draw_diagonal, _draw_removals
    rng = random.Random(seed)
    diag = np.array([_draw_diagonal(rng) for _ in range(n)], dtype=np.uint8).reshape(n, 81)
    full, st = O.solve_batch(diag)
    assert (st == 1).all()
    out = full.copy()
    for k in range(n):
        out[k, _draw_removals(rng, 30 + k % 26, [True] * 81)] = 0
    return out


def _shallow_dead(grids, rng):
    """Full grids with 12 cells blanked and one of the blanks filled again
    with a digit the grid does not hold there and sudoku.py's is_valid
    accepts (the givens stay clean), kept when no completion is left."""
    out = []
    for g in grids:
        while True:
            h = g.copy()
            blanks = rng.choice(81, 12, replace=False)
            h[blanks] = 0
            cell = int(rng.choice(blanks))
            ok = [v for v in range(1, 10) if v != g[cell] and O.is_valid(h, cell // 9, cell % 9, v)]
            if not ok:
                continue
            h[cell] = ok[0]
            if O.count_solutions(h, 1) == 0:
                out.append(h)
                break
    return np.array(out, dtype=np.uint8)


def _clashing(grids, rng):
    """CLASH and one board per grid: a cell overwritten with its right (even
    grids) or lower (odd grids) neighbour's digit, then 3..8 other cells
    blanked."""
    out = [_b81(CLASH)]
    for k, g in enumerate(grids):
        h = g.copy()
        cell = int(rng.integers(0, 72))
        r, c = divmod(cell, 9)
        other = cell + 9 if k % 2 or c == 8 else cell + 1
        h[cell] = h[other]
        free = np.setdiff1d(np.arange(81), [cell, other])
        h[rng.choice(free, int(rng.integers(3, 9)), replace=False)] = 0
        out.append(h)
    return np.array(out, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pool():
    """{"boards": (k, 81), "kind": (k,) index into KINDS, "want": {order:
    (rows (k, 81), status (k,) int32)}, "seconds": the oracle's time for all
    answers of both orders}; every array read-only."""
    import count_cases as C
    import frontier_cases as F
    from test_gpu_frontier import _slow_dead
    from sudoku_solver_distributed_amd.gen import hard17_batch
    rng = np.random.default_rng(SEED)
    hard = hard17_batch(256, seed=SEED).numpy().copy()
    gen = _generated(256, SEED)
    grids, cnt = O.solve_unique_batch(hard17_batch(96, seed=SEED + 1).numpy())
    assert (cnt == 1).all()
    dead = np.concatenate([_shallow_dead(grids[:16], rng), _slow_dead(64)[:32], F.b81(F.DEAD)[None]])
    clash = _clashing(grids[16:79], rng)
    assert len(clash) == 64 and all(C.givens_clash(g) for g in clash)
    assert not any(C.givens_clash(g) for g in dead)
    invalid = np.stack([hard[0], hard[1], gen[0], gen[1], _b81(FULL), clash[1], np.zeros(81, np.uint8), hard[2]])
    for g, (cell, v) in zip(invalid, ((0, 10), (80, 255), (40, 255), (79, 10), (1, 10), (3, 255), (80, 10), (0, 255))):
        g[cell] = v
    single = np.stack([np.zeros(81, np.uint8), _b81(FULL)])
    parts = (hard, gen, dead, clash, invalid, single)
    boards = np.ascontiguousarray(np.concatenate(parts))
    kind = np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)])
    lo = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    sl = {name: slice(lo[i], lo[i + 1]) for i, name in enumerate(KINDS)}
    t0 = time.perf_counter()
    want = {}
    uniq, cnt = O.solve_unique_batch(hard)
    assert (cnt == 1).all()
    gone = O.solve_unique_batch(dead[16:])[1]
    assert (gone == 0).all()
    for order in ("gen", "node"):
        rows, st = boards.copy(), np.zeros(len(boards), dtype=np.int32)
        rows[sl["hard17"]], st[sl["hard17"]] = uniq, 1
        rows[sl["gen"]], st[sl["gen"]] = O.solve_batch(gen, order=order)
        a, b = O.solve_batch(dead[:16], order=order)
        assert (b == 0).all() and np.array_equal(a, dead[:16])
        rows[sl["clash"]], st[sl["clash"]] = O.solve_batch(clash, order="node_literal" if order == "node" else "gen")
        st[sl["invalid"]] = -1
        rows[sl["single"]], st[sl["single"]] = O.solve_batch(single, order=order)
        want[order] = (rows, st)
    seconds = time.perf_counter() - t0
    for v in (boards, kind, *want["gen"], *want["node"]):
        v.setflags(write=False)
    return {"boards": boards, "kind": kind, "want": want, "seconds": seconds}


def kind_indices(name):
    return np.nonzero(pool()["kind"] == KINDS.index(name))[0]


def mixed(n, seed=0, kinds=KINDS):
    """Pool indices of an n-board batch that interleaves `kinds`: every
    board of them at least once where n allows, in one seeded permutation, so
    solved boards neighbour unsolvable, deferred and invalid ones."""
    src = np.concatenate([kind_indices(k) for k in kinds])
    rng = np.random.default_rng(seed + n)
    idx = np.concatenate([rng.permutation(src), rng.choice(src, size=max(0, n - len(src)))])[:n]
    rng.shuffle(idx)
    return idx


# ------------------------------- poisoned scratch and stream order (the GPU)
def _stream_handle(solver, stream=None):
    s = stream if stream is not None else torch.cuda.current_stream(solver.device)
    return int(s.cuda_stream)


def _poisons(view):
    """The two pre-fills of a scratch: 0xFF, then seeded random bytes."""
    yield "0xFF", lambda: view.fill_(0xFF)
    g = torch.Generator(device="cpu").manual_seed(view.numel())
    yield "random", lambda: view.copy_(torch.randint(0, 256, (view.numel(),), dtype=torch.uint8, generator=g))


@functools.lru_cache(maxsize=None)
def _delay_rate(device):
    """Units of device delay per millisecond: cycles of torch.cuda._sleep
    where there is one, else fills of a 256 MB tensor (measured with events
    on the device, after a warm-up)."""
    big = None if hasattr(torch.cuda, "_sleep") else torch.empty(1 << 28, dtype=torch.uint8, device=device)

    def run(units):
        if big is None:
            torch.cuda._sleep(int(units))
        else:
            for _ in range(int(units)):
                big.fill_(1)
    probe = 20_000_000 if big is None else 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        torch.cuda.synchronize()
        e0.record()
        run(probe)
        e1.record()
        torch.cuda.synchronize()
    return run, probe / e0.elapsed_time(e1)


def _on_side_stream(solver, what, inputs, call, outputs, scratch=(), dirty=None, blocking=False):
    """The library call on a side stream behind a delay and an input copy
    queued on that stream only; the default stream stays idle.  inputs:
    (argument view, device tensor with the real contents) pairs -- the views
    hold 0xFF until the copy on the side stream runs; outputs: views, copied
    on the side stream after the call; scratch: views the call fills for its
    own later kernels, 0xFF before it; dirty: a call queued on the side
    stream before the input copy that leaves the queue head used (the same
    entry on the 0xFF inputs, into other outputs).  Returns the copies.  A
    launch or memset on any other stream runs at once: it reads 0xFF, or its
    result is overwritten (a queue head re-armed early is used again by
    `dirty`), or never reaches the copy.

    blocking: the entry is SYNCHRONOUS on its stream, so the host is back
    from it only when the delay is long over.  `early` is then sampled after
    the copies and fills are queued, immediately before the call; there is no
    `dirty` call, and in its place the side stream carries, between the delay
    and the call, the input copy, a refill of every output with OUT_FILL and
    a refill of every scratch view with 0xFF: what an init kernel or a memset
    wrote early on another stream is overwritten before the call's own
    kernels start.  The outputs are read by the copies on the side stream
    alone."""
    assert not (blocking and dirty is not None)
    run, rate = _delay_rate(solver.device)
    side = torch.cuda.Stream(solver.device)
    keep = [(v, v.clone()) for v in outputs]

    def prepare():
        if dirty is not None:
            dirty(side)
        for view, real in inputs:
            view.copy_(real, non_blocking=True)
        if blocking:
            for v in outputs:
                v.view(torch.uint8).fill_(OUT_FILL)
            for v in scratch:
                v.view(torch.uint8).fill_(IN_FILL)

    # dry runs: every kernel loaded, then the host's time to enqueue what
    # follows the delay, up to the call (the larger of two measurements); a
    # blocking call's own time is no enqueue time, so it is left out and the
    # call runs in the first dry run only
    torch.cuda.synchronize()
    enq_ms = 0.0
    with torch.cuda.stream(side):
        for k in range(3):
            t0 = time.perf_counter()
            prepare()
            t1 = time.perf_counter()
            if not (blocking and k):
                call(side)
            if k:
                enq_ms = max(enq_ms, ((t1 if blocking else time.perf_counter()) - t0) * 1e3)
            side.synchronize()
    for view in [v for v, _ in inputs] + list(scratch):
        view.view(torch.uint8).fill_(IN_FILL)
    for v, was in keep:
        v.copy_(was)
    torch.cuda.synchronize()
    delay_ms = 10.0 * enq_ms
    after_delay = torch.cuda.Event()
    with torch.cuda.stream(side):
        run(max(1, delay_ms * rate))
        after_delay.record(side)
        prepare()
        if blocking:
            early = not after_delay.query()
        call(side)
        if not blocking:
            early = not after_delay.query()
        got = [v.clone() for v in outputs]
    side.synchronize()
    print(f"{what}: enqueue {enq_ms:.3f} ms, delay {delay_ms:.3f} ms")
    assert early, f"{what}: the delay of {delay_ms:.3f} ms was over before the call was enqueued ({enq_ms:.3f} ms)"
    return got
