"""Batches whose byte extents pass 2^31 and 2^32 (test_gpu_large.py on the
GPU, test_large_cases.py checks this file itself on the CPU).  No test here.

Every board array of the C ABI is n * 81 bytes and every marks array n * 162
bytes, so the first batch sizes at which a byte offset needs bit 31 / bit 32
are (all exact, asserted below)

    row bytes   first n with n * row >= 2^31   ... >= 2^32
    81          R31 = 26 512 144               R32 = 53 024 288
    162         M31 = 13 256 072               M32 = 26 512 144
    64 * 2592   C31 = 12 946                   C32 = 25 891   (canon scratch)

Row R31 - 1 straddles byte 2^31 and row R32 - 1 byte 2^32.  N81 = R32 + 777 and
N162 = M32 + 777 are the batch sizes; both are odd, N81 * 81 is 1 mod 4 (the
batch's last dword is partial) and exceeds 0xFFFFFFF0, the largest
num_records the plane kernel's span loads put into a buffer descriptor.  Row
INDICES stay far below 2^31.

The harness never lets a torch op of its own see 2^31 elements: tensors are
written, read and compared in slices of at most CHUNK rows, and a slice of a
contiguous tensor is pointer arithmetic.  Two builders:

  Dense   every row is a pool board, row p -> pool index by a fixed
          arithmetic rule (groups taken in turn, a * q + b inside a group, a
          rarer set of groups every `every`-th row), so the expected answer of
          a chunk is a gather of per-board answers by the same rule.
  Sparse  the window rows (windows(): both ends of the batch and 192 rows
          either side of every threshold) are pool boards in a seeded order;
          every other row is a numbered filler -- byte 0 is 255, bytes 1..10
          the row index in decimal, the rest 0 -- which every entry answers at
          once (a byte > 9) and which is unique, so a read or write that lands
          on the wrong row shows.
"""
import contextlib
import gc
import math

import numpy as np
import pytest
import torch

T31, T32 = 2 ** 31, 2 ** 32
GIB = 1 << 30


def first_n(row_bytes, t):
    """The smallest n with n * row_bytes >= t."""
    return -(-t // row_bytes)


R31, R32 = 26_512_144, 53_024_288
M31, M32 = 13_256_072, 26_512_144
CANON_SLICES = 2592
C31, C32 = 12_946, 25_891
assert (R31, R32) == (first_n(81, T31), first_n(81, T32))
assert (M31, M32) == (first_n(162, T31), first_n(162, T32))
assert (C31, C32) == (first_n(64 * CANON_SLICES, T31), first_n(64 * CANON_SLICES, T32))
assert (R31 - 1) * 81 < T31 < R31 * 81 and (R32 - 1) * 81 < T32 < R32 * 81  # the rows before them straddle
N81, N162 = R32 + 777, M32 + 777
assert (N81, N162) == (53_025_065, 26_512_921) and N81 % 2 == 1 and N162 % 2 == 1
assert N81 * 81 % 4 == 1 and N81 * 81 > 0xFFFFFFF0 and N162 * 162 > T32 and N162 * 81 > T31
assert N81 < T31  # row indices are out of scope

CHUNK = 1 << 22  # rows per harness op: 2^22 * 162 elements < 2^31
SPAN = 192       # three waves on each side of a boundary
MAX_PEAK = 16 * GIB


# ------------------------------------------------------------------ windows
def thresholds(n, row_bytes):
    """The threshold rows (first_n) of arrays of these row sizes that a batch
    of n rows reaches, ascending."""
    sizes = (row_bytes,) if isinstance(row_bytes, int) else tuple(row_bytes)
    return sorted({first_n(b, t) for b in sizes for t in (T31, T32) if first_n(b, t) <= n})


def windows(n, row_bytes):
    """The rows that must be real boards: the first and last SPAN rows and the
    SPAN rows before and after every threshold row (row_bytes: one row size or
    several, one per array the call touches).  Sorted, unique, int64."""
    runs = [(0, SPAN), (n - SPAN, n)] + [(t - SPAN, t + SPAN) for t in thresholds(n, row_bytes)]
    return np.unique(np.concatenate([np.arange(max(lo, 0), min(hi, n), dtype=np.int64) for lo, hi in runs]))


def runs_of(rows):
    """[(lo, hi)] of the contiguous runs of a sorted row list."""
    rows = np.asarray(rows, dtype=np.int64)
    if not len(rows):
        return []
    cut = np.flatnonzero(np.diff(rows) != 1) + 1
    return [(int(r[0]), int(r[-1]) + 1) for r in np.split(rows, cut)]


def chunks(n):
    return [(lo, min(n, lo + CHUNK)) for lo in range(0, n, CHUNK)]


def _fdiv(x, d):
    return torch.div(x, d, rounding_mode="floor") if isinstance(x, torch.Tensor) else x // d


# ------------------------------------------------------------------ fillers
def filler_boards(lo, hi, device, per=1):
    """Rows lo..hi-1 as numbered fillers, (hi - lo, 81) uint8; with per > 1,
    row q carries q / per (the filler board an item of the sampler came from)."""
    rows = _fdiv(torch.arange(lo, hi, dtype=torch.int64, device=device), per)
    out = torch.zeros((hi - lo, 81), dtype=torch.uint8, device=device)
    out[:, 0] = 255
    for k in range(10):
        out[:, 1 + k] = (_fdiv(rows, 10 ** (9 - k)) % 10).to(torch.uint8)
    return out


def filler_row(board):
    """The row index a filler carries, or None if `board` is no filler."""
    b = np.asarray(board)
    if b[0] != 255 or (b[1:11] > 9).any() or b[11:].any():
        return None
    return int("".join(str(int(d)) for d in b[1:11]))


def constant(value, width, dtype):
    """A filler of one value: (rows, width), or (rows,) for width 0."""
    def fill(lo, hi, device):
        return torch.full((hi - lo, width) if width else (hi - lo,), value, dtype=dtype, device=device)
    return fill


# ----------------------------------------------------------------- builders
class Dense:
    """Row p -> pool index.  groups / rare: lists of pool-index arrays.  Row p
    with p % every == 0 (when there are rare groups) is rare row j = p / every:
    group j % len(rare), member (a * (j / len(rare)) + b) % its length; every
    other row is group p % len(groups), member (a * (p / len(groups)) + b) %
    its length.  a is coprime to every length, so each group's members all
    come up, in an order that is not the pool's."""
    A = 1_000_003

    def __init__(self, groups, rare=(), every=61, b=12_345):
        self.main = [np.asarray(g, dtype=np.int64) for g in groups]
        self.rare = [np.asarray(g, dtype=np.int64) for g in rare]
        self.every, self.b = int(every), int(b)
        assert self.main and all(len(g) for g in self.main + self.rare)
        # (the rows the rare groups take are no fixed members of a main group)
        assert not self.rare or all(math.gcd(self.every, len(g)) == 1 for g in self.main)
        for g in self.main + self.rare:
            assert math.gcd(self.A, len(g)) == 1
            # a wrapped byte offset is no multiple of a period of the rule: it never lands on an identical row
            for k in (len(g), len(g) * self.every * max(1, len(self.rare)) * len(self.main)):
                assert T31 % (81 * k) and T32 % (81 * k)
        self._np = {"main": self._tables(self.main), "rare": self._tables(self.rare) if self.rare else None}
        self._dev = {}
        self._counts = {}

    @staticmethod
    def _tables(groups):
        lens = np.array([len(g) for g in groups], dtype=np.int64)
        return np.concatenate(groups), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens

    def _on(self, device):
        if device not in self._dev:
            self._dev[device] = {k: None if v is None else tuple(torch.from_numpy(x).to(device) for x in v)
                                 for k, v in self._np.items()}
        return self._dev[device]

    def _pick(self, tables, r):
        tab, starts, lens = tables
        g = r % len(lens)
        return tab[starts[g] + (self.A * _fdiv(r, len(lens)) + self.b) % lens[g]]

    def index(self, p):
        """Pool indices of rows p (a numpy int64 array or a torch int64 tensor)."""
        t = self._on(p.device) if isinstance(p, torch.Tensor) else self._np
        idx = self._pick(t["main"], p)
        if t["rare"] is None:
            return idx
        where = torch.where if isinstance(p, torch.Tensor) else np.where
        return where(p % self.every == 0, self._pick(t["rare"], _fdiv(p, self.every)), idx)

    def gather(self, table, lo, hi):
        """Rows lo..hi-1 of the batch whose row p is table[index(p)] (a device tensor)."""
        return table.index_select(0, self.index(torch.arange(lo, hi, dtype=torch.int64, device=table.device)))

    def counts(self, n, size):
        """How often each of `size` pool boards occurs in rows 0..n-1 (numpy alone)."""
        if (n, size) not in self._counts:
            c = np.zeros(size, dtype=np.int64)
            for lo, hi in chunks(n):
                c += np.bincount(self.index(np.arange(lo, hi, dtype=np.int64)), minlength=size)
            self._counts[n, size] = c
        return self._counts[n, size]

    def real_rows(self, n, row_bytes):
        return windows(n, row_bytes)

    def histogram(self, n, values):
        """value -> rows of the batch whose board has that per-board value."""
        values = np.asarray(values)
        c = self.counts(n, len(values))
        return {int(v): int(c[values == v].sum()) for v in np.unique(values[c > 0])}


class Sparse:
    """Window rows are pool boards in a seeded order (every board of the pool
    once before any comes twice); every other row is a filler."""

    def __init__(self, n, row_bytes, pool_size, seed=0, rows=None, picks=None):
        """rows: the real rows where they are not windows(n, row_bytes); picks:
        their pool indices where they are not the seeded order."""
        self.n = int(n)
        self.rows = windows(n, row_bytes) if rows is None else np.asarray(rows, dtype=np.int64)
        assert (np.diff(self.rows) > 0).all() and self.rows[0] >= 0 and self.rows[-1] < n
        rng = np.random.default_rng(seed)
        reps = -(-len(self.rows) // pool_size)
        self.picks = np.concatenate([rng.permutation(pool_size) for _ in range(reps)])[:len(self.rows)].astype(np.int64) \
            if picks is None else np.asarray(picks, dtype=np.int64)
        assert len(self.picks) == len(self.rows)

    def index(self, p):
        """Pool indices of window rows p (numpy)."""
        at = np.searchsorted(self.rows, p)
        assert np.array_equal(self.rows[at], p)
        return self.picks[at]

    def gather(self, table, lo, hi, filler):
        """Rows lo..hi-1: filler(lo, hi, device), the window rows among them from `table`."""
        out = filler(lo, hi, table.device)
        a, b = np.searchsorted(self.rows, [lo, hi])
        if b > a:
            out[torch.from_numpy(self.rows[a:b] - lo).to(table.device)] = \
                table[torch.from_numpy(self.picks[a:b]).to(table.device)]
        return out

    def real_rows(self, n, row_bytes):
        return self.rows

    def histogram(self, n, values, filler_value):
        values = np.asarray(values)[self.picks]
        h = {int(v): int((values == v).sum()) for v in np.unique(values)}
        h[int(filler_value)] = h.get(int(filler_value), 0) + self.n - len(self.rows)
        return h


class Windowed(Sparse):
    """Every row real: the window rows are boards of the whole pool in a
    seeded order, every other row follows a Dense rule over a part of it (the
    boards that are cheap)."""

    def __init__(self, n, row_bytes, pool_size, dense, seed=0):
        super().__init__(n, row_bytes, pool_size, seed)
        self.dense = dense

    def index(self, p):
        idx = self.dense.index(p)
        at = np.minimum(np.searchsorted(self.rows, p), len(self.rows) - 1)
        hit = self.rows[at] == p
        idx[hit] = self.picks[at[hit]]
        return idx

    def gather(self, table, lo, hi):
        return super().gather(table, lo, hi, lambda a, b, device: self.dense.gather(table, a, b))

    def real_rows(self, n, row_bytes):
        """The windows and 64 rows of the rule either side of each."""
        near = [np.arange(max(lo - 64, 0), min(hi + 64, self.n)) for lo, hi in runs_of(self.rows)]
        return np.unique(np.concatenate(near))

    def histogram(self, n, values):
        values = np.asarray(values)
        c = self.dense.counts(self.n, len(values)).copy()
        np.subtract.at(c, self.dense.index(self.rows), 1)
        np.add.at(c, self.picks, 1)
        return {int(v): int(c[values == v].sum()) for v in np.unique(values[c > 0])}


def build(n, chunk_fn, device):
    """A device tensor of n rows, chunk by chunk: chunk_fn(lo, hi) -> rows lo..hi-1."""
    out = None
    for lo, hi in chunks(n):
        part = chunk_fn(lo, hi)
        if out is None:
            out = torch.empty((n,) + tuple(part.shape[1:]), dtype=part.dtype, device=device)
        out[lo:hi] = part
    return out


def filled(n, width, dtype, value, device):
    """(n, width) (or (n,) for width 0) of one value; a byte pattern for uint8 / int values."""
    out = torch.empty((n, width) if width else (n,), dtype=dtype, device=device)
    for lo, hi in chunks(n):
        out[lo:hi].fill_(value)
    return out


# ------------------------------------------------------------------ compare
def compare(got, want_fn, n, what, accept=None):
    """got[lo:hi] == want_fn(lo, hi) for every chunk, on the device.  accept
    (rows of got, their row indices) -> bool per row: rows that differ from
    want but are right all the same.  The first mismatch is reported with its
    byte offset against both thresholds."""
    assert got.shape[0] == n
    row_bytes = got[0:1].numel() * got.element_size()
    for lo, hi in chunks(n):
        g, w = got[lo:hi], want_fn(lo, hi)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
        bad = g != w
        if bad.dim() > 1:
            bad = bad.flatten(1).any(dim=1)
        if accept is not None and bool(bad.any()):
            for at in torch.nonzero(bad)[:, 0].split(1 << 19):
                bad[at] = ~accept(g[at], at + lo)
        if bool(bad.any()):
            k = int(torch.nonzero(bad)[0, 0])
            off = (lo + k) * row_bytes
            raise AssertionError(
                f"{what}: row {lo + k} differs, {int(bad.sum())} rows of chunk [{lo}, {hi}); byte offset {off} = "
                f"2^31 {off - T31:+d} = 2^32 {off - T32:+d}\n got  {g[k].flatten().tolist()}\n want {w[k].flatten().tolist()}")


def histogram(values, n, lowest=-8):
    """value -> count of an int32 device array, chunk by chunk."""
    assert values.shape == (n,)
    total = np.zeros(256, dtype=np.int64)
    for lo, hi in chunks(n):
        v = values[lo:hi].to(torch.int64) - lowest
        assert int(v.min()) >= 0 and int(v.max()) < len(total), f"a value outside [{lowest}, {lowest + len(total)})"
        total += torch.bincount(v, minlength=len(total)).cpu().numpy()
    return {int(k) + lowest: int(c) for k, c in enumerate(total) if c}


def self_check(batch, builder, pool, n, row_bytes, fillers=False):
    """The batch is what the test thinks it is: its window rows, copied to
    the host run by run, equal numpy's own gather from the pool; with
    `fillers`, the eight rows on either side of every run that are no window
    rows are fillers whose digits say their row."""
    rows = builder.real_rows(n, row_bytes)
    want = np.asarray(pool)[builder.index(rows)]
    at = 0
    for lo, hi in runs_of(rows):
        host = batch[lo:hi].cpu().numpy()
        assert np.array_equal(host, want[at:at + hi - lo]), f"rows [{lo}, {hi}) of the input are not the pool's"
        at += hi - lo
        if fillers:
            for a, b in ((max(lo - 8, 0), lo), (hi, min(hi + 8, n))):
                for k, board in enumerate(batch[a:b].cpu().numpy()):
                    if a + k not in rows:
                        assert filler_row(board) == a + k, f"row {a + k} is no filler of its own number"


def valid_rows(g):
    """(m,) bool on the device: row k of the (m, 81) uint8 tensor is a grid
    whose rows, columns and boxes each hold 1..9 once (enum_cases.valid_grids
    restated: nine powers of two out of 2..512 sum to 1022 only if they are
    all different)."""
    v = g.to(torch.int16)  # nine times 512 fits
    bits = (torch.bitwise_left_shift(torch.ones_like(v), v.clamp(max=9)) * ((v >= 1) & (v <= 9))).view(-1, 9, 9)
    boxes = bits.view(-1, 3, 3, 3, 3).sum(dim=(2, 4)).view(-1, 9)
    return ((bits.sum(dim=2) == 0x3FE).all(dim=1) & (bits.sum(dim=1) == 0x3FE).all(dim=1) & (boxes == 0x3FE).all(dim=1))


# ------------------------------------------------------------------- memory
def need_memory(peak_bytes):
    """Skip when the device has less free memory than the test's stated peak plus 2 GiB."""
    assert peak_bytes <= MAX_PEAK
    free, total = torch.cuda.mem_get_info()
    if free < peak_bytes + 2 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB of {total / GIB:.1f} free, {peak_bytes / GIB:.1f} + 2 needed")


@contextlib.contextmanager
def budget(peak_bytes):
    """The body allocates at most peak_bytes (never more than 16 GiB) on top
    of what the process holds already -- the session solver's workspace and
    cached scratches -- and leaves nothing cached."""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    need_memory(peak_bytes)
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        yield
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"peak {peak / GIB:.2f} GiB ({(peak - held) / GIB:.2f} this test's, {peak_bytes / GIB:.2f} stated)")
        assert peak - held <= peak_bytes <= MAX_PEAK, (peak, held, peak_bytes)
    finally:
        gc.collect()
        torch.cuda.empty_cache()
