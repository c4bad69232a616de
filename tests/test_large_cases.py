"""large_cases.py checked on the CPU at small sizes: the builders' torch and
numpy index rules agree, the compare names the row it should, and the grid
check restates enum_cases.valid_grids.  (The thresholds are asserted when the
module is imported.)"""
import numpy as np
import pytest
import torch

import large_cases as L


def test_windows_cover_both_ends_and_every_threshold():
    rows = L.windows(L.N81, 81)
    assert L.runs_of(rows) == [(0, 192), (L.R31 - 192, L.R31 + 192), (L.R32 - 192, L.R32 + 192), (L.N81 - 192, L.N81)]
    assert L.R31 - 1 in rows and L.R32 - 1 in rows  # the rows that straddle 2^31 and 2^32
    both = L.windows(L.N162, (81, 162))
    assert L.thresholds(L.N162, (81, 162)) == [L.M31, L.M32] and L.M32 == L.R31
    assert L.runs_of(both) == [(0, 192), (L.M31 - 192, L.M31 + 192), (L.M32 - 192, L.M32 + 192), (L.N162 - 192, L.N162)]
    assert L.thresholds(1000, 81) == [] and L.runs_of(L.windows(1000, 81)) == [(0, 192), (808, 1000)]
    assert L.runs_of(L.windows(100, 81)) == [(0, 100)]


def test_dense_rule_is_the_same_in_numpy_and_torch():
    D = L.Dense([np.arange(0, 7), np.arange(7, 12)], rare=[np.arange(12, 15), np.arange(15, 17)], every=3)
    with pytest.raises(AssertionError):
        L.Dense([np.arange(0, 7), np.arange(7, 12)], rare=[np.arange(12, 15)], every=5)
    p = np.concatenate([np.arange(0, 4000), np.arange(L.R32 - 50, L.R32 + 50)]).astype(np.int64)
    idx = D.index(p)
    assert np.array_equal(idx, D.index(torch.from_numpy(p)).numpy())
    rare = p % 3 == 0
    assert idx[rare].min() >= 12 and idx[~rare].max() < 12 and set(idx) == set(range(17))
    turn = D.index(np.array([0, 3, 6, 9]))  # the rare groups in turn
    assert (turn[[0, 2]] < 15).all() and (turn[[1, 3]] >= 15).all()
    table = torch.arange(17 * 3, dtype=torch.int32).view(17, 3)
    assert torch.equal(D.gather(table, 100, 164), table[torch.from_numpy(D.index(np.arange(100, 164)))])
    n = 12_345
    counts = D.counts(n, 17)
    assert counts.sum() == n and np.array_equal(counts, np.bincount(D.index(np.arange(n)), minlength=17))
    assert D.histogram(n, np.arange(17) // 12) == {0: int(counts[:12].sum()), 1: int(counts[12:].sum())}
    built = L.build(n, lambda lo, hi: D.gather(table, lo, hi), "cpu")
    assert torch.equal(built, table[torch.from_numpy(D.index(np.arange(n)))])


def test_sparse_batch_is_pool_rows_in_the_windows_and_numbered_fillers():
    n, pool = 1000, torch.arange(40 * 81, dtype=torch.int64).remainder(10).to(torch.uint8).view(40, 81)
    S = L.Sparse(n, 81, 40, seed=3)
    assert len(S.rows) == 384 and set(S.picks) == set(range(40))
    b = L.build(n, lambda lo, hi: S.gather(pool, lo, hi, L.filler_boards), "cpu")
    L.self_check(b, S, pool.numpy(), n, 81, fillers=True)
    host = b.numpy()
    for row in (192, 500, 807):
        assert L.filler_row(host[row]) == row and host[row].max() > 9
    assert L.filler_row(host[0]) is None
    big = L.filler_boards(L.R32 - 2, L.R32 + 2, "cpu").numpy()
    assert [L.filler_row(r) for r in big] == list(range(L.R32 - 2, L.R32 + 2))
    st = L.build(n, lambda lo, hi: S.gather(torch.ones(40, dtype=torch.int32), lo, hi, L.constant(-1, 0, torch.int32)), "cpu")
    assert L.histogram(st, n) == S.histogram(n, np.ones(40, dtype=np.int32), -1) == {1: 384, -1: 616}
    b[193, 3] = 7  # a filler beside a window that says another row
    with pytest.raises(AssertionError):
        L.self_check(b, S, pool.numpy(), n, 81, fillers=True)


def test_compare_reports_the_row_and_its_offsets():
    n = 300
    got = L.filled(n, 81, torch.uint8, 0xEE, "cpu")
    L.compare(got, lambda lo, hi: torch.full((hi - lo, 81), 0xEE, dtype=torch.uint8), n, "fill")
    got[257, 80] = 1
    with pytest.raises(AssertionError) as e:
        L.compare(got, lambda lo, hi: torch.full((hi - lo, 81), 0xEE, dtype=torch.uint8), n, "fill")
    text = str(e.value)
    assert "row 257 differs" in text and f"byte offset {257 * 81} = 2^31 {257 * 81 - 2 ** 31:+d}" in text
    L.compare(got, lambda lo, hi: torch.full((hi - lo, 81), 0xEE, dtype=torch.uint8), n, "fill",
              accept=lambda rows, at: at == 257)
    marks = L.filled(n, 81, torch.int16, -4370, "cpu")
    marks[5, 0] = 0
    with pytest.raises(AssertionError, match=f"byte offset {5 * 162} "):
        L.compare(marks, lambda lo, hi: torch.full((hi - lo, 81), -4370, dtype=torch.int16), n, "marks")


def test_valid_rows_restates_the_numpy_check():
    import enum_cases as E
    from abi_arena import FULL
    full = np.array([int(c) for c in FULL], dtype=np.uint8)
    rng = np.random.default_rng(5)
    rows = np.tile(full, (200, 1))
    for k in range(1, 200):
        cells = rng.choice(81, int(rng.integers(1, 4)), replace=False)
        rows[k, cells] = rng.integers(0, 16, len(cells))
    rows[199] = 5  # every unit sums to 45
    want = E.valid_grids(rows)
    assert want[0] and not want[199] and 0 < want.sum() < 200
    assert np.array_equal(L.valid_rows(torch.from_numpy(rows)).numpy(), want)
