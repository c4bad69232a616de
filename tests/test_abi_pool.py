"""The helpers of the C ABI buffer tests, on the CPU: abi_arena's board pool
(every kind present, with the statuses test_gpu_abi_buffers.py relies on, and
cheap enough for the oracle) and Arena itself (addresses, guard sizes, and a
planted one-byte write on each side of a region found and named)."""
import numpy as np
import pytest
import torch

import abi_arena as A
import count_cases as C
from oracle import oracle as O


def test_pool_is_cheap_and_complete():
    P = A.pool()
    print(f"oracle: {P['seconds']:.2f} s for {len(P['boards'])} boards, both orders")
    assert P["seconds"] < 5.0
    boards, kind = P["boards"], P["kind"]
    count = {name: int((kind == i).sum()) for i, name in enumerate(A.KINDS)}
    assert count == {"hard17": 256, "gen": 256, "dead": 49, "clash": 64, "invalid": 8, "single": 2}
    clean = np.array([not C.givens_clash(g) for g in boards])
    for order in ("gen", "node"):
        rows, st = P["want"][order]
        of = {name: st[kind == i] for i, name in enumerate(A.KINDS)}
        assert (of["hard17"] == 1).all() and (of["gen"] == 1).all() and (of["single"] == 1).all()
        assert (of["dead"] == 0).all() and (of["invalid"] == -1).all()
        assert set(of["clash"]) == {0, 1}, "the walk solves some clashing boards and not others"
        print(f"{order}: the walk 'solves' {int((of['clash'] == 1).sum())} of 64 clashing boards")
        # unsolved rows are the input; solved ones are full and keep the givens
        assert np.array_equal(rows[st != 1], boards[st != 1])
        solved = st == 1
        assert (rows[solved] != 0).all()
        assert (rows[solved][boards[solved] != 0] == boards[solved][boards[solved] != 0]).all()
        # ... and are valid grids exactly where the givens are clean
        valid = np.array([O.check(g) for g in rows[solved]])
        assert np.array_equal(valid, clean[solved])
    g = A.kind_indices("gen")
    empties = (boards[g] == 0).sum(axis=1)
    assert empties.min() == 30 and empties.max() == 55
    assert clean[A.kind_indices("dead")].all() and not clean[A.kind_indices("clash")].any()
    assert np.array_equal(boards[A.kind_indices("clash")[0]], A._b81(A.CLASH))
    assert sorted(set(boards[A.kind_indices("invalid")].max(axis=1))) == [10, 255]
    # both walks agree on one-completion boards only: the generated ones tell the orders apart
    assert not np.array_equal(P["want"]["gen"][0][g], P["want"]["node"][0][g])


def test_mixed_batches_cover_every_kind():
    kind = A.pool()["kind"]
    for n in (65, 257, 2049):
        idx = A.mixed(n)
        assert idx.shape == (n,) and np.array_equal(idx, A.mixed(n))
        if n >= 257:
            assert set(kind[idx]) == set(range(len(A.KINDS)))
        if n >= len(kind):
            assert len(np.unique(idx)) == len(kind)
    only = A.mixed(300, kinds=("clash",))
    assert (kind[only] == A.KINDS.index("clash")).all()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_arena_addresses_and_planted_writes(offset):
    a = A.Arena("cpu", A.OUT_FILL, 1 << 16)
    first = a.carve(81 * 5, offset, name="first")
    st = a.carve(4 * 5, itemsize=4, name="status")
    off = a.carve(8 * 6, itemsize=8, name="offsets")
    rows = a.boards(3, (offset + 1) % 4, name="rows")
    scratch = a.carve(1000, align=256, name="scratch")
    assert first.data_ptr() % 4 == offset and rows.data_ptr() % 4 == (offset + 1) % 4 and rows.shape == (3, 81)
    assert st.dtype == torch.int32 and st.data_ptr() % 4 == 0 and st.shape == (5,)
    assert off.dtype == torch.int64 and off.data_ptr() % 8 == 0 and off.shape == (6,)
    assert scratch.data_ptr() % 256 == 0
    spans = [(0, 0)] + [(s, e) for s, e, _ in a.regions] + [(a.buf.numel(), a.buf.numel())]
    assert all(b[0] - p[1] >= A.GUARD for p, b in zip(spans, spans[1:]))
    # writes inside the regions are the caller's business
    for v in (first, st, off, rows, scratch):
        v.fill_(7)
    a.assert_guards()
    assert a.first_damage() is None
    for s, e, name in a.regions:
        for at, side in ((s - 1, "before"), (e, "after")):
            a.buf[at] = 0
            hit = a.first_damage()
            assert hit == (at, 0, name, side, 1), (name, side, hit)
            with pytest.raises(AssertionError, match=f"1 byte\\(s\\) {side} region {name}"):
                a.assert_guards()
            a.buf[at] = A.OUT_FILL
    # far from any region: the nearest one is named, with the distance
    a.buf[a.regions[0][0] - 200] = 1
    assert a.first_damage()[2:] == ("first", "before", 200)
    a.buf[a.regions[0][0] - 200] = A.OUT_FILL
    a.buf[a.regions[-1][1] + 255] = 1
    assert a.first_damage()[2:] == ("scratch", "after", 256)
    with pytest.raises(ValueError):
        A.Arena("cpu", 0, 1024).carve(600)
