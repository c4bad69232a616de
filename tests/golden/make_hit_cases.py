"""Write tests/golden/hit_cases.json: families of cell sets with allowed and
required masks and their k-cell hitting sets as the tests use
them.

    python tests/golden/make_hit_cases.py

csrc/hit.h has no part in it.  Every answer comes from hit_cases.brute_rows
(all k-subsets of A that hold R, at most 2^20 of them a case) where that
applies, and from hit_cases.restated_rows / restated_count (cell c in or out,
in cell order) otherwise; wherever both run they are asserted equal here.  A
case records the number of its rows and their sha256; up to hit_cases.LIST_CAP
rows are listed as well, in tests/golden/hit_cases.npz.

The families: the cyclic grid's 81 six-cell sets; the minimal unavoidable sets
at 6 and at 12 cells of the first four hard17_classes grids and the first four
random_grids(seed = 1) grids (read from ua_cases.npz by name), with A the
cells of a recorded superset Q, 20..24 clues, of a proper puzzle P of the grid
(P: the 17-clue puzzle, or the grid minimised by count_host_batch in a seeded
order); the empty family; one one-cell set; a set of all 81 cells; a set
outside A; an all-zero mask; a duplicated set; a shuffled copy; sets, A and R
on cells 0, 31, 32, 63, 64 and 80; k = |R|, |A|, |A| + 1, < |R| and 0;
R outside A and a bit 81 in A or R; and per real grid tau -- the least k with
a row at A = all cells, R empty, sets at 6 -- with the number of rows there.
A few minutes.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import hit_cases as H  # noqa: E402
import native_build  # noqa: E402
import ua_cases as U  # noqa: E402

OUT = os.path.join(HERE, "hit_cases.json")
OUT_ROWS = os.path.join(HERE, "hit_cases.npz")
REAL = [f"hard17_{k}" for k in range(4)] + [f"random_{k}" for k in range(4)]
EDGE = (0, 31, 32, 63, 64, 80)


def completions(board, limit=2):
    lib = native_build.host_lib("count_host")
    b = np.ascontiguousarray(board, dtype=np.uint8)
    cnt, out = np.zeros(1, dtype=np.int32), np.zeros(81, dtype=np.uint8)
    p, d = ctypes.c_uint64(0), ctypes.c_uint32(0)
    lib.count_host_batch(b.ctypes.data, cnt.ctypes.data, out.ctypes.data, 1, limit, 81, ctypes.byref(p), ctypes.byref(d))
    return int(cnt[0]), out


def proper_puzzle(name, grid):
    """A proper puzzle of `grid`: hard17_k's own 17 clues, else the smallest
    of 40 seeded greedy minimisations."""
    from sudoku_solver_distributed_amd import gen
    if name.startswith("hard17_"):
        p = np.array([int(ch) for ch in gen.hard17_classes()[int(name[7:])]], dtype=np.uint8)
        assert completions(p)[0] == 1 and np.array_equal(completions(p)[1], grid)
        return p
    best = None
    rng = np.random.default_rng(int(name[7:]) + 100)
    for _ in range(40):
        p = np.array(grid, dtype=np.uint8)
        for c in rng.permutation(81):
            v, p[c] = p[c], 0
            if completions(p)[0] != 1:
                p[c] = v
        if best is None or (p != 0).sum() < (best != 0).sum():
            best = p
    return best


def answers(sets, A, R, ks):
    out = {}
    for k in ks:
        rows = H.brute_rows(sets, A, R, k)
        if rows is None or len(sets) <= 200:
            again = H.restated_rows(sets, A, R, k)
            assert rows is None or rows == again, k
            rows = again
        assert H.restated_count(sets, A, R, k) == len(rows), k
        a = {"count": len(rows)}
        if len(rows) <= H.LIST_CAP:
            a["rows"] = ["%x" % m for m in rows]
        else:
            a["digest"] = H.digest(rows)
        out[str(k)] = a
    return out


def write(docs, source):
    """The cases into the JSON file, one line a case, their listed rows into
    the npz file: "<name>/<k>" (count, 11) uint8, a mask as 11 little-endian
    bytes, in ascending cell-list order; the JSON entry keeps their sha256."""
    arrays = {}
    for d in docs:
        for k, a in d["k"].items():
            if "rows" in a:
                masks = [int(x, 16) for x in a.pop("rows")]
                a["digest"] = H.digest(masks)
                arrays["%s/%s" % (d["name"], k)] = np.frombuffer(b"".join(m.to_bytes(11, "little") for m in masks),
                                                                 dtype=np.uint8).reshape(-1, 11)
    with open(OUT, "w") as f:
        f.write('{"source": %s,\n "cases": [\n%s\n]}\n' % (json.dumps(source), ",\n".join(json.dumps(d) for d in docs)))
    np.savez_compressed(OUT_ROWS, **arrays)
    print(f"{len(docs)} cases -> {os.path.relpath(OUT, ROOT)} ({os.path.getsize(OUT)} bytes), "
          f"{os.path.relpath(OUT_ROWS, ROOT)} ({os.path.getsize(OUT_ROWS)} bytes)")


def main():
    by_name = {c.name: c for c in U.load_fixture()}
    docs = []

    def add(name, family, A, R, ks, **more):
        sets = H.family_of(family)
        d = {"name": name, "family": family, "A": "%x" % A, "R": "%x" % R, "status": H.status_of(A, R),
             "k": answers(sets, A, R, ks)}
        d.update(more)
        docs.append(d)
        print(name, len(sets), {k: v["count"] for k, v in d["k"].items()}, more, flush=True)
        return d

    lit = lambda masks: {"sets": ["%x" % m for m in masks]}
    rng = np.random.default_rng(25)
    # the cyclic grid.  Small: A a greedy hitting set (the cell that meets most unhit sets, lowest first) and 8 more cells,
    # R every second cell of the hitting set -- brute force reaches it.  Large: A 64 seeded cells that meet every set, R
    # every third of them -- the restatement alone.
    cyc = by_name["cyclic"].minimal(8)
    assert len(cyc) == 81
    G, left = 0, list(cyc)
    while left:
        c = max(range(81), key=lambda x: (sum(m >> x & 1 for m in left), -x))
        G, left = G | 1 << c, [m for m in left if not m >> c & 1]
    g = H.popcount(G)
    A = G | U.mask_of(rng.permutation([x for x in range(81) if not G >> x & 1])[:8])
    R = U.mask_of(U.cells_of(G)[::2])
    add("cyclic", {"ua": "cyclic", "size": 8}, A, R, (g - 2, g - 1, g, g + 1, g + 2))
    add("cyclic_shuffled", {"ua": "cyclic", "size": 8, "shuffle": 3}, A, R, (g, g + 1))
    add("cyclic_repeats", {"ua": "cyclic", "size": 8, "repeat": [0, 5, 5, 80]}, A, R, (g, g + 1))
    A = 0
    while any(not m & A for m in cyc):
        A |= 1 << int(rng.integers(0, 81))
    R = U.mask_of(U.cells_of(A)[::3])
    k = H.popcount(R)
    while H.restated_count(cyc, A, R, k) == 0:
        k += 1
    add("cyclic_wide", {"ua": "cyclic", "size": 8}, A, R, (k - 1, k))
    # the real grids
    for name in REAL:
        c = by_name[name]
        grid = np.array(c.grid)
        P = proper_puzzle(name, grid)
        clues = int((P != 0).sum())
        assert completions(P)[0] == 1 and clues <= 24, (name, clues)
        extra = rng.permutation(np.nonzero(P == 0)[0])[:min(24, max(22, clues + 1)) - clues]
        Q = U.mask_of(np.nonzero(P)[0]) | U.mask_of(extra)
        assert 20 <= H.popcount(Q) <= 24
        Pm = U.mask_of(np.nonzero(P)[0])
        ks = sorted({clues - 1, clues, clues + 1, H.popcount(Q) - 1})
        for size in (6, 12):
            d = add(f"{name}_at{size}", {"ua": name, "size": size}, Q, 0, ks, puzzle="%x" % Pm)
            rows = [int(s, 16) for s in d["k"][str(clues)].get("rows", [])]
            assert not rows or Pm in rows, name
        keep = U.mask_of(U.cells_of(Pm)[::2])
        add(f"{name}_required", {"ua": name, "size": 12}, Q, keep, (clues, clues + 2), puzzle="%x" % Pm)
        # tau at 6 cells: A every cell, R empty; counted by the memo, listed where few
        sets = c.minimal(6)
        k = 0
        while H.restated_count(sets, H.ALL81, 0, k) == 0:
            k += 1
        n = H.restated_count(sets, H.ALL81, 0, k)
        d = {"name": f"{name}_tau6", "family": {"ua": name, "size": 6}, "A": "%x" % H.ALL81, "R": "0", "status": H.DONE,
             "tau": k, "minimum": n, "k": {}}
        for kk in (k - 1, k):
            a = {"count": H.restated_count(sets, H.ALL81, 0, kk)}
            if a["count"] <= H.LIST_CAP:
                rows = H.restated_rows(sets, H.ALL81, 0, kk)
                assert len(rows) == a["count"]
                a["rows"] = ["%x" % m for m in rows]
            d["k"][str(kk)] = a
        docs.append(d)
        print(d["name"], len(sets), "tau", k, "minimum", n, flush=True)
    # hand-made families
    E = U.mask_of(EDGE)
    A20 = U.mask_of(range(0, 80, 4))
    add("empty_family", lit([]), A20, U.mask_of([0, 4]), (0, 1, 2, 3, 5, 20, 21))
    add("empty_family_all_cells", lit([]), H.ALL81, 0, (0, 1, 2))
    add("one_cell", lit([1 << 40]), A20, 0, (0, 1, 2, 3))
    add("one_cell_required", lit([1 << 40]), A20, 1 << 40, (0, 1, 2))
    add("all_cells", lit([H.ALL81]), E, 0, (0, 1, 3, 6, 7))
    add("outside_allowed", lit([U.mask_of([1, 2, 3]), U.mask_of([0, 4])]), A20, 0, (1, 2, 3))
    add("zero_mask", lit([U.mask_of([0, 4]), 0]), A20, 0, (1, 2))
    add("zero_mask_alone", lit([0]), A20, 0, (0, 1))
    pairs = [U.mask_of([a, b]) for a, b in ((0, 31), (31, 32), (32, 63), (63, 64), (64, 80), (80, 0))]
    add("edge_cells", lit(pairs), E | U.mask_of([8, 40, 72]), 0, (2, 3, 4, 5, 9, 10))
    add("edge_cells_required", lit(pairs), E | U.mask_of([8, 40, 72]), U.mask_of([31, 80]), (1, 2, 3, 4))
    add("edge_cells_repeats", {"sets": ["%x" % m for m in pairs], "repeat": [0, 0, 3], "shuffle": 9},
        E | U.mask_of([8, 40, 72]), 0, (3, 4))
    add("required_all", lit(pairs), E, E, (5, 6, 7))
    add("required_outside", lit(pairs), E, U.mask_of([0, 8]), (2, 3))
    add("bit81_allowed", lit(pairs), E | 1 << 81, 0, (3,))
    add("bit81_required", lit(pairs), H.ALL81 | 1 << 81, 1 << 81, (3,))
    # thirty-two clues: the complement of a 3-cell set inside 34 allowed cells, few rows
    A34 = U.mask_of(range(0, 68, 2))
    add("k32", lit([U.mask_of([0, 2, 4])] + [U.mask_of([c]) for c in range(6, 62, 2)]), A34, 0, (31, 32))
    source = ("make_hit_cases.py: brute force over the k-subsets of A that hold R and the cell-by-cell restatement; a "
              "mask is hex, cell c = bit c; family: {ua: a grid of ua_cases.json, size: its minimal sets of at most that "
              "many cells, in the public order} or {sets: [...]}, then shuffle (a numpy default_rng seed) and repeat "
              "(indices appended); per k the count and the sha256 of the rows in ascending cell-list order; the rows of a case that "
              "lists them are in hit_cases.npz")
    write(docs, source)


if __name__ == "__main__":
    main()
