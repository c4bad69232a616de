"""What the unavoidable-set tests share (test_ua_host.py on the CPU,
test_gpu_ua.py on the GPU): the loader of tests/golden/ua_cases.json and
ua_cases.npz (written by tests/golden/make_ua_cases.py, which csrc/ua.h has
no part in: the JSON file names the grids and tallies their sets by size, the
npz file holds the sets) and the
definitions of DESIGN.md §24 in plain Python -- neighbour, link, connected,
minimal, and the repair search restated.  A cell set is a Python int here,
cell c its bit c; a row of the C ABI is the words {m & M32, m >> 32 & M32,
m >> 64, owner}.  Loaded once per process and shared, never modified.
"""
import functools
import json
import os
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ua_cases.json")
FIXTURE_SETS = os.path.join(HERE, "golden", "ua_cases.npz")
DONE, INVALID, NOT_A_GRID = 1, -1, -2   # SDK_UA_DONE, SDK_INVALID, SDK_UA_NOT_A_GRID
MIN_SIZE, MAX_SIZE = 4, 16              # SDK_UA_MAX_SIZE
M32 = 0xFFFFFFFF

PEERS = [sorted({a for a in range(81)
                 if a != c and (a // 9 == c // 9 or a % 9 == c % 9 or (a // 27 == c // 27 and a % 9 // 3 == c % 9 // 3))})
         for c in range(81)]


def cyclic_grid():
    return np.array([((r % 3) * 3 + r // 3 + c) % 9 + 1 for r in range(9) for c in range(9)], dtype=np.uint8)


def status_of(grid):
    g = [int(v) for v in grid]
    if any(v < 1 or v > 9 for v in g):
        return INVALID
    if any(g[a] == g[c] for c in range(81) for a in PEERS[c]):
        return NOT_A_GRID
    return DONE


def cells_of(mask):
    return [c for c in range(81) if (mask >> c) & 1]


def mask_of(cells):
    m = 0
    for c in cells:
        m |= 1 << int(c)
    return m


def sort_key(mask):
    """The public order within a grid: by size, then the ascending cell list."""
    cells = cells_of(mask)
    return len(cells), cells


def connected(g, g2):
    """Is D(g2) connected under links (the graph definition)?"""
    D = [c for c in range(81) if g[c] != g2[c]]
    if not D:
        return False
    inD = set(D)
    seen, todo = {D[0]}, [D[0]]
    while todo:
        c = todo.pop()
        for a in PEERS[c]:
            if a in inD and a not in seen and (g2[c] == g[a] or g[c] == g2[a]):
                seen.add(a)
                todo.append(a)
    return len(seen) == len(D)


def minimal_flags(masks):
    """Per mask: no OTHER mask of the list is a proper subset of it."""
    distinct = sorted(set(masks), key=lambda m: bin(m).count("1"))
    size = [bin(m).count("1") for m in distinct]
    good = {}
    for k, m in enumerate(distinct):
        good[m] = not any(size[j] < size[k] and distinct[j] & ~m == 0 for j in range(k))
    return [good[m] for m in masks]


def python_rows(grid, m):
    """The rows of `grid` at max_size m as a list of masks (a multiset), by the
    repair search of §24 restated: dicts and sets, recursion, nothing shared
    with csrc/ua.h."""
    g = [int(v) for v in grid]
    rows = []

    def holders(c, d, new):
        return {p for p in PEERS[c] if g[p] == d and p not in new}

    def rec(new, pending, seed):
        if len(new) + len(pending) > m:
            return
        if not pending:
            rows.append(mask_of(new))
            return
        c = min(pending)
        for d in range(1, 10):
            if d == g[c] or any(new.get(p) == d for p in PEERS[c]):
                continue
            add = holders(c, d, new)
            if any(p < seed for p in add):
                continue
            new[c] = d
            rec(new, (pending - {c}) | add, seed)
            del new[c]

    for s in range(81):
        for d in range(1, 10):
            if d == g[s]:
                continue
            add = holders(s, d, {s: d})
            if any(p < s for p in add):
                continue
            rec({s: d}, add, s)
    return rows


def rows_to_words(masks, owner=0):
    """(k, 4) uint32: the C ABI's rows of these masks."""
    return np.array([[m & M32, (m >> 32) & M32, m >> 64, owner] for m in masks], dtype=np.uint32).reshape(-1, 4)


def words_to_masks(rows):
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 32 | int(r[2]) << 64 for r in rows]


def by_owner(rows, n):
    """The rows of a raw list as one Counter of masks per grid."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 4)
    out = [Counter() for _ in range(n)]
    for r, m in zip(rows, words_to_masks(rows)):
        out[int(r[3])][m] += 1
    return out


def grid_text(grid):
    return "".join("%x" % int(v) for v in grid)


def grid_from_text(s):
    return np.array([int(ch, 16) for ch in s], dtype=np.uint8)


class Case:
    """name, grid (81,) uint8, status; for a DONE grid rows12 (Counter of
    masks, the Python restatement at m = 12), enum9 (Counter, the enumeration
    at m = 9) and minimal12 (the set of masks of rows12 that are minimal)."""

    def rows(self, m):
        """The rows at max_size m <= 12 as a Counter."""
        assert m <= 12
        return Counter({k: v for k, v in self.rows12.items() if bin(k).count("1") <= m})

    def minimal(self, m):
        """The minimal sets of at most m <= 12 cells, in the public order."""
        return sorted((k for k in self.minimal12 if bin(k).count("1") <= m), key=sort_key)


def _record(arrays, key, tallies):
    """(Counter of masks, set of the minimal ones) of one record of the npz
    file, checked against the JSON file's tallies by size."""
    sets = [int.from_bytes(bytes(r), "little") for r in arrays[key + "_sets"]]
    mult = [int(v) for v in arrays[key + "_mult"]]
    flags = [int(v) for v in arrays[key + "_minimal"]] if key + "_minimal" in arrays else None
    assert sets == sorted(set(sets), key=sort_key) and len(mult) == len(sets)
    by = {}
    for k, m in enumerate(sets):
        t = by.setdefault(str(bin(m).count("1")), [0, 0, 0])
        t[0] += mult[k]
        t[1] += 1
        t[2] += flags[k] if flags else 0
    assert {k: (v if flags else v[:2]) for k, v in by.items()} == {k: list(v) for k, v in tallies.items()}, key
    return Counter(dict(zip(sets, mult))), {m for m, f in zip(sets, flags or ()) if f}


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/ua_cases.json with ua_cases.npz as a list of Case, in
    file order."""
    with open(FIXTURE) as f:
        doc = json.load(f)["cases"]
    arrays = np.load(FIXTURE_SETS)
    out = []
    for d in doc:
        c = Case()
        c.name, c.grid, c.status = d["name"], grid_from_text(d["grid"]), int(d["status"])
        c.grid.setflags(write=False)
        if c.status == DONE:
            c.rows12, c.minimal12 = _record(arrays, c.name + "_rows12", d["rows12"])
            c.enum9, _ = _record(arrays, c.name + "_enum9", d["enum9"])
        else:
            c.rows12, c.enum9, c.minimal12 = Counter(), Counter(), set()
        out.append(c)
    return out


def valid_cases():
    return [c for c in load_fixture() if c.status == DONE]
