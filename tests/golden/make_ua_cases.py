"""Write tests/golden/ua_cases.json and tests/golden/ua_cases.npz: solution
grids and their unavoidable sets as the tests use them.

    python tests/golden/make_ua_cases.py

The JSON file holds what a reader can check by eye -- names, grids, statuses
and, per grid, how many rows, distinct sets and minimal sets there are of every
size; the sets themselves, some 20 000 masks of 11 bytes, go to the compressed
npz file (ua_cases.load_fixture asserts that the two agree).  csrc/ua.h has no
part in either.  Per valid grid two records:

  enum9: the rows at max_size 9 from ENUMERATION.  A digit that moves appears
    in at least two cells of D, so a neighbour with |D| <= 9 moves at most four
    digits: for each of the C(9, 4) = 126 digit quadruples the 36 cells that
    hold them are erased and enum_host_batch (tests/native/enum_host.cpp,
    pinned by tests/test_enum_host.py) lists every completion; those with
    1 <= |D| <= 9 are kept, deduplicated by g', and those connected by the
    graph definition (ua_cases.connected) are the rows.
  rows12: the rows at max_size 12 from ua_cases.python_rows, the repair search
    restated in plain Python, with the minimal flags by the subset definition
    (ua_cases.minimal_flags).  Asserted here: restricted to at most 9 cells it
    IS enum9, as a multiset.

The grids: the cyclic grid g[r][c] = ((r % 3) * 3 + r // 3 + c) % 9 + 1; the
solutions of the first 12 hard17_classes (count_host_batch's completion); the
first 8 rows of random_grids(seed = 1) as tests/golden/sample_cases.json
records them (group z); a grid with a byte 0, one with a byte 10 and one with
a row repeat.  Asserted: the figures DESIGN.md §24 lists for the cyclic grid,
and a set of 4 or 6 cells in every hard17 grid.  A few minutes.
"""
import ctypes
import json
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import enum_cases as E  # noqa: E402
import native_build  # noqa: E402
import sample_cases  # noqa: E402
import ua_cases as U  # noqa: E402

OUT = os.path.join(HERE, "ua_cases.json")
OUT_SETS = os.path.join(HERE, "ua_cases.npz")
QUADS = [(a, b, c, d) for a in range(1, 10) for b in range(a + 1, 10) for c in range(b + 1, 10) for d in range(c + 1, 10)]


def solution(board):
    lib = native_build.host_lib("count_host")
    b = np.ascontiguousarray(board, dtype=np.uint8)
    cnt, out = np.zeros(1, dtype=np.int32), np.zeros(81, dtype=np.uint8)
    p, d = ctypes.c_uint64(0), ctypes.c_uint32(0)
    lib.count_host_batch(b.ctypes.data, cnt.ctypes.data, out.ctypes.data, 1, 2, 81, ctypes.byref(p), ctypes.byref(d))
    assert cnt[0] == 1
    return out


def enumeration(lib, g):
    """Counter of the D of every connected neighbour of g with |D| <= 9."""
    boards = np.repeat(g[None, :], len(QUADS), axis=0)
    for k, q in enumerate(QUADS):
        boards[k][np.isin(g, q)] = 0
    capacity = 1 << 20
    while True:
        grids, _, _, status, info = E.host_enum(lib, boards, capacity)
        if info["listed"] == info["total"]:
            break
        capacity = info["total"]
    assert (status == E.DONE).all()
    rows = grids[:info["listed"]]
    size = (rows != g[None, :]).sum(axis=1)
    near = np.unique(rows[(size >= 1) & (size <= 9)], axis=0)
    gl = [int(v) for v in g]
    out = Counter()
    for r in near:
        if U.connected(gl, [int(v) for v in r]):
            out[U.mask_of(np.nonzero(r != g)[0])] += 1
    return out, int(info["total"])


def record(arrays, key, counter, flags=None):
    """The sets of a Counter in the public order into `arrays` (masks as 11
    little-endian bytes, multiplicities, minimal flags); returns the tallies by
    size for the JSON file: {size: [rows, distinct sets, minimal sets]}."""
    sets = sorted(counter, key=U.sort_key)
    arrays[key + "_sets"] = np.frombuffer(b"".join(m.to_bytes(11, "little") for m in sets), dtype=np.uint8).reshape(-1, 11)
    arrays[key + "_mult"] = np.array([counter[m] for m in sets], dtype=np.uint8)
    if flags is not None:
        arrays[key + "_minimal"] = np.array([flags[m] for m in sets], dtype=np.uint8)
    by = {}
    for m in sets:
        t = by.setdefault(bin(m).count("1"), [0, 0, 0])
        t[0] += counter[m]
        t[1] += 1
        t[2] += int(bool(flags and flags[m]))
    return {str(k): (v if flags is not None else v[:2]) for k, v in sorted(by.items())}


def main():
    from sudoku_solver_distributed_amd import gen
    lib = native_build.host_lib("enum_host")
    cases = [("cyclic", U.cyclic_grid())]
    for k, s in enumerate(gen.hard17_classes()[:12]):
        cases.append((f"hard17_{k}", solution(np.array([int(ch) for ch in s], dtype=np.uint8))))
    z = sample_cases.load_fixture()["z"]
    assert z["null"] and z["seed"] == 1 and z["first_key"] == 0 and (z["status"][:8] == 1).all()
    for k in range(8):
        cases.append((f"random_{k}", z["out"][k].copy()))
    g0 = cases[1][1]
    zero, ten, rep = g0.copy(), g0.copy(), g0.copy()
    zero[17] = 0
    ten[40] = 10
    rep[1] = rep[0]
    cases += [("byte_0", zero), ("byte_10", ten), ("row_repeat", rep)]

    docs, arrays = [], {}
    for name, g in cases:
        st = U.status_of(g)
        doc = {"name": name, "grid": U.grid_text(g), "status": st}
        if st == U.DONE:
            enum9, listed = enumeration(lib, g)
            rows12 = Counter(U.python_rows(g, 12))
            upto9 = Counter({m: v for m, v in rows12.items() if bin(m).count("1") <= 9})
            assert upto9 == enum9, name
            masks = list(rows12)
            flags = dict(zip(masks, U.minimal_flags(masks)))
            doc["enum9"] = record(arrays, name + "_enum9", enum9)
            doc["rows12"] = record(arrays, name + "_rows12", rows12, flags)
            sizes = Counter(bin(m).count("1") for m in masks if flags[m])
            print(name, listed, sum(enum9.values()), sum(rows12.values()), len(rows12), dict(sorted(sizes.items())), flush=True)
            if name == "cyclic":
                by = lambda m: Counter({k: v for k, v in rows12.items() if bin(k).count("1") <= m})
                assert sum(by(8).values()) == 81 and sum(by(10).values()) == 99 and len(by(10)) == 90
                assert sum(rows12.values()) == 963 and dict(sizes) == {6: 81, 12: 54}
                assert not any(bin(m).count("1") == 4 for m in masks)
            if name.startswith("hard17_"):
                assert sizes[4] + sizes[6] >= 1, name
        else:
            print(name, st, flush=True)
        docs.append(doc)
    source = ("make_ua_cases.py: enum9 from enum_host_batch over the 126 digit quadruples, rows12 from "
              "ua_cases.python_rows; a grid byte is one hex digit; per size [rows, distinct sets] and for rows12 [rows, "
              "distinct sets, minimal sets]; the sets are in ua_cases.npz: <name>_<record>_sets (k, 11) uint8, a mask as 11 "
              "little-endian bytes, cell c = bit c, in the public order; _mult: how many neighbours have that D; "
              "_minimal: 0 / 1")
    with open(OUT, "w") as f:  # one line a case
        f.write('{"source": %s,\n "cases": [\n%s\n]}\n' % (json.dumps(source), ",\n".join(json.dumps(d) for d in docs)))
    np.savez_compressed(OUT_SETS, **arrays)
    print(f"{len(docs)} cases -> {os.path.relpath(OUT, ROOT)}, {os.path.relpath(OUT_SETS, ROOT)}")


if __name__ == "__main__":
    main()
