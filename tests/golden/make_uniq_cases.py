"""Write tests/golden/uniq_cases.json: the boards of cand_cases.json (same
names, same order) with, per cell, the digits exactly one valid completion
puts there (once), the digits at least one does (marks) and the count the
marks imply (0, 1, 2 = several; -1 for a byte > 9).

    python tests/golden/make_uniq_cases.py

Every answer comes from the oracle's counter asked once per empty cell and
digit at limit 2 (tests/uniq_cases.py oracle_once), on the CPU, spread over the
machine's cores.  Before anything is written the recorded marks and counts
must equal cand_cases.json's, and once must be a subset of marks.

Cost condition (uniq_cases.PASS_BUDGET): the host build of plane_uniq.h
(tests/native/uniq_host.cpp) at the default sweep is run on every board and
its passes are printed; a board of a set a-e over the budget is replaced by
the next board of its set that is not in the fixture and is within the budget
(such a board has no row in cand_cases.json and is checked against
cand_cases.oracle_marks instead).  At least 8 set-b boards and the empty board
must remain.
"""
import ctypes
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cand_cases as K  # noqa: E402
import count_cases as C  # noqa: E402
import native_build  # noqa: E402
import uniq_cases as U  # noqa: E402

_vp = ctypes.c_void_p
native_build.PROTOS.setdefault("uniq_host", {
    "uniq_host_batch": ([_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp], None)})


def host_passes(boards):
    """Passes of the host model per board, at the compiled (default) sweep."""
    lib = native_build.host_lib("uniq_host")
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    once = np.zeros((n, 81), dtype=np.uint16)
    passes = np.zeros(n, dtype=np.uint64)
    lib.uniq_host_batch(boards.ctypes.data, once.ctypes.data, None, None, n, 81, 0, None, passes.ctypes.data)
    return passes


def main():
    names, boards, marks, count = K.load_fixture()
    names, boards = list(names), boards.copy()
    passes = host_passes(boards)
    sets = C.sets()
    swapped = set()
    for k in np.nonzero(passes > U.PASS_BUDGET)[0]:
        key = names[k].split("_")[0]
        if key not in "abcde" or len(key) != 1:
            raise SystemExit(f"{names[k]} takes {passes[k]} passes (budget {U.PASS_BUDGET}) and has no set to replace it from")
        used = {int(n.split("_")[1]) for n in names if n.startswith(key + "_")}
        for i in range(len(sets[key])):
            if i not in used and host_passes(sets[key][i])[0] <= U.PASS_BUDGET:
                print(f"{names[k]}: {passes[k]} passes, replaced by {key}_{i}")
                names[k], boards[k], passes[k] = f"{key}_{i}", sets[key][i], host_passes(sets[key][i])[0]
                swapped.add(k)
                break
        else:
            raise SystemExit(f"no board of set {key} within the budget")
    for n, p in zip(names, passes):
        print(f"{n:28s} {int(p):7d} passes")
    print(f"most: {int(passes.max())} ({names[int(passes.argmax())]}), budget {U.PASS_BUDGET}; "
          f"mean {passes.mean():.1f}")
    assert sum(n.startswith("b_") for n in names) >= 8 and "f_empty" in names
    assert (passes <= U.PASS_BUDGET).all()

    with Pool(os.cpu_count() or 1) as pool:
        answers = pool.map(U.oracle_once, list(boards), chunksize=1)
    for k, (name, (once, m, c)) in enumerate(zip(names, answers)):
        want_m, want_c = K.oracle_marks(boards[k]) if k in swapped else (marks[k].tolist(), int(count[k]))
        assert m == list(want_m) and c == want_c, (name, c, want_c)
        assert not any(o & ~w for o, w in zip(once, m)), name
    doc = {"source": "tests/uniq_cases.py oracle_once(board) (make_uniq_cases.py) on the boards of cand_cases.json; "
                     "board: one hex digit a cell, once / marks: three hex digits a cell",
           "cases": [{"name": n, "board": K.board_text(b), "once": K.marks_text(o), "marks": K.marks_text(m), "count": int(c)}
                     for n, b, (o, m, c) in zip(names, boards, answers)]}
    with open(U.FIXTURE, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(names)} cases -> {os.path.relpath(U.FIXTURE, ROOT)}")


if __name__ == "__main__":
    main()
