"""Write tests/golden/cand_cases.json: boards with their exact candidate
marks (the digits some valid completion puts into each cell) and the count
the marks imply (0, 1, 2 = several; -1 for a byte > 9).

    python tests/golden/make_cand_cases.py

Every answer comes from the oracle's counter asked once per empty cell and
digit (tests/cand_cases.py oracle_marks), on the CPU, spread over the
machine's cores; the boards of set a take their unique completion from
O.solve_unique_batch.  Every count is checked against
O.count_solutions(board, 2) before anything is written.  The boards (seeded,
reproducible): the first 32 / 64 / 64 / 16 of count_cases.sets() a, c, d, e;
16 of b (its first 15 and its costliest board, cand_cases.HEAVY_B); the five
single boards of f; and the first 8 boards of rate_cases.json with rating 5.
"""
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
import rate_cases as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

F_NAMES = ("empty", "full", "full_one_cell_changed", "clash_with_open_cells", "byte_10")


def main():
    sets = C.sets()
    cases = []
    for key, positions in K.TAKE:
        for i in positions:
            cases.append((f"f_{F_NAMES[i]}" if key == "f" else f"{key}_{i}", sets[key][i]))
    names, boards, rating, _, _ = R.load_fixture()
    five = np.nonzero(rating == 5)[0][:K.RATE5]
    assert len(five) == K.RATE5
    cases += [(f"rate5_{names[i]}", boards[i]) for i in five]

    na = len(dict(K.TAKE)["a"])
    assert cases[na - 1][0] == f"a_{na - 1}"
    sols, cnt = O.solve_unique_batch(sets["a"][:na])
    assert (cnt == 1).all()
    answers = [([1 << (int(v) - 1) for v in g], 1) for g in sols]
    with Pool(os.cpu_count() or 1) as pool:
        answers += pool.map(K.oracle_marks, [b for _, b in cases[na:]], chunksize=1)
    for (name, b), (marks, count) in zip(cases, answers):
        if (b > 9).any():
            want = K.INVALID
        elif C.givens_clash(b):
            want = 0
        else:
            want = O.count_solutions(b, 2)
        assert count == want == (K.count_of(marks) if want >= 0 else K.INVALID), (name, count, want)
    by_name = {n: a for (n, _), a in zip(cases, answers)}
    assert by_name["f_empty"] == ([K.ALL] * 81, 2) and by_name["f_byte_10"] == ([0] * 81, K.INVALID)
    doc = {"source": "tests/cand_cases.py oracle_marks(board) (make_cand_cases.py); board: one hex digit a cell, "
                     "marks: three hex digits a cell",
           "cases": [{"name": n, "board": K.board_text(b), "marks": K.marks_text(m), "count": int(c)}
                     for (n, b), (m, c) in zip(cases, answers)]}
    with open(K.FIXTURE, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.relpath(K.FIXTURE, ROOT)}")


if __name__ == "__main__":
    main()
