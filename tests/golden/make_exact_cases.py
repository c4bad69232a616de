"""Write tests/golden/exact_cases.json: exact completion counts recorded on
the CPU from the oracle's counter, O.count_solutions(board, 2**31 - 1).

    python tests/golden/make_exact_cases.py

  b       the 256 boards of count_cases.sets()["b"] (17 clues minus one), in order
  h1, h2  the two heavy boards of exact_cases.heavy(): the oracle's solve of
          the empty board with 62 / 63 seeded cells erased; their counts are
          asserted here, so that a drifted grid is noticed

Sets c-f are cheap and the tests count them live.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import count_cases as C  # noqa: E402
import exact_cases as E  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    doc = {"source": "oracle.count_solutions(board, 2**31 - 1) (make_exact_cases.py); b: count_cases.sets()['b'] in "
                     "order; h1, h2: exact_cases.heavy(62), heavy(63), one digit a cell"}
    for key, k, want in (("h1", E.H1_ERASED, E.H1_COUNT), ("h2", E.H2_ERASED, E.H2_COUNT)):
        g = E.heavy(k)
        t = time.time()
        c = O.count_solutions(g, E.NO_LIMIT)
        print(f"{key}: {c} completions, {time.time() - t:.1f} s")
        assert c == want, (key, c, want)
        doc[key] = {"board": "".join(str(int(v)) for v in g), "count": int(c)}
    t = time.time()
    doc["b"] = [int(O.count_solutions(g, E.NO_LIMIT)) for g in C.sets()["b"]]
    print(f"b: {len(doc['b'])} boards, {min(doc['b'])} .. {max(doc['b'])} completions, {time.time() - t:.1f} s")
    with open(E.FIXTURE, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('],"', '],\n"').replace('},"', '},\n"') + "\n")
    print(f"-> {os.path.relpath(E.FIXTURE, ROOT)} ({os.path.getsize(E.FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
