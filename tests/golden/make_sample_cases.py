"""Write tests/golden/sample_cases.json: boards, a seed, keys, and what
sdk_sample_batch must answer for them (out, status).

    python tests/golden/make_sample_cases.py

The answers are the host model's (tests/native/sample_host.cpp: the header
csrc/plane_sample.h compiled with g++ in its default build -- run this without
SDK_HOST_CFLAGS).  A random completion has no oracle to record it from; what
the oracle can say about these rows -- valid, the givens kept, the one
completion where there is one, none where there is none -- test_sample_host.py
checks on its own, and it re-derives every row, so the file cannot go stale.
The groups (sample_cases.GROUPS; boards from count_cases.sets(), one seed):

  z  64 rows of the empty board, made with NULL boards, keys 0..63
  a  a[:32]: 17 clues, one completion
  b  b[:32]: many completions
  d  d[:32] with per_board 4: a few completions, 128 rows
  e  e[:8]: none (status 0, out = input)
  f  the five boards of f: statuses 1, 1, 0, 0, -1
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import native_build  # noqa: E402
import sample_cases as S  # noqa: E402


def main():
    assert not native_build.HOST_FLAGS, "the fixture records the default build"
    lib = native_build.host_lib("sample_host")
    groups = {}
    for name, (src, k, per_board, first_key) in S.GROUPS.items():
        boards = S.group_boards(name)
        out, status = S.host_sample(lib, boards, S.SEED, per_board, first_key, n=k)
        assert len(out) == k * per_board
        groups[name] = {"seed": S.SEED, "first_key": first_key, "per_board": per_board,
                        "boards": None if boards is None else [S.board_text(b) for b in boards],
                        "status": [int(s) for s in status], "out": [S.board_text(g) for g in out]}
    assert tuple(groups["f"]["status"]) == S.F_STATUS and not any(groups["e"]["status"])
    assert all(s == 1 for key in "zabd" for s in groups[key]["status"])
    with open(S.FIXTURE, "w") as f:
        f.write('{"source": %s,\n"groups": {\n' % json.dumps(
            "tests/native/sample_host.cpp in its default build (make_sample_cases.py); boards (null: NULL boards, "
            "every board empty), out: one hex digit a cell; row q of a group is board q // per_board under key "
            "first_key + q"))
        f.write(",\n".join("%s: %s" % (json.dumps(n), json.dumps(g, separators=(",", ":")).replace('","', '",\n"'))
                           for n, g in groups.items()))
        f.write("\n}}\n")
    rows = sum(len(g["out"]) for g in groups.values())
    print(f"{rows} rows -> {os.path.relpath(S.FIXTURE, ROOT)} ({os.path.getsize(S.FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
