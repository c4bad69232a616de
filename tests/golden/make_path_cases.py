"""Write tests/golden/path_cases.json and path_cases.npz: states (a subset of
logic_cases' states and its five Hall violations) with their solving paths
under the rule masks of path_cases.MASKS.

    python tests/golden/make_path_cases.py

Every answer comes from tests/path_cases.py, the definition in plain Python,
and from nothing else (the states are spread over the machine's cores).  The
runs:

  run 0       every state under ALL;
  runs 1..3   every fourth state, and the violations, under N|H|L, N|S4|F4
              and N|L;
  run 4       the same states under ALL with max_rounds = 2.

The JSON holds the names, the runs' masks and the facts the coverage asserts
below establish; the npz the states (boards, start, has_board, has_start) and
per run k idx_k (the states run), status_k, rounds_k, hist_k, marks_k,
offsets_k and events_k (sorted per state, path_cases.COLUMNS).
"""
import json
import os
import sys
from collections import Counter
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logic_cases as G  # noqa: E402
import path_cases as P  # noqa: E402

PER_STEP = 6      # boards of every first solving step
PER_PLANT = 3     # planted states of every (kind, size)
CUT = 2           # run 4's max_rounds


def _run(arg):
    board, start, rules, max_rounds = arg
    return P.path(board, start, rules, max_rounds)


def select(fx):
    """Indices into logic_cases' fixture: PER_STEP boards of every step, every
    board the X-wing or the swordfish / jellyfish step removes candidates on,
    PER_PLANT planted states of every kind and size."""
    board = fx["kind"] == ""
    sel = [np.nonzero(board & (fx["step"] == k))[0][:PER_STEP] for k in range(9)]
    sel.append(np.nonzero(board & (fx["left"][:, 5] != fx["left"][:, 4]))[0])
    sel.append(np.nonzero(board & (fx["left"][:, 6] != fx["left"][:, 5]))[0])
    for kind in G.KINDS:
        for k in (2, 3, 4):
            sel.append(np.nonzero((fx["kind"] == kind) & (fx["k"] == k))[0][:PER_PLANT])
    return np.unique(np.concatenate(sel))


def main():
    fx = G.load_fixture()
    sel = select(fx)
    names = [fx["names"][i] for i in sel]
    boards = [fx["boards"][i] for i in sel]
    starts = [fx["start"][i] for i in sel]
    has_board = [bool(fx["has_board"][i]) for i in sel]
    has_start = [bool(fx["has_start"][i]) for i in sel]
    first_violation = len(names)
    for name, (start, _) in G.violations().items():
        names.append(name)
        boards.append(np.zeros(81, np.uint8))
        starts.append(np.array(start, dtype=np.uint16))
        has_board.append(False)
        has_start.append(True)
    n = len(names)
    quarter = sorted(set(range(0, first_violation, 4)) | set(range(first_violation, n)))
    runs = [(P.ALL, 0, list(range(n)))] + [(m, 0, quarter) for m in P.MASKS[1:]] + [(P.ALL, CUT, quarter)]
    jobs = [(boards[i] if has_board[i] else None, starts[i] if has_start[i] else None, rules, mr)
            for rules, mr, idx in runs for i in idx]
    with Pool(os.cpu_count() or 1) as pool:
        answers = pool.map(_run, jobs, chunksize=2)
    arrays = {"boards": np.array(boards, dtype=np.uint8), "start": np.array(starts, dtype=np.uint16),
              "has_board": np.array(has_board), "has_start": np.array(has_start)}
    at = 0
    classes, dirs, sizes, statuses = Counter(), Counter(), Counter(), Counter()
    size1 = hall_dead = many = cut = 0
    full = {}
    for k, (rules, mr, idx) in enumerate(runs):
        mine = answers[at:at + len(idx)]
        at += len(idx)
        arrays[f"idx_{k}"] = np.array(idx, dtype=np.int64)
        arrays[f"status_{k}"] = np.array([a[1] for a in mine], dtype=np.int32)
        arrays[f"rounds_{k}"] = np.array([a[2] for a in mine], dtype=np.int32)
        arrays[f"hist_{k}"] = np.array([a[3] for a in mine], dtype=np.int32)
        arrays[f"marks_{k}"] = np.array([a[4] for a in mine], dtype=np.uint16)
        arrays[f"offsets_{k}"] = np.cumsum([0] + [len(a[0]) for a in mine]).astype(np.int64)
        arrays[f"events_{k}"] = np.array([e for a in mine for e in a[0]], dtype=np.int32).reshape(-1, 8)
        for i, a in zip(idx, mine):
            statuses[a[1]] += 1
            if k == 0:
                full[i] = a
            if mr and a[1] == P.LIMITED and full[i][2] > mr:
                cut += 1
            per_round = Counter()
            for rnd, cls, m, I, u, removed, left, contra in a[0]:
                if contra:
                    size1 += cls == 0
                    hall_dead += cls >= 3
                    continue
                assert removed > 0
                classes[cls] += 1
                if m >= 72:
                    dirs[m - 72] += 1
                else:
                    sizes[m // 9, P.CLASS_SIZE[cls]] += 1
                    per_round[rnd, m] += 1
            many += any(sum(1 for (r2, _) in per_round if r2 == r) >= 2 for (r, _) in per_round)
    # ---- the coverage the tests rely on
    assert set(classes) == set(range(9)), classes                       # an effective event of every class
    assert set(dirs) == {0, 1}, dirs                                    # both L directions
    want = {(kind, k) for kind in (0, 1) for k in (2, 3, 4)} | {(kind, k) for kind in range(2, 8) for k in (1, 2, 3, 4)}
    assert want <= set(sizes), sorted(want - set(sizes))                # every matrix kind at every size it has
    assert set(statuses) >= {P.DEAD, P.SOLVED, P.STUCK, P.LIMITED}, statuses
    assert size1 and hall_dead and many and cut, (size1, hall_dead, many, cut)
    facts = {"states": n, "events_by_class": [classes[c] for c in range(9)], "l_directions": [dirs[0], dirs[1]],
             "size1_contradictions": size1, "hall_contradictions": hall_dead, "boards_with_parallel_events": many,
             "boards_cut_mid_path": cut, "status_tally": {str(k): v for k, v in sorted(statuses.items())}}
    doc = {"source": "tests/path_cases.py path(board, start, rules, max_rounds) (make_path_cases.py); the arrays: path_cases.npz",
           "columns": list(P.COLUMNS), "names": names,
           "runs": [{"rules": rules, "max_rounds": mr, "states": len(idx)} for rules, mr, idx in runs], "facts": facts}
    with open(os.path.join(HERE, "path_cases.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "path_cases.npz"), **arrays)
    print(json.dumps(facts))
    print(n, "states,", sum(len(a[0]) for a in answers), "events,", os.path.getsize(os.path.join(HERE, "path_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
