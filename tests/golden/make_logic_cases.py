"""Write tests/golden/logic_cases.json and logic_cases.npz: states with their
name and step (the JSON) and their open and left counts, pencil marks and
candidate marks (the arrays `open`, `left`, `start` and `marks` of the npz, a
row a state in the JSON's order) at the default ladder.

    python tests/golden/make_logic_cases.py

Every answer comes from tests/logic_cases.py, the definition in plain Python,
and from nothing else (the states are spread over the machine's cores).  The
states:

  every board of rate_cases.json, read from that file and named, not copied;
  planted states (logic_cases.planted): for each of naked, hidden, row_fish,
    col_fish and k = 2, 3, 4 the first PER seeds whose first change of `left`
    is at the pattern's own step of the default ladder;
  the Hall violations of logic_cases.violations(), under their ladders.
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
import rate_cases as R  # noqa: E402

OUT = os.path.join(HERE, "logic_cases.json")
PER = 16
DRAWS = 96  # seeds tried per (kind, k)


def _board(board):
    return G.logic(R.digits(board), None)


def _planted(arg):
    kind, k, seed = arg
    start = G.planted(kind, k, seed)
    ans = G.logic(None, start)
    return start, ans, G.first_change(sum(G.POP[m] for m in start), ans[2])


def _violation(arg):
    start, ladder = arg
    return G.logic(None, start, ladder)


def main():
    with open(os.path.join(HERE, "rate_cases.json")) as f:
        rate = json.load(f)["cases"]
    draws = [(kind, k, seed) for kind in G.KINDS for k in (2, 3, 4) for seed in range(DRAWS)]
    viol = G.violations()
    runs = [(name, start, list(ladder)) for name, (start, ladders) in viol.items() for ladder in ladders]
    with Pool(os.cpu_count() or 1) as pool:
        answers = pool.map(_board, [c["board"] for c in rate], chunksize=4)
        drawn = pool.map(_planted, draws, chunksize=4)
        viol_answers = pool.map(_violation, [(s, l) for _, s, l in runs])
    # (the boards themselves stay in rate_cases.json: load_fixture finds them by name)
    cases = [{"name": c["name"], "step": a[0]} for c, a in zip(rate, answers)]
    kept, starts = list(answers), [[G.ALL] * 81 for _ in answers]
    print("first solving step:", dict(sorted(Counter(a[0] for a in answers).items())))
    # steps 1..3 are the rating's levels 1..3
    for c, a in zip(rate, answers):
        want = R.at_level(c["rating"], c["open"], 3)
        if want[0] != 4:
            assert a[0] == want[0] and (a[0] == 0 or a[1][:3] == want[1][:3]), c["name"]
    passed = Counter()
    for (kind, k, seed), (start, a, first) in zip(draws, drawn):
        passed[kind, k] += first == G.pattern_step(kind, k)
        if first == G.pattern_step(kind, k) and sum(c.get("kind") == kind and c.get("k") == k for c in cases) < PER:
            cases.append({"name": f"{kind}_{k}_{seed}", "kind": kind, "k": k, "step": a[0]})
            kept.append(a)
            starts.append(start)
    print("planted draws that pass, of", DRAWS, ":", dict(passed))
    for kind in G.KINDS:
        for k in (2, 3, 4):
            assert sum(c.get("kind") == kind and c.get("k") == k for c in cases) == PER, (kind, k)
    violations = []
    for name, (start, ladders) in viol.items():
        mine = [(l, a) for (n, _, l), a in zip(runs, viol_answers) if n == name]
        assert mine[0][1][0] != 0 or name == "two_cells_one_digit", name   # the first ladder does not see it
        assert mine[-1][1][0] == 0, name                                   # the last one does
        violations.append({"name": name, "start": G.marks_text(start),
                           "runs": [{"ladder": l, "step": a[0], "open": a[1], "left": a[2], "marks": G.marks_text(a[3])}
                                    for l, a in mine]})
        print(name, [(l, a[0]) for l, a in mine])
    doc = {"source": "tests/logic_cases.py logic(board, start, ladder) (make_logic_cases.py); open, left, start and marks of the cases: "
                     "logic_cases.npz; of the violations: three hex digits a cell",
           "ladder": G.DEFAULT_LADDER, "cases": cases, "violations": violations}
    # one line a state
    line = lambda x: json.dumps(x, separators=(",", ":"))
    with open(OUT, "w") as f:
        f.write('{"source":%s,\n"ladder":%s,\n"cases":[\n' % (line(doc["source"]), line(doc["ladder"])))
        f.write(",\n".join(line(c) for c in cases))
        f.write('\n],\n"violations":[\n')
        f.write(",\n".join(line(v) for v in violations))
        f.write("\n]}\n")
    np.savez_compressed(os.path.join(HERE, "logic_cases.npz"), start=np.array(starts, dtype=np.uint16),
                        open=np.array([a[1] for a in kept], dtype=np.int32), left=np.array([a[2] for a in kept], dtype=np.int32),
                        marks=np.array([a[3] for a in kept], dtype=np.uint16))
    print(f"{len(cases)} cases, {len(violations)} violations -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
