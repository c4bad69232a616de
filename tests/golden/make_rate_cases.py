"""Write tests/golden/rate_cases.json: boards with their rating, open counts
and candidate marks at max_level 4.

    python tests/golden/make_rate_cases.py

Every answer comes from tests/rate_cases.py, the definition in plain Python,
and from nothing else (about 0.2 s a board; the boards are spread over the
machine's cores).  The boards:

  the 80 lines of data/hard17_classes.txt and the 256 of hard_search_seeds.txt;
  the named boards of rate_cases.NAMED (their rating and open are asserted);
  the first 60 puzzles_30 boards of random_generated.npz;
  one-given mutations of the two corpora (one given changed to another
    digit): the first found whose dead state first shows at level 1, at
    level 2, at level 3 and -- among the first MUTATIONS tried -- at level 4.
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
import rate_cases as R  # noqa: E402

OUT = os.path.join(HERE, "rate_cases.json")
MUTATIONS = 3000


def _rate(board):
    return R.rate(R.digits(board), 4)


def mutations(boards, n, seed=20261):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        b = R.digits(boards[k % len(boards)])
        cell = rng.choice(np.nonzero(b)[0])
        b[cell] = (b[cell] - 1 + rng.integers(1, 9)) % 9 + 1
        out.append("".join(str(int(v)) for v in b))
    return out


def main():
    classes, seeds = R.corpus("hard17_classes.txt"), R.corpus("hard_search_seeds.txt")
    cases = [(f"class_{k}", b) for k, b in enumerate(classes)]
    cases += [(f"seed_{k}", b) for k, b in enumerate(seeds)]
    cases += [(name, b) for name, (b, _, _) in R.NAMED.items()]
    cases += [(f"puzzles_30_{k}", b) for k, b in enumerate(R.puzzles_30(60))]
    muts = mutations(classes + seeds, MUTATIONS)
    with Pool(os.cpu_count() or 1) as pool:
        answers = pool.map(_rate, [b for _, b in cases], chunksize=4)
        mut_answers = pool.map(_rate, muts, chunksize=16)
    by_name = {n: a for (n, _), a in zip(cases, answers)}
    for name, (_, rating, opens) in R.NAMED.items():
        assert by_name[name][:2] == (rating, opens), (name, by_name[name][:2])
    tally = lambda p: dict(sorted(Counter(a[0] for (n, _), a in zip(cases, answers) if n.startswith(p)).items()))
    assert tally("class_") == {2: 34, 3: 20, 4: 26}, tally("class_")
    assert tally("seed_") == {3: 34, 4: 222}, tally("seed_")
    assert by_name["class_0"][1] == [63, 0, 0, 0] and by_name["seed_0"][:2] == (4, [57, 54, 54, 0])
    p30 = [a for (n, _), a in zip(cases, answers) if n.startswith("puzzles_30_")]
    # 48 solved by naked singles; 12 with several completions, four cells left open (one of them
    # needs hidden singles to get there: its level 1 leaves 12)
    assert sum(a[0] == 1 for a in p30) == 48 and sum(a[0] == 5 and a[1][1:] == [4, 4, 4] for a in p30) == 12
    assert sorted(a[1][0] for a in p30 if a[0] == 5) == [4] * 11 + [12]
    found = {}
    for b, a in zip(muts, mut_answers):
        if a[0] == 0:
            level = a[1].index(-1) + 1  # the level the dead state first shows at
            if level not in found:
                found[level] = (b, a)
    for level in sorted(found):
        b, a = found[level]
        cases.append((f"mutation_dead_at_level_{level}", b))
        answers.append(a)
    print("mutations:", dict(sorted(Counter(a[0] for a in mut_answers).items())), "dead first seen at levels", sorted(found))
    assert {1, 2, 3} <= set(found)
    doc = {"source": "tests/rate_cases.py rate(board, 4) (make_rate_cases.py); marks: three hex digits a cell",
           "cases": [{"name": n, "board": b, "rating": a[0], "open": a[1], "marks": R.marks_text(a[2])}
                     for (n, b), a in zip(cases, answers)]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
