"""Write tests/golden/root_full_cases.json: boards whose root propagation
(rules A-D of csrc/plane_solver.h, no guess) ends with every cell single and
is NOT a completion -- the boards on which the plane kernel's root rule
(search_step_impl's root_full) takes a false answer and the outbox flush's
plane::grid_complete has to reject it.

    python tests/golden/make_root_full_cases.py

A seeded search with the host entry (tests/native/rootfull_host.cpp
rootfull_compare): shuffle a valid grid, blank 25-49 cells, change one
remaining given to a digit no remaining peer of it holds (so the givens do not
clash, and the board has no completion in most cases), and keep the boards
that end by the rule and are rejected.  Every kept board must have no
completion by the oracle's counter.  The host model sets boards with clashing
givens aside before it propagates, so this search finds none of those; the
GPU tests add a clashing board of their own.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import root_full_cases as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 20261
WANT = 40
BATCH = 20000
FULL = "897124635531679284642385179154293867289716453376458912923867541765941328418532796"
PEERS = [[j for j in range(81) if j != i and (j // 9 == i // 9 or j % 9 == i % 9 or
                                             (j // 27 == i // 27 and (j % 9) // 3 == (i % 9) // 3))] for i in range(81)]


def shuffled(rng):
    """A valid grid: FULL under a random digit relabelling, row / column
    permutations within bands / stacks, band / stack permutations, transpose."""
    g = np.array([int(c) for c in FULL]).reshape(9, 9)
    g = np.concatenate([[0], rng.permutation(9) + 1])[g]
    rows = np.concatenate([3 * b + rng.permutation(3) for b in rng.permutation(3)])
    cols = np.concatenate([3 * b + rng.permutation(3) for b in rng.permutation(3)])
    g = g[rows][:, cols]
    return (g.T if rng.integers(2) else g).reshape(81).astype(np.uint8)


def candidate(rng):
    g = shuffled(rng)
    g[rng.choice(81, int(rng.integers(25, 50)), replace=False)] = 0
    kept = np.nonzero(g)[0]
    for cell in rng.permutation(kept):
        held = {int(g[j]) for j in PEERS[cell]} | {int(g[cell])}
        free = [d for d in range(1, 10) if d not in held]
        if free:
            g[cell] = free[int(rng.integers(len(free)))]
            return g
    return None


def main():
    rng = np.random.default_rng(SEED)
    found, tries = [], 0
    while len(found) < WANT:
        boards = [b for b in (candidate(rng) for _ in range(BATCH)) if b is not None]
        tries += BATCH
        boards = np.array(boards, dtype=np.uint8)
        r = R.compare(boards)
        hit = np.nonzero((r["by_rule"] == 1) & (r["rejected"] == 1))[0]
        found.extend(boards[i] for i in hit)
        print(f"{tries} tries: {len(found)} boards")
    found = np.array(found[:WANT], dtype=np.uint8)
    _, cnt = O.solve_unique_batch(found)
    assert (cnt == 0).all()
    doc = {"source": "tests/golden/make_root_full_cases.py: seed %d, the first %d hits of %d tries; board: one digit "
                     "a cell; count: the oracle's completions" % (SEED, WANT, tries),
           "cases": [{"board": "".join(str(int(c)) for c in b), "count": 0} for b in found]}
    with open(R.FIXTURE, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(found)} cases -> {os.path.relpath(R.FIXTURE, ROOT)}")


if __name__ == "__main__":
    main()
