"""Write tests/golden/canon_cases.json: boards with their canonical form.

    python tests/golden/make_canon_cases.py

Every `canon` comes from the repository's own CPU tool and from nothing else:
scripts/hard17/hard17_search.c, `hard17_search --canon`, one board per
invocation (the tool drops duplicate outputs, and two of these boards share a
class on purpose).  The boards:

  empty, one clue, two clues (one row / one box / unrelated);
  8 full grids: the cyclic (3*(r%3) + r//3 + c) % 9 + 1 and seven generate_batch
    grids from tests/golden/random_generated.npz;
  16 puzzles of those grids with 24..40 clues;
  8 boards of random bytes 0..9 (they break the rules);
  8 hard_search_seeds();
  a 17-clue board and one of its symmetry images.
"""
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
TOOL_SRC = os.path.join(ROOT, "scripts", "hard17", "hard17_search.c")
OUT = os.path.join(HERE, "canon_cases.json")


def build_tool(tmp):
    exe = os.path.join(tmp, "hard17_search")
    subprocess.run(["gcc", "-O3", "-fopenmp", "-o", exe, TOOL_SRC], check=True)
    return exe


def tool_canon(exe, board):
    """hard17_search --canon on one board (an 81-digit string)."""
    out = subprocess.run([exe, "--canon"], input=board + "\n", check=True, capture_output=True, text=True,
                         env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.split()
    assert len(out) == 1 and len(out[0]) == 81, out
    return out[0]


def text(b):
    return "".join(str(int(x)) for x in b)


def boards():
    from sudoku_solver_distributed_amd import gen
    rng = np.random.default_rng(20251)
    cases = []

    def sparse(name, *cells):
        b = np.zeros(81, dtype=np.uint8)
        for cell, v in cells:
            b[cell] = v
        cases.append((name, b))

    sparse("empty")
    sparse("one_clue", (40, 7))
    sparse("two_clues_row", (30, 4), (34, 9))
    sparse("two_clues_box", (30, 4), (40, 9))
    sparse("two_clues_unrelated", (0, 4), (40, 4))
    grids = [np.array([(3 * (r % 3) + r // 3 + c) % 9 + 1 for r in range(9) for c in range(9)], dtype=np.uint8)]
    z = np.load(os.path.join(HERE, "random_generated.npz"))
    assert (z["gen_status_30"][:7] == 1).all()
    grids += [z["gen_solutions_30"][k] for k in range(7)]
    for k, g in enumerate(grids):
        assert (g > 0).all()
        cases.append(("cyclic_grid" if k == 0 else f"grid_{k}", g))
    for k in range(16):
        clues = 24 + k + (k > 0)  # 24, 26, 27, ..., 40
        p = grids[k % 8].copy()
        p[rng.permutation(81)[clues:]] = 0
        assert (p > 0).sum() == clues
        cases.append((f"puzzle_{clues}", p))
    for k in range(8):
        cases.append((f"random_bytes_{k}", rng.integers(0, 10, size=81).astype(np.uint8)))
    for k, s in enumerate(gen.hard_search_seeds()[:8]):
        cases.append((f"hard_search_{k}", np.array([int(c) for c in s], dtype=np.uint8)))
    base = np.array([[int(c) for c in gen.SEEDS_17[2]]], dtype=np.uint8)
    cases.append(("pair_a", base[0]))
    cases.append(("pair_b", gen._symmetry_images(base, 1, 77)[0]))
    return cases


def main():
    cases = boards()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_tool(tmp)
        with ThreadPoolExecutor(8) as ex:
            canons = list(ex.map(lambda c: tool_canon(exe, text(c[1])), cases))
    by_name = dict(zip((c[0] for c in cases), canons))
    assert by_name["one_clue"] == "0" * 80 + "1"
    assert by_name["pair_a"] == by_name["pair_b"]
    doc = {"source": "scripts/hard17/hard17_search.c --canon, one board per invocation (make_canon_cases.py)",
           "cases": [{"name": n, "board": text(b), "canon": c} for (n, b), c in zip(cases, canons)]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
