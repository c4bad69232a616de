"""Which band should the completion count branch in?  (Tooling, not product
code; DESIGN.md §3 "Branching".)

    python scripts/pick_study.py [--boards 20000] [--out profiles/r09/pick_study.json]

Host model (scripts/native/pick_study.cpp over host_model.h): the lane solver
on the look-ahead path, gen order, depth 32, switch to the count at 128 passes,
no root shortcut, with the count's branch rule replaced.  Per rule, on
hard17_batch (seeds 3 and 2024) and on hard_search_batch(8000, seed=5): mean
passes and branch nodes per board, p99 / p99.9 / max passes per board, and
whether every answer is the first rule's.  A rule whose p99.9 or maximum on
the 17-clue sets exceeds the first rule's by more than 10 % fails the cap: a
launch ends with its heaviest boards.

--bench-batch: the benchmark's own batch (hard17_batch(2^20, seed=2024)) with
the root shortcut, rule 0 against rule 4: the prediction for the GPU's
sweeps_per_board and guesses_per_board.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ["first band with a cell of S (before)",
         "most cells of S",
         "fewest undetermined cells",
         "fewest cells of S",
         "fewest cells of S, tie -> most undetermined cells (pick_count_masks)",
         "most undetermined cells",
         "most undetermined cells, tie -> fewest cells of S",
         "rule 4, then the band's row with the fewest cells of S",
         "rule 3, then the band's row with the fewest cells of S"]
# VALU the rule adds to the search step, roughly (three v_bcnt per popcount
# key, compares and selects; a row choice: three masks, three counts, selects)
COST = [0, 10, 10, 10, 16, 10, 16, 30, 24]


def load(tmp):
    so = os.path.join(tmp, "libpick_study.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so,
                           os.path.join(ROOT, "scripts/native/pick_study.cpp")])
    lib = ctypes.CDLL(so)
    lib.pick_study.restype = ctypes.c_int64
    lib.pick_study.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                               ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 4
    return lib


def run(lib, boards, rule, ref, root_full=0, mrv_after=128):
    n = len(boards)
    passes = np.zeros(n, np.uint32)
    g = ctypes.c_uint64()
    differ = lib.pick_study(boards.ctypes.data, n, rule, 0, 32, mrv_after, root_full, passes.ctypes.data,
                            ctypes.byref(g), ref[0].ctypes.data, ref[1].ctypes.data)
    p = passes.astype(np.int64)
    return {"passes_per_board": round(float(p.mean()), 4), "guesses_per_board": round(g.value / n, 4),
            "passes_p99": float(np.percentile(p, 99)), "passes_p999": float(np.percentile(p, 99.9)),
            "passes_max": int(p.max()), "boards_above_40_passes": int((p > 40).sum()),
            "answers_differ_from_rule_0": int(differ)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=20000)
    ap.add_argument("--bench-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles/r09/pick_study.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sudoku_solver_distributed_amd.gen import hard17_batch, hard_search_batch
    sets = {"hard17_seed3": hard17_batch(a.boards, seed=3), "hard17_seed2024": hard17_batch(a.boards, seed=2024),
            "hard_search_8000_seed5": hard_search_batch(8000, seed=5)}
    res = {"what": "host model of the count mode's branch rule (scripts/pick_study.py): look-ahead lane solver, "
                   "gen order, depth 32, switch at 128, no root shortcut",
           "boards_per_hard17_set": a.boards, "rules": {}}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load(tmp)
        for name, t in sets.items():
            b = np.ascontiguousarray(t.cpu().numpy(), dtype=np.uint8)
            ref = (np.zeros_like(b), np.zeros(len(b), np.int32))
            for rule, label in enumerate(RULES):
                r = run(lib, b, rule, ref)
                res["rules"].setdefault(label, {"rule": rule, "valu_added_about": COST[rule]})[name] = r
                print(name, rule, r, flush=True)
        if a.bench_batch:
            b = np.ascontiguousarray(hard17_batch(1 << 20, seed=2024).cpu().numpy(), dtype=np.uint8)
            ref = (np.zeros_like(b), np.zeros(len(b), np.int32))
            res["bench_batch_root_shortcut"] = {
                "boards": len(b), "before": run(lib, b, 0, ref, root_full=1), "pick_count_masks": run(lib, b, 4, ref, root_full=1)}
            print(res["bench_batch_root_shortcut"], flush=True)
    base = res["rules"][RULES[0]]
    for label, r in res["rules"].items():
        r["within_tail_cap"] = all(r[s]["passes_max"] <= 1.1 * base[s]["passes_max"] and
                                   r[s]["passes_p999"] <= 1.1 * base[s]["passes_p999"]
                                   for s in ("hard17_seed3", "hard17_seed2024"))
        r["passes_vs_before"] = {s: round(r[s]["passes_per_board"] / base[s]["passes_per_board"] - 1, 4) for s in sets}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["within_tail_cap"], v["passes_vs_before"]) for k, v in res["rules"].items()}, indent=1))


if __name__ == "__main__":
    main()
